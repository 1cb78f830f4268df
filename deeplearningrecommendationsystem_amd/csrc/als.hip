// ALS: implicit-feedback matrix factorisation by alternating least squares (Hu, Koren & Volinsky 2008).  A half-sweep
// solves, for every row u of one table with the OTHER table Y fixed and G = Y^T Y,
//     (G + alpha * sum_{i in N(u)} y_i y_i^T + reg I) x_u = (1 + alpha) * sum_{i in N(u)} y_i
// where N(u) is row u of a CSR.  Two kernels on the fp32 matrix cores (v_mfma_f32_16x16x4_f32):
//
//   als_gram       : G = Y^T Y.  A workgroup takes one slab of kSlab rows (a constant, not a function of the CU count)
//                    and leaves its k x k partial in the workspace; a second launch adds the partials in ascending slab
//                    order.  No atomics: G is bitwise reproducible.
//   als_solve_rows : ONE workgroup per output row, never more.
//     (a) the row's list is walked in ascending order in chunks of kChunk entries; the gathered rows of Y are staged
//         in LDS (double buffered, the next chunk's loads in flight under the products) and S += X^T X is accumulated
//         on the matrix cores.  S is symmetric: only the k/16 (k/16 + 1) / 2 tiles on and below the diagonal are
//         formed, dealt round-robin over the four waves.  Both operands of a tile are reads of the same staged rows at
//         two column offsets: lane (r, q) feeds X[e = 4 step + q][16 ta + r] and X[e][16 tb + r]; accumulator
//         register c of lane (r, q) is S[16 ta + 4 q + c][16 tb + r].  The column sum s rides alongside: kGroups
//         threads per column, each over its share of the chunk, met in ascending order at the end.
//     (b) A = G + alpha S + reg I (lower tiles) and b = (1 + alpha) s go to LDS; the stage buffers are dead by then and
//         A takes their place.  b is kept as row k of A: the factorisation's panel step then IS the forward
//         substitution, L y = b.
//     (c) Cholesky blocked by 16, right-looking: the 16 x 16 diagonal block inside one wave (a lane holds a row,
//         pivots travel by shuffle), the panel below it one row per thread, the trailing update
//         A22 -= L21 L21^T on the matrix cores (tile reads and writes in the accumulator layout above).  Then
//         L^T x = y in one wave, x in registers, and the k results are written.
//   No scratch, no per-row global workspace, no (rows, k, k) tensor.  Every sum runs in an order fixed by the row's list
//   alone, so a result is a bitwise function of (list, Y, G, reg, alpha): not of which rows are asked for, in what
//   order, how often, or of the grid.
//
//   als_solve_rows_weighted : the same frame for per-entry weights from a values array aligned with the CSR,
//         (G + sum_e w_e y_e y_e^T + (reg + reg_per_entry n) I) x = sum_e t_e y_e,   w_e = fmaf(w1, v_e, w0),
//         t_e = fmaf(t1, v_e, t0), n the list length, G = gram or 0 (confidences c = 1 + alpha v: (0, alpha, 1, alpha);
//         explicit ratings, Zhou et al. 2008: no G, (1, 0, 0, 1), reg_per_entry).  The chunk's 32 values are read by
//         32 threads beside the row loads (in flight under the products, as the rows are), turned into w_e and t_e
//         (one fused multiply-add each) when the rows are stored, and staged in LDS with them; entries past the end
//         of the list carry w = t = 0 and are not read.  w_e scales ONE
//         operand of each product, the A-side read: lane (r, q) feeds entry 4 step + q, so it keeps the eight weights
//         of its entries in registers for the chunk (two 16-byte LDS reads, the same address over a (., q) group).
//         (w x_a) x_b and x_a (w x_b) round differently, so S is well defined only because every tile on or below the
//         diagonal is formed once and nothing above the diagonal is ever read by (c).  The column sum is
//         sum_e t_e x_e.  Every sum still runs in list order: a row is a bitwise function of (list, values, Y, G, the
//         six scalars).  A non-finite value or scalar ends in the guards below: a zero row and bit 2.
//
// Guards, none of which traps: a CSR index outside [0, y_rows) (or a row id outside the CSR, or a row whose offsets run
// backwards) is never dereferenced, sets bit 1 of *err_flag and gives a zero row; a pivot that is not a positive finite number, or a non-finite result,
// sets bit 2 and gives a zero row.  No NaN or Inf is ever stored.  The flag is OR-ed with the only atomic of the file,
// on the error path alone; it carries no result.
#include <math.h>

#include "ctr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 32;      // list entries (rows of Y) staged at a time
constexpr int kSlab = 512;      // rows of one Gram partial
constexpr int kErrIndex = 1, kErrPivot = 2;

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <int KB>
struct Geo {
  static constexpr int K = 16 * KB;
  static constexpr int K4 = K / 4;
  // stage row stride (floats): the four entry rows a wave reads at once fall into four different bank quarters
  static constexpr int XS = (KB & 1) ? K : K + 16;
  static constexpr int NT = KB * (KB + 1) / 2;              // tiles on and below the diagonal
  static constexpr int TPW = (NT + kWaves - 1) / kWaves;    // ... per wave
  static constexpr int LDA = K + 4;                         // row stride of A: operand reads of (c) hit 64 banks
  static constexpr int kGroups = K <= 16 ? 16 : K <= 32 ? 8 : K <= 64 ? 4 : 2;   // column-sum threads per column
  static constexpr int kPerGroup = kChunk / kGroups;
  static constexpr int kStage = 2 * kChunk * XS;
  static constexpr int kA = (K + 1) * LDA;                  // A and, as row K, b
  static constexpr int kMain = kStage > kA ? kStage : kA;
  static constexpr int kVec = kChunk * K4;                  // float4 of one chunk
  static constexpr int kVecPer = (kVec + kThreads - 1) / kThreads;
};

// the tiles of one wave: tile t = wave + kWaves i of the row-major walk (0,0) (1,0) (1,1) (2,0) ...
template <int KB>
struct Tiles {
  int ta[Geo<KB>::TPW], tb[Geo<KB>::TPW];
  __device__ __forceinline__ explicit Tiles(int wave) {
#pragma unroll
    for (int i = 0; i < Geo<KB>::TPW; ++i) {
      const int t = wave + kWaves * i;
      int a = 0;
      while ((a + 1) * (a + 2) / 2 <= t) ++a;
      ta[i] = a;
      tb[i] = t - a * (a + 1) / 2;
    }
  }
  __device__ __forceinline__ bool live(int i, int wave) const { return wave + kWaves * i < Geo<KB>::NT; }
};

// the per-entry weights of als_accumulate.  NoWeights: every entry counts once, nothing is staged or multiplied.
struct NoWeights {
  static constexpr bool kOn = false;
};
// Weights: entry e of the row counts with w_e = fmaf(w1, values[e], w0) in S and t_e = fmaf(t1, values[e], t0) in the
// column sum.  lds: 2 buffers of 2 kChunk floats, 16-byte aligned; a buffer holds w of entry e at (e % 4) * 8 + e / 4
// -- the eight weights of lane group q are contiguous -- and t of entry e at kChunk + e.
struct Weights {
  static constexpr bool kOn = true;
  const float* values;   // of the row: values[e] for e < n, nothing beyond is read
  float w0, w1, t0, t1;
  float* lds;
};

// S += X^T W X and the column sums sum_e t_e x_e over n gathered rows (W = I, t = 1 without weights); row_of(e): the
// address of entry e's row of Y, or nullptr for a row that counts as zeros.  On return every wave's tiles are in acc,
// a thread's column-sum share in cs, and the stage buffers are dead (the last product is behind a barrier).
template <int KB, typename RowOf, typename Wt>
__device__ __forceinline__ void als_accumulate(int64_t n, RowOf row_of, const Wt& wt, float* __restrict__ stage,
                                               const Tiles<KB>& tiles, f32x4 (&acc)[Geo<KB>::TPW], float& cs) {
  using G = Geo<KB>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t chunks = (n + kChunk - 1) / kChunk;

  f32x4 stg[G::kVecPer];
  // the value of entry c * kChunk + tid (tid < kChunk) and whether the list has that entry; the value stays a load in
  // flight until store() turns it into w and t, as the rows do
  [[maybe_unused]] float val = 0.0f;
  [[maybe_unused]] bool val_live = false;
  auto load = [&](int64_t c) {
#pragma unroll
    for (int i = 0; i < G::kVecPer; ++i) {
      const int v = tid + kThreads * i;
      stg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (v < G::kVec) {
        const int64_t e = c * kChunk + v / G::K4;
        const float* src = e < n ? row_of(e) : nullptr;
        if (src) stg[i] = *(const CTR_GLOBAL f32x4*)(src + 4 * (v % G::K4));
      }
    }
    if constexpr (Wt::kOn) {
      if (tid < kChunk) {
        const int64_t e = c * kChunk + tid;
        val_live = e < n;
        if (val_live) val = wt.values[e];
      }
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G::kVecPer; ++i) {
      const int v = tid + kThreads * i;
      if (v < G::kVec)
        *reinterpret_cast<f32x4*>(stage + buf * kChunk * G::XS + (v / G::K4) * G::XS + 4 * (v % G::K4)) = stg[i];
    }
    if constexpr (Wt::kOn) {
      if (tid < kChunk) {
        float* wb = wt.lds + buf * 2 * kChunk;
        wb[(tid & 3) * (kChunk / 4) + (tid >> 2)] = val_live ? fmaf(wt.w1, val, wt.w0) : 0.0f;
        wb[kChunk + tid] = val_live ? fmaf(wt.t1, val, wt.t0) : 0.0f;
      }
    }
  };

  const int cs_col = tid % G::K, cs_group = tid / G::K;
  if (chunks > 0) {
    load(0);
    store(0);
  }
  __syncthreads();
  for (int64_t c = 0; c < chunks; ++c) {
    const int buf = (int)(c & 1);
    const bool more = c + 1 < chunks;
    if (more) load(c + 1);
    const float* xb = stage + buf * kChunk * G::XS;
    if constexpr (Wt::kOn) {
      const float* wb = wt.lds + buf * 2 * kChunk;
      const f32x4 w03 = *reinterpret_cast<const f32x4*>(wb + q * (kChunk / 4));       // entries q, 4 + q, 8 + q, 12 + q
      const f32x4 w47 = *reinterpret_cast<const f32x4*>(wb + q * (kChunk / 4) + 4);   // ... 16 + q .. 28 + q
      const float w[kChunk / 4] = {w03[0], w03[1], w03[2], w03[3], w47[0], w47[1], w47[2], w47[3]};
#pragma unroll
      for (int i = 0; i < G::TPW; ++i) {
        if (tiles.live(i, wave)) {
          const float* pa = xb + q * G::XS + 16 * tiles.ta[i] + r;
          const float* pb = xb + q * G::XS + 16 * tiles.tb[i] + r;
#pragma unroll
          for (int s = 0; s < kChunk / 4; ++s) acc[i] = mfma4(w[s] * pa[4 * s * G::XS], pb[4 * s * G::XS], acc[i]);
        }
      }
      if (cs_group < G::kGroups) {
        const float* pc = xb + cs_group * G::kPerGroup * G::XS + cs_col;
        const float* pt = wb + kChunk + cs_group * G::kPerGroup;
#pragma unroll
        for (int e = 0; e < G::kPerGroup; ++e) cs = fmaf(pt[e], pc[e * G::XS], cs);
      }
    } else {
#pragma unroll
      for (int i = 0; i < G::TPW; ++i) {
        if (tiles.live(i, wave)) {
          const float* pa = xb + q * G::XS + 16 * tiles.ta[i] + r;
          const float* pb = xb + q * G::XS + 16 * tiles.tb[i] + r;
#pragma unroll
          for (int s = 0; s < kChunk / 4; ++s) acc[i] = mfma4(pa[4 * s * G::XS], pb[4 * s * G::XS], acc[i]);
        }
      }
      if (cs_group < G::kGroups) {
        const float* pc = xb + cs_group * G::kPerGroup * G::XS + cs_col;
#pragma unroll
        for (int e = 0; e < G::kPerGroup; ++e) cs += pc[e * G::XS];
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Gram
// ---------------------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kThreads) void als_gram_slab_kernel(const float* __restrict__ Y, int64_t rows,
                                                                 float* __restrict__ ws) {
  using G = Geo<KB>;
  __shared__ __attribute__((aligned(16))) float stage[G::kStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kSlab;
  const int64_t n = rows - row0 < kSlab ? rows - row0 : kSlab;
  const Tiles<KB> tiles(wave);
  f32x4 acc[G::TPW];
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs = 0.0f;
  als_accumulate<KB>(n, [&](int64_t e) { return Y + (row0 + e) * G::K; }, NoWeights{}, stage, tiles, acc, cs);
  float* part = ws + (int64_t)blockIdx.x * G::K * G::K;
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) {
    if (tiles.live(i, wave)) {
#pragma unroll
      for (int c = 0; c < 4; ++c) part[(16 * tiles.ta[i] + 4 * q + c) * G::K + 16 * tiles.tb[i] + r] = acc[i][c];
    }
  }
}

// G[i][j] = G[j][i] = the partials' entry (max, min), added in ascending slab order
__global__ __launch_bounds__(kThreads) void als_gram_merge_kernel(const float* __restrict__ ws, int64_t slabs, int k,
                                                                  float* __restrict__ gram) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= k * k) return;
  const int i = e / k, j = e % k;
  const int src = i >= j ? e : j * k + i;
  float a = 0.0f;
  for (int64_t s = 0; s < slabs; ++s) a += ws[s * k * k + src];
  gram[e] = a;
}

// ---------------------------------------------------------------------------------------------------------------
// row solves
// ---------------------------------------------------------------------------------------------------------------
// the scalars of one launch.  Unit: A = gram + alpha S + reg I, b = (1 + alpha) s.  Weighted: the weights are already
// in S and s, A = (gram or 0) + S + (reg + reg_per_entry n) I, b = s.
struct UnitSystem {
  static constexpr bool kWeighted = false;
  float reg, alpha;
};
struct WeightedSystem {
  static constexpr bool kWeighted = true;
  const float* values;   // aligned with indices
  float w0, w1, t0, t1, reg, reg_per_entry;
};

// one kernel text, two families of instantiations that differ in `sys` alone
template <int KB, typename Sys>
__global__ __launch_bounds__(kThreads) void als_solve_rows_kernel(
    const float* __restrict__ Y, int64_t y_rows, const float* __restrict__ gram, const int64_t* __restrict__ indptr,
    const int32_t* __restrict__ indices, int64_t csr_rows, const int64_t* __restrict__ rows, const Sys sys,
    float* __restrict__ out, int64_t ldo, int32_t* __restrict__ err_flag) {
  using G = Geo<KB>;
  constexpr int K = G::K, LDA = G::LDA;
  __shared__ __attribute__((aligned(16))) float smem[G::kMain];
  __shared__ float s_cs[G::kGroups * K];
  __shared__ int s_err;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  float* dst = out + (int64_t)blockIdx.x * ldo;

  const int64_t row = rows ? rows[blockIdx.x] : (int64_t)blockIdx.x;
  const bool row_ok = row >= 0 && row < csr_rows;
  int64_t p0 = 0, p1 = 0;
  if (row_ok) {
    p0 = indptr[row];
    p1 = indptr[row + 1];
  }
  const int64_t n = p1 > p0 ? p1 - p0 : 0;
  if (n == 0) {   // an empty list: b = 0, so x = 0 exactly (uniform over the workgroup)
    if (tid < K) dst[tid] = 0.0f;
    // a row id outside the CSR, or offsets that run backwards: nothing was dereferenced
    if ((!row_ok || p1 < p0) && tid == 0 && err_flag) atomicOr(err_flag, kErrIndex);
    return;
  }
  if (tid == 0) s_err = 0;

  // (a)
  const Tiles<KB> tiles(wave);
  f32x4 acc[G::TPW];
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs = 0.0f;
  bool bad_index = false;
  als_accumulate<KB>(
      n,
      [&](int64_t e) -> const float* {
        const int64_t id = indices[p0 + e];
        if (id < 0 || id >= y_rows) {
          bad_index = true;
          return nullptr;
        }
        return Y + id * K;
      },
      [&] {
        if constexpr (Sys::kWeighted) {
          __shared__ __attribute__((aligned(16))) float s_wt[2 * 2 * kChunk];
          return Weights{sys.values + p0, sys.w0, sys.w1, sys.t0, sys.t1, s_wt};
        } else {
          return NoWeights{};
        }
      }(),
      smem, tiles, acc, cs);
  if (bad_index) s_err = kErrIndex;   // every writer stores the same value

  // (b) the stage buffers are dead: A takes their place
  float* A = smem;
  [[maybe_unused]] float diag = 0.0f;
  if constexpr (Sys::kWeighted) diag = fmaf(sys.reg_per_entry, (float)n, sys.reg);
#pragma unroll
  for (int i = 0; i < G::TPW; ++i) {
    if (tiles.live(i, wave)) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ai = 16 * tiles.ta[i] + 4 * q + c, aj = 16 * tiles.tb[i] + r;
        float v;
        if constexpr (Sys::kWeighted) {
          v = acc[i][c];
          if (gram) v += gram[ai * K + aj];
          if (ai == aj) v += diag;
        } else {
          v = fmaf(sys.alpha, acc[i][c], gram[ai * K + aj]);
          if (ai == aj) v += sys.reg;
        }
        A[ai * LDA + aj] = v;
      }
    }
  }
  if (tid < G::kGroups * K) s_cs[tid] = cs;
  __syncthreads();
  if (tid < K) {
    float s = 0.0f;
#pragma unroll
    for (int g = 0; g < G::kGroups; ++g) s += s_cs[g * K + tid];
    if constexpr (!Sys::kWeighted) s = (1.0f + sys.alpha) * s;
    A[K * LDA + tid] = s;
  }

  // (c) A = L L^T by blocks of 16; row K becomes y
  for (int j = 0; j < KB; ++j) {
    const int c0 = 16 * j;
    __syncthreads();
    if (wave == 0) {   // the diagonal block: lane l (and its three copies) holds row l
      float a[16];
      const float* src = A + (c0 + r) * LDA + c0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src + 4 * v);
        a[4 * v] = t[0]; a[4 * v + 1] = t[1]; a[4 * v + 2] = t[2]; a[4 * v + 3] = t[3];
      }
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        float piv = __shfl(a[c], c, 16);
        if (!(piv > 0.0f) || piv == INFINITY) {
          bad = true;
          piv = 1.0f;
        }
        const float d = sqrtf(piv);
        a[c] = r == c ? d : a[c] / d;
#pragma unroll
        for (int c2 = c + 1; c2 < 16; ++c2) a[c2] -= a[c] * __shfl(a[c], c2, 16);
      }
      if (lane < 16) {
        float* d4 = A + (c0 + r) * LDA + c0;
#pragma unroll
        for (int v = 0; v < 4; ++v)
          *reinterpret_cast<f32x4*>(d4 + 4 * v) = f32x4{a[4 * v], a[4 * v + 1], a[4 * v + 2], a[4 * v + 3]};
      }
      if (bad && lane == 0) s_err |= kErrPivot;
    }
    __syncthreads();
    // the panel: rows c0 + 16 .. K (row K is b), one per thread: x L11^T = a
    const int prow = c0 + 16 + tid;
    if (prow <= K) {
      float x[16];
      float* src = A + prow * LDA + c0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(src + 4 * v);
        x[4 * v] = t[0]; x[4 * v + 1] = t[1]; x[4 * v + 2] = t[2]; x[4 * v + 3] = t[3];
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float* lrow = A + (c0 + c) * LDA + c0;
        float v = x[c];
#pragma unroll
        for (int d = 0; d < c; ++d) v -= x[d] * lrow[d];
        x[c] = v / lrow[c];
      }
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<f32x4*>(src + 4 * v) = f32x4{x[4 * v], x[4 * v + 1], x[4 * v + 2], x[4 * v + 3]};
    }
    __syncthreads();
    // the trailing update: tiles on and below the diagonal of A22 dealt over the waves, and row K by threads
    int cnt = 0;
    for (int ta = j + 1; ta < KB; ++ta)
      for (int tb = j + 1; tb <= ta; ++tb) {
        if ((cnt++ & (kWaves - 1)) != wave) continue;
        float* pc = A + (16 * ta + 4 * q) * LDA + 16 * tb + r;
        f32x4 t = f32x4{pc[0], pc[LDA], pc[2 * LDA], pc[3 * LDA]};
        const float* pa = A + (16 * ta + r) * LDA + c0 + q;
        const float* pb = A + (16 * tb + r) * LDA + c0 + q;
#pragma unroll
        for (int s = 0; s < 4; ++s) t = mfma4(-pa[4 * s], pb[4 * s], t);
        pc[0] = t[0]; pc[LDA] = t[1]; pc[2 * LDA] = t[2]; pc[3 * LDA] = t[3];
      }
    const int bc = c0 + 16 + tid;
    if (bc < K) {
      const float* yb = A + K * LDA + c0;
      const float* lr = A + bc * LDA + c0;
      float v = A[K * LDA + bc];
#pragma unroll
      for (int d = 0; d < 16; ++d) v -= yb[d] * lr[d];
      A[K * LDA + bc] = v;
    }
  }
  __syncthreads();

  // L^T x = y in one wave: lane l holds elements l and l + 64
  if (wave == 0) {
    float x0 = lane < K ? A[K * LDA + lane] : 0.0f;
    float x1 = lane + 64 < K ? A[K * LDA + lane + 64] : 0.0f;
    for (int c = K - 1; c >= 0; --c) {
      const float* lrow = A + c * LDA;
      const float yc = __shfl(c >= 64 ? x1 : x0, c & 63, 64);
      const float xc = yc / lrow[c];
      if (lane == (c & 63)) {
        if (c >= 64) x1 = xc; else x0 = xc;
      }
      if (lane < c) x0 -= lrow[lane] * xc;
      if (lane + 64 < c) x1 -= lrow[lane + 64] * xc;
    }
    const bool finite = fabsf(x0) < INFINITY && fabsf(x1) < INFINITY;   // false for a NaN too
    int err = s_err;
    if (!__all(finite)) err |= kErrPivot;
    if (err) {
      x0 = 0.0f;
      x1 = 0.0f;
      if (lane == 0 && err_flag) atomicOr(err_flag, err);
    }
    if (lane < K) dst[lane] = x0;
    if (lane + 64 < K) dst[lane + 64] = x1;
  }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

bool dim_ok(int k) { return k >= 16 && k <= CTR_ALS_MAX_DIM && k % 16 == 0; }

static_assert(CTR_ALS_MAX_DIM == 16 * 8, "one template instance per k block of 16; x of the back substitution in two registers");

#define ALS_CASES(LAUNCH) \
  switch (k / 16) {       \
    case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; case 4: LAUNCH(4); break; \
    case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; case 7: LAUNCH(7); break; case 8: LAUNCH(8); break; \
    default: return CTR_ELIMIT;                                                                              \
  }

}  // namespace

extern "C" int ctr_als_gram_workspace_bytes(int64_t rows, int k, int64_t* bytes) {
  CTR_REQUIRE(bytes && rows >= 1 && k >= 1, CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && rows < (1ll << 31), CTR_ELIMIT);
  *bytes = ctr_ceil_div(rows, kSlab) * k * k * (int64_t)sizeof(float);
  return CTR_OK;
}

extern "C" int ctr_als_gram(const float* y, int64_t rows, int k, float* gram, void* workspace, int64_t workspace_bytes,
                            void* stream) {
  CTR_REQUIRE(y && gram && workspace && rows >= 1 && k >= 1, CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && rows < (1ll << 31), CTR_ELIMIT);
  const int64_t slabs = ctr_ceil_div(rows, kSlab);
  CTR_REQUIRE(workspace_bytes >= slabs * k * k * (int64_t)sizeof(float), CTR_EINVAL);
  CTR_REQUIRE(aligned_to(y, 16) && aligned_to(gram, 4) && aligned_to(workspace, 4), CTR_EALIGN);
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
#define ALS_GRAM(KB) \
  hipLaunchKernelGGL((als_gram_slab_kernel<KB>), dim3((unsigned)slabs), dim3(kThreads), 0, s, y, rows, ws)
  ALS_CASES(ALS_GRAM)
#undef ALS_GRAM
  const int rc = ctr_launch_status();
  if (rc != CTR_OK) return rc;
  hipLaunchKernelGGL(als_gram_merge_kernel, dim3((unsigned)ctr_ceil_div(k * k, kThreads)), dim3(kThreads), 0, s, ws,
                     slabs, k, gram);
  return ctr_launch_status();
}

extern "C" int ctr_als_solve_rows(const float* y, int64_t y_rows, int k, const float* gram, const int64_t* indptr,
                                  const int32_t* indices, int64_t csr_rows, const int64_t* rows, int64_t count,
                                  float reg, float alpha, float* out, int64_t ldo, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(count >= 0 && y_rows >= 1 && csr_rows >= 1 && k >= 1, CTR_EINVAL);
  if (count == 0) return CTR_OK;
  // indices may be NULL: a CSR without a single pair
  CTR_REQUIRE(y && gram && indptr && out && ldo >= k && reg == reg && alpha == alpha, CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && count < (1ll << 31) && y_rows < (1ll << 31), CTR_ELIMIT);
  CTR_REQUIRE(aligned_to(y, 16) && aligned_to(gram, 4) && aligned_to(indptr, 8) && aligned_to(indices, 4) &&
                  aligned_to(rows, 8) && aligned_to(out, 4) && aligned_to(err_flag, 4),
              CTR_EALIGN);
  hipStream_t s = (hipStream_t)stream;
  const UnitSystem sys{reg, alpha};
#define ALS_SOLVE(KB)                                                                                             \
  hipLaunchKernelGGL((als_solve_rows_kernel<KB, UnitSystem>), dim3((unsigned)count), dim3(kThreads), 0, s, y,     \
                     y_rows, gram, indptr, indices, csr_rows, rows, sys, out, ldo, err_flag)
  ALS_CASES(ALS_SOLVE)
#undef ALS_SOLVE
  return ctr_launch_status();
}

extern "C" int ctr_als_solve_rows_weighted(const float* y, int64_t y_rows, int k, const float* gram,
                                           const int64_t* indptr, const int32_t* indices, const float* values,
                                           int64_t csr_rows, const int64_t* rows, int64_t count, float w0, float w1,
                                           float t0, float t1, float reg, float reg_per_entry, float* out, int64_t ldo,
                                           int32_t* err_flag, void* stream) {
  CTR_REQUIRE(count >= 0 && y_rows >= 1 && csr_rows >= 1 && k >= 1, CTR_EINVAL);
  if (count == 0) return CTR_OK;
  // indices may be NULL: a CSR without a single pair, the only one that may come without values; gram may be NULL
  CTR_REQUIRE(y && indptr && out && ldo >= k && (values || !indices), CTR_EINVAL);
  CTR_REQUIRE(w0 == w0 && w1 == w1 && t0 == t0 && t1 == t1 && reg == reg && reg_per_entry == reg_per_entry,
              CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && count < (1ll << 31) && y_rows < (1ll << 31), CTR_ELIMIT);
  CTR_REQUIRE(aligned_to(y, 16) && aligned_to(gram, 4) && aligned_to(indptr, 8) && aligned_to(indices, 4) &&
                  aligned_to(values, 4) && aligned_to(rows, 8) && aligned_to(out, 4) && aligned_to(err_flag, 4),
              CTR_EALIGN);
  hipStream_t s = (hipStream_t)stream;
  const WeightedSystem sys{values, w0, w1, t0, t1, reg, reg_per_entry};
#define ALS_SOLVE_W(KB)                                                                                           \
  hipLaunchKernelGGL((als_solve_rows_kernel<KB, WeightedSystem>), dim3((unsigned)count), dim3(kThreads), 0, s, y, \
                     y_rows, gram, indptr, indices, csr_rows, rows, sys, out, ldo, err_flag)
  ALS_CASES(ALS_SOLVE_W)
#undef ALS_SOLVE_W
  return ctr_launch_status();
}
