// Full softmax over the catalogue: the cross entropy of a target item against EVERY item, its loss and both gradients
//     z[b, i] = <X[b], Q[i]>,   lse[b] = log sum_i exp(z[b, i]),   nll[b] = lse[b] - z[b, t_b],
//     G[b, i] = g_b (exp(z[b, i] - lse[b]) - [i == t_b]),   dX = G Q,   dQ = G^T X
// on the fp32 matrix cores.  The B x I logits and G only ever exist as register tiles.
//
// The frame is gdcf.hip's: a workgroup OWNS 64 rows of one matrix (4 waves x 16), walks 16-row tiles of the STREAMED
// matrix staged through LDS (double buffered), forms the 16 streamed x 16 owners score tile with
// v_mfma_f32_16x16x4_f32 (one accumulator chain per pair) and feeds a tile in the accumulator layout back as the B
// operand of the gradient product (see gdcf.hip for the operand layouts).
//   row pass   : owner = batch row, streamed = items.  ONE sweep with a running maximum m, a denominator l and a
//                rescaled accumulator acc = sum_i exp(z_i - m) Q[i] (an attention forward with K = V = Q):
//                lse = m + log l, nll = lse - z_t, dX_unit = acc / l - Q[t] (the gradient for g = 1).
//                An owner's sixteen streamed scores sit in lanes l, l+16, l+32, l+48 x four registers, so the tile
//                maximum and sum are two cross-lane steps; every accumulator register of a lane belongs to that lane's
//                owner, so a rescale is one multiply per register.
//   column pass: owner = item, streamed = batch rows with their lse, g and t staged beside the tile.  G is formed as
//                above, the indicator by comparison: no scatter for the target term, no atomics.  -> dQ
//                The target's entry g (p_t - 1) cancels when p_t approaches 1, and a float32 lse cannot hold
//                log l below half an ulp of m; the row pass therefore forms nll = (m - z_t) + log l, which keeps it,
//                and the column pass takes the entry as g expm1(-nll) when it is handed nll.
// Padding items count as -inf, padding batch rows as g = 0, padding owners write nothing.  exp never sees a positive
// argument.  A target outside [0, I) is never dereferenced: no indicator, nll = lse, *err_flag = 1.
//
// When the owners alone do not fill the device, the streamed range is split over gridDim.y parts; a part leaves
// (m, l, z_t, acc) per row, resp. its partial dQ, in the workspace and a short second launch merges the parts in
// ascending order.  The part count depends on (B, I, k), the CU count and the caller's override only, and nothing is
// accumulated with atomics, so every output is bitwise reproducible.
#include <math.h>

#include "ctr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kOwn = 16;                 // owner rows per wave
constexpr int kBO = kWaves * kOwn;       // owner rows per workgroup
constexpr int kTS = 16;                  // streamed rows per tile
constexpr int kTRow = kTS + 4;           // transposed tile row in LDS (floats; 16-byte aligned, staggers banks)
constexpr int kMaxSplits = 64;           // the largest override
constexpr int kAutoParts = 16;           // the most parts the automatic choice takes (bounds the workspace)
constexpr int kMinTiles = 8;             // ... and the fewest tiles it leaves a part
constexpr int kStat = 4;                 // floats of a row's (m, l, z_t, -) in the workspace

enum { kRowsLoss = 0, kRowsGrad = 1, kCols = 2 };

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// KB = k blocks of 16.  X (no, k) the owners, Z (ns, k) the streamed rows.  target / lse_in / gout belong to the batch
// rows: the owners of the row modes, the streamed rows of kCols.  gridDim.y parts of tiles_per_part tiles each, none
// empty; one part writes the outputs, several write the workspace.
template <int KB, int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void softmax_full_pass_kernel(
    const float* __restrict__ X, int64_t no, const float* __restrict__ Z, int64_t ns, int k,
    const int64_t* __restrict__ target, int64_t num_items, const float* __restrict__ lse_in,
    const float* __restrict__ nll_in, const float* __restrict__ gout, int64_t tiles_per_part, float* __restrict__ nll, float* __restrict__ lse,
    float* __restrict__ grad, float* __restrict__ ws, int32_t* __restrict__ err_flag) {
  constexpr bool ROWS = MODE != kCols, GRAD = MODE != kRowsLoss;
  constexpr int KP = 16 * KB;            // padded k
  constexpr int KRow = KP + 4;           // natural tile row in LDS (floats)
  constexpr int kStage = kTS * KP / kThreads;   // tile elements staged per thread (= KB)
  __shared__ float s_zn[2][kTS * KRow];
  __shared__ float s_zt[GRAD ? 2 : 1][GRAD ? KP * kTRow : 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_side[ROWS ? 1 : 2][ROWS ? 1 : 4 * kTS];   // lse, g, t, g (p_t - 1)

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t o = (int64_t)blockIdx.x * kBO + wave * kOwn + r;   // this lane's owner row (B column / D column)
  const bool own_ok = o < no;
  const int parts = gridDim.y, part = blockIdx.y;

  // X operand: step s = 4 j + c is dimension 16 j + 4 q + c
  float xb[4 * KB];
#pragma unroll
  for (int j = 0; j < KB; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d = 16 * j + 4 * q + c;
      xb[4 * j + c] = (own_ok && d < k) ? X[o * k + d] : 0.0f;
    }

  f32x4 acc[GRAD ? KB : 1];
#pragma unroll
  for (int b = 0; b < (GRAD ? KB : 1); ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // row modes: the owner's target and its running softmax
  int64_t tb = -1;
  float m = -INFINITY, l = 0.0f, zt = 0.0f;
  if constexpr (ROWS) {
    if (own_ok) {
      tb = target[o];
      if (tb < 0 || tb >= num_items) {
        tb = -1;
        if (err_flag && part == 0 && q == 0) *err_flag = 1;
      }
    }
  }

  const int64_t T = (ns + kTS - 1) / kTS;
  const int64_t t0 = part * tiles_per_part, t1 = (t0 + tiles_per_part < T) ? t0 + tiles_per_part : T;
  // staging: a thread takes columns scol + 16 i of tile row srow_, so every address is one base plus a constant
  const int srow_ = threadIdx.x >> 4, scol = threadIdx.x & 15;
  float stage[kStage];
  auto load_tile = [&](int64_t t) {
    const int64_t zr = t * kTS + srow_;
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int col = scol + 16 * i;
      stage[i] = (zr < ns && col < k) ? Z[zr * k + col] : 0.0f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int col = scol + 16 * i;
      s_zn[buf][srow_ * KRow + col] = stage[i];
      if constexpr (GRAD) s_zt[buf][col * kTRow + srow_] = stage[i];
    }
  };
  // kCols: threads 0..63 stage the tile's sixteen lse, g, t and target entries g expm1(-nll) (a padding row: g = 0,
  // no target)
  uint32_t side = 0u;
  auto load_side = [&](int64_t t) {
    if constexpr (!ROWS) {
      if (threadIdx.x < 4 * kTS) {
        const int which = threadIdx.x >> 4;
        const int64_t row = t * kTS + (threadIdx.x & 15);
        const bool ok = row < ns;
        if (which == 0) {
          side = ok ? __float_as_uint(lse_in[row]) : 0u;
        } else if (which == 1) {
          side = ok ? __float_as_uint(gout[row]) : 0u;
        } else if (which == 2) {
          const int64_t tv = ok ? target[row] : -1;
          side = (tv >= 0 && tv < num_items) ? (uint32_t)tv : 0xffffffffu;
        } else {
          side = (ok && nll_in) ? __float_as_uint(gout[row] * expm1f(-fmaxf(nll_in[row], 0.0f))) : 0u;
        }
      }
    }
  };
  auto store_side = [&](int buf) {
    if constexpr (!ROWS) {
      if (threadIdx.x < 4 * kTS) s_side[buf][threadIdx.x] = side;
    }
  };

  load_tile(t0);
  load_side(t0);
  store_tile(0);
  store_side(0);
  __syncthreads();

  for (int64_t t = t0; t < t1; ++t) {
    const int buf = (int)((t - t0) & 1);
    const bool more = t + 1 < t1;
    if (more) {
      load_tile(t + 1);
      load_side(t + 1);
    }

    // scores: one accumulator chain over the k steps
    const float* zn = &s_zn[buf][r * KRow + 4 * q];
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(zn + 16 * j);
#pragma unroll
      for (int c = 0; c < 4; ++c) s = mfma4(a[c], xb[4 * j + c], s);
    }

    float g[4];
    const int64_t srow = t * kTS + 4 * q;   // streamed row of register 0
    if constexpr (ROWS) {
      float sv[4], tmax = -INFINITY;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sv[c] = srow + c < ns ? s[c] : -INFINITY;
        tmax = fmaxf(tmax, sv[c]);
        if (srow + c == tb) zt = s[c];
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float mn = fmaxf(m, tmax);        // finite: a tile has at least one item
      const float sc = expf(m - mn);          // 0 at the first tile (m = -inf), never of a positive argument
      float ps = 0.0f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        g[c] = expf(sv[c] - mn);              // a padding item: exp(-inf) = 0
        ps += g[c];
      }
      ps += __shfl_xor(ps, 16, 64);
      ps += __shfl_xor(ps, 32, 64);
      l = l * sc + ps;
      m = mn;
      if constexpr (GRAD) {
#pragma unroll
        for (int b = 0; b < KB; ++b) acc[b] *= sc;
      }
    } else {
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(&s_side[buf][4 * q]);
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(&s_side[buf][kTS + 4 * q]);
      const f32x4 gt4 = *reinterpret_cast<const f32x4*>(&s_side[buf][3 * kTS + 4 * q]);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float e = expf(fminf(s[c] - l4[c], 0.0f));   // lse >= z up to rounding: never a positive argument
        const bool hit = s_side[buf][2 * kTS + 4 * q + c] == (uint32_t)o;
        const float v = hit ? (nll_in ? gt4[c] : g4[c] * (e - 1.0f)) : g4[c] * e;
        g[c] = (own_ok && srow + c < ns) ? v : 0.0f;
      }
    }

    if constexpr (GRAD) {
      const float* zt_ = &s_zt[buf][r * kTRow + 4 * q];
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(zt_ + 16 * b * kTRow);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[b] = mfma4(a[c], g[c], acc[b]);
      }
    }

    if (more) {
      store_tile(buf ^ 1);
      store_side(buf ^ 1);
    }
    __syncthreads();
  }

  if constexpr (ROWS) {
    // the target's score sits in one of the owner's four lanes
    zt += __shfl_xor(zt, 16, 64);
    zt += __shfl_xor(zt, 32, 64);
  }
  if (!own_ok) return;

  if constexpr (ROWS) {
    if (parts == 1) {
      if (q == 0) {
        const float ll = logf(l);
        lse[o] = m + ll;
        nll[o] = tb >= 0 ? (m - zt) + ll : m + ll;   // m - z_t first: log l survives a large m
      }
      if constexpr (GRAD) {
#pragma unroll
        for (int b = 0; b < KB; ++b)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int d = 16 * b + 4 * q + c;
            if (d < k) grad[o * k + d] = acc[b][c] / l - (tb >= 0 ? Z[tb * k + d] : 0.0f);
          }
      }
    } else {
      const int64_t slot = (int64_t)part * no + o;
      if (q == 0) {
        float* st = ws + slot * kStat;
        st[0] = m;
        st[1] = l;
        st[2] = zt;
      }
      if constexpr (GRAD) {
        float* pa = ws + (int64_t)parts * no * kStat + slot * k;
#pragma unroll
        for (int b = 0; b < KB; ++b)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int d = 16 * b + 4 * q + c;
            if (d < k) pa[d] = acc[b][c];
          }
      }
    }
  } else {
    float* dst = parts == 1 ? grad + o * k : ws + ((int64_t)part * no + o) * k;
#pragma unroll
    for (int b = 0; b < KB; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int d = 16 * b + 4 * q + c;
        if (d < k) dst[d] = acc[b][c];
      }
  }
}

// the row pass's parts of one batch row, merged by one wave in ascending part order
__global__ __launch_bounds__(kThreads) void softmax_full_rows_merge_kernel(
    const float* __restrict__ ws, int parts, int64_t batch, int k, const int64_t* __restrict__ target,
    int64_t num_items, const float* __restrict__ Q, float* __restrict__ nll, float* __restrict__ lse,
    float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= batch) return;
  float M = -INFINITY;
  for (int p = 0; p < parts; ++p) M = fmaxf(M, ws[((int64_t)p * batch + b) * kStat]);
  float L = 0.0f, zt = 0.0f;
  for (int p = 0; p < parts; ++p) {
    const float* st = ws + ((int64_t)p * batch + b) * kStat;
    L += st[1] * expf(st[0] - M);
    zt += st[2];
  }
  int64_t tb = target[b];
  if (tb < 0 || tb >= num_items) tb = -1;
  if (lane == 0) {
    const float ll = logf(L);
    lse[b] = M + ll;
    nll[b] = tb >= 0 ? (M - zt) + ll : M + ll;
  }
  if (grad) {
    const float* pa = ws + (int64_t)parts * batch * kStat;
    for (int d = lane; d < k; d += 64) {
      float a = 0.0f;
      for (int p = 0; p < parts; ++p) {
        const int64_t slot = (int64_t)p * batch + b;
        a += pa[slot * k + d] * expf(ws[slot * kStat] - M);
      }
      grad[b * k + d] = a / L - (tb >= 0 ? Q[tb * k + d] : 0.0f);
    }
  }
}

// dQ = the column pass's partial dQ summed in ascending part order
__global__ __launch_bounds__(kThreads) void softmax_full_cols_merge_kernel(const float* __restrict__ ws, int parts,
                                                                           int64_t n, float* __restrict__ grad) {
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < n; e += (int64_t)gridDim.x * kThreads) {
    float a = 0.0f;
    for (int p = 0; p < parts; ++p) a += ws[(int64_t)p * n + e];
    grad[e] = a;
  }
}

struct Split {
  int parts;
  int64_t tiles_per_part;
};

// how the streamed range is cut: `splits` parts when the caller says so, else enough to fill the device twice over
// with workgroups, at most kAutoParts and none shorter than kMinTiles tiles; never an empty part
Split split_of(int64_t owners, int64_t streamed, int splits) {
  const int64_t T = ctr_ceil_div(streamed, kTS);
  int64_t want = splits;
  if (splits <= 0) {
    want = 2 * kCtrCUs / ctr_ceil_div(owners, kBO);
    if (want > T / kMinTiles) want = T / kMinTiles;
    if (want > kAutoParts) want = kAutoParts;
  }
  if (want > T) want = T;
  if (want < 1) want = 1;
  Split s;
  s.tiles_per_part = ctr_ceil_div(T, want);
  s.parts = (int)ctr_ceil_div(T, s.tiles_per_part);
  return s;
}

int64_t rows_bytes(int64_t batch, int k, int parts) {
  return parts > 1 ? (int64_t)parts * batch * (kStat + k) * (int64_t)sizeof(float) : 0;
}
int64_t cols_bytes(int64_t num_items, int k, int parts) {
  return parts > 1 ? (int64_t)parts * num_items * k * (int64_t)sizeof(float) : 0;
}

template <int MODE>
int launch_pass(const float* X, int64_t no, const float* Z, int64_t ns, int k, const int64_t* target,
                int64_t num_items, const float* lse_in, const float* nll_in, const float* gout, const Split& sp, float* nll, float* lse,
                float* grad, float* ws, int32_t* err_flag, hipStream_t stream) {
  const dim3 grid((unsigned)ctr_ceil_div(no, kBO), (unsigned)sp.parts), block(kThreads);
#define SFM_CASE(KB)                                                                                              \
  case KB:                                                                                                      \
    hipLaunchKernelGGL((softmax_full_pass_kernel<KB, MODE>), grid, block, 0, stream, X, no, Z, ns, k, target,  \
                       num_items, lse_in, nll_in, gout, sp.tiles_per_part, nll, lse, grad, ws, err_flag);              \
    break;
  switch ((k + 15) / 16) {
    SFM_CASE(1) SFM_CASE(2) SFM_CASE(3) SFM_CASE(4) SFM_CASE(5) SFM_CASE(6) SFM_CASE(7) SFM_CASE(8)
    SFM_CASE(9) SFM_CASE(10) SFM_CASE(11) SFM_CASE(12) SFM_CASE(13) SFM_CASE(14) SFM_CASE(15) SFM_CASE(16)
    default: return CTR_ELIMIT;
  }
#undef SFM_CASE
  return ctr_launch_status();
}

static_assert(CTR_SOFTMAX_FULL_MAX_DIM == 16 * 16, "one template instance per k block of 16");

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks both passes share, in the family's order; *empty: nothing to do
int softmax_full_check(int64_t batch, int64_t num_items, int k, int splits, bool pointers, bool* empty) {
  CTR_REQUIRE(batch >= 0 && num_items >= 1 && k >= 1 && splits >= 0, CTR_EINVAL);
  *empty = batch == 0;
  if (*empty) return CTR_OK;
  CTR_REQUIRE(pointers, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_SOFTMAX_FULL_MAX_DIM && batch < (1ll << 31) && num_items < (1ll << 31) && splits <= kMaxSplits,
              CTR_ELIMIT);
  return CTR_OK;
}

}  // namespace

extern "C" int ctr_softmax_full_workspace_bytes(int64_t batch, int64_t num_items, int k, int splits_rows,
                                                int splits_cols, int64_t* bytes) {
  CTR_REQUIRE(bytes && batch >= 0 && num_items >= 1 && k >= 1 && splits_rows >= 0 && splits_cols >= 0, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_SOFTMAX_FULL_MAX_DIM && batch < (1ll << 31) && num_items < (1ll << 31) &&
                  splits_rows <= kMaxSplits && splits_cols <= kMaxSplits,
              CTR_ELIMIT);
  *bytes = 0;
  if (batch == 0) return CTR_OK;
  const int64_t rows = rows_bytes(batch, k, split_of(batch, num_items, splits_rows).parts);
  const int64_t cols = cols_bytes(num_items, k, split_of(num_items, batch, splits_cols).parts);
  *bytes = rows > cols ? rows : cols;
  return CTR_OK;
}

extern "C" int ctr_softmax_full_rows(const float* x, const float* q, int64_t batch, int64_t num_items, int k,
                                     const int64_t* target, float* nll, float* lse, float* grad_x, int splits,
                                     void* workspace, int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  bool empty = false;
  const int rc = softmax_full_check(batch, num_items, k, splits, x && q && target && nll && lse, &empty);
  if (rc != CTR_OK || empty) return rc;
  const Split sp = split_of(batch, num_items, splits);
  CTR_REQUIRE(sp.parts == 1 || (workspace && workspace_bytes >= rows_bytes(batch, k, sp.parts)), CTR_EINVAL);
  CTR_REQUIRE(aligned_to(x, 4) && aligned_to(q, 4) && aligned_to(nll, 4) && aligned_to(lse, 4) &&
                  aligned_to(grad_x, 4) && aligned_to(target, 8) && aligned_to(err_flag, 4) &&
                  aligned_to(workspace, 4),
              CTR_EALIGN);
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const int r = grad_x ? launch_pass<kRowsGrad>(x, batch, q, num_items, k, target, num_items, nullptr, nullptr, nullptr, sp,
                                                nll, lse, grad_x, ws, err_flag, s)
                       : launch_pass<kRowsLoss>(x, batch, q, num_items, k, target, num_items, nullptr, nullptr, nullptr, sp,
                                                nll, lse, nullptr, ws, err_flag, s);
  if (r != CTR_OK || sp.parts == 1) return r;
  hipLaunchKernelGGL(softmax_full_rows_merge_kernel, dim3((unsigned)ctr_ceil_div(batch, kWaves)), dim3(kThreads), 0,
                     s, ws, sp.parts, batch, k, target, num_items, q, nll, lse, grad_x);
  return ctr_launch_status();
}

extern "C" int ctr_softmax_full_cols(const float* x, const float* q, int64_t batch, int64_t num_items, int k,
                                     const int64_t* target, const float* lse, const float* nll, const float* gout,
                                     float* grad_q, int splits, void* workspace, int64_t workspace_bytes, void* stream) {
  bool empty = false;
  const int rc = softmax_full_check(batch, num_items, k, splits, x && q && target && lse && gout && grad_q, &empty);
  if (rc != CTR_OK || empty) return rc;   // an empty batch: grad_q is not written (the caller's zeros stand)
  hipStream_t s = (hipStream_t)stream;
  const Split sp = split_of(num_items, batch, splits);
  CTR_REQUIRE(sp.parts == 1 || (workspace && workspace_bytes >= cols_bytes(num_items, k, sp.parts)), CTR_EINVAL);
  CTR_REQUIRE(aligned_to(x, 4) && aligned_to(q, 4) && aligned_to(lse, 4) && aligned_to(nll, 4) &&
                  aligned_to(gout, 4) && aligned_to(grad_q, 4) && aligned_to(target, 8) && aligned_to(workspace, 4),
              CTR_EALIGN);
  float* ws = static_cast<float*>(workspace);
  const int r = launch_pass<kCols>(q, num_items, x, batch, k, target, num_items, lse, nll, gout, sp, nullptr, nullptr,
                                   grad_q, ws, nullptr, s);
  if (r != CTR_OK || sp.parts == 1) return r;
  const int64_t n = num_items * k;
  hipLaunchKernelGGL(softmax_full_cols_merge_kernel, dim3((unsigned)ctr_stream_grid(n, kThreads)), dim3(kThreads), 0,
                     s, ws, sp.parts, n, grad_q);
  return ctr_launch_status();
}
