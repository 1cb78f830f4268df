// Neighbourhood collaborative filtering (UserCF_Final.py / ItemCF_Final.py of the reference) on the matrix cores.
//
// ctr_cf_knn: fused cosine top-(k+1) self-join of a 0/1 int8 matrix X (rows x cols_pad, zero padded).  The cosine of
// two binary rows is c / sqrt(a b) with c = |N(u) n N(v)| an integer, so the K-loop is i8 MFMA with i32 accumulation
// and the counts are exact.  The rows x rows similarity matrix is never written: a workgroup owns kBM query rows,
// walks every column tile of kBN base rows in ascending order and keeps, per query row, the best 64 entries
//     (float32 sim bits << 32) | ~index                (larger = better, then smaller index; 0 = empty slot)
// sorted in LDS.  A tile's candidate is first screened with an fp32 estimate against the row's (k+1)-th entry and only
// the survivors get the exact key float32(c / sqrt(a b)) evaluated in float64; since an entry carries its index, the
// strict `>` against the threshold is the full tie rule and does not depend on the order the tiles arrive in.  The
// survivors of a row (at most 64 per tile) are sorted by one 64-lane bitonic network in registers and merged with the
// row's list by a half-cleaner + 6-stage bitonic merge.
//
//   workgroup: 4 waves x 32 query rows; per tile the wave computes a 32 x 64 block as two 32x32 accumulators
//   K-loop   : 128 bytes per step.  The B tile (64 rows x 128 B) goes global -> registers -> LDS, double buffered,
//              one barrier per step; each wave reads its own 32 A rows straight from global into registers (no other
//              wave uses them), prefetched one step ahead.
//   i8 operand map: lane l feeds row (l & 31) and 16 bytes of k; A and B take the SAME 16 bytes (64 (l >> 5) + 16 s
//              of the step), so whatever order the instruction gives the k inside a fragment, the dot product sums the
//              same pairs -- the counts are checked bitwise against an exact host restatement by the tests.
//
// ctr_usercf_scores / ctr_itemcf_scores: the predictions of prediction_dating (UserCF_Final.py:26-39) and
// prediction_item_based (ItemCF_Final.py:27-38) for a batch of users, float32 accumulated in neighbour order, rated
// items set to -inf (the caller ranks with ctr_topk_rows).
#include "ctr_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveRows = 32;
constexpr int kBM = kWaves * kWaveRows;   // query rows per workgroup
constexpr int kBN = 64;                   // base rows per column tile
constexpr int kKC = 128;                  // bytes of k per K-loop step
constexpr int kLdsRow = kKC + 16;         // padded B row in LDS (bytes)
constexpr int kList = CTR_CF_KNN_MAX_K;   // entries kept per query row (64)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }

// one value per lane, result descending over lanes 0..63
__device__ __forceinline__ u64 wave_sort_desc(u64 v, int lane) {
#pragma unroll
  for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const u64 o = shfl_xor64(v, stride);
      const bool lower = (lane & stride) == 0;
      const bool desc = (lane & size) == 0;
      v = (lower == desc) ? umax64(v, o) : umin64(v, o);
    }
  }
  return v;
}
// a bitonic sequence over 64 lanes -> descending
__device__ __forceinline__ u64 wave_merge_desc(u64 v, int lane) {
#pragma unroll
  for (int stride = 32; stride > 0; stride >>= 1) {
    const u64 o = shfl_xor64(v, stride);
    v = (lane & stride) == 0 ? umax64(v, o) : umin64(v, o);
  }
  return v;
}

__device__ __forceinline__ float cf_exact_sim(int c, int a, int b) {
  if (c == 0 || a == 0 || b == 0) return 0.0f;
  return (float)((double)c / sqrt((double)a * (double)b));
}

// the key of candidate (query count a, base row bidx with count b, intersection c), or 0 when it cannot enter a list
// whose current last entry is thr
__device__ __forceinline__ u64 cf_candidate(int c, int a, int b, int64_t bidx, int64_t rows, u64 thr, float tsim) {
  if (bidx >= rows) return 0ull;
  float sim = 0.0f;
  if (c != 0 && a != 0 && b != 0) {
    const float est = (float)c * rsqrtf((float)a * (float)b);   // within a few ulp of the exact value
    if (est * 1.0001f < tsim) return 0ull;
    sim = cf_exact_sim(c, a, b);
  }
  const u64 e = ((u64)__float_as_uint(sim) << 32) | (uint32_t)~(uint32_t)bidx;
  return e > thr ? e : 0ull;
}

__global__ void __launch_bounds__(kThreads)
cf_knn_kernel(const int8_t* __restrict__ x, int64_t rows, int64_t cols_pad, const int32_t* __restrict__ counts,
              int64_t q_begin, int64_t q_end, int kk, int64_t* __restrict__ idx_out, float* __restrict__ sim_out) {
  __shared__ __attribute__((aligned(16))) int8_t s_b[2][kBN * kLdsRow];
  __shared__ u64 s_list[kWaves][kWaveRows][kList];
  __shared__ int s_bcnt[kBN];
  __shared__ int s_qcnt[kBM];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int64_t q0 = q_begin + (int64_t)blockIdx.x * kBM;
  for (int i = tid; i < kWaves * kWaveRows * kList; i += kThreads) (&s_list[0][0][0])[i] = 0ull;
  for (int i = tid; i < kBM; i += kThreads) s_qcnt[i] = q0 + i < q_end ? counts[q0 + i] : 0;

  const int64_t qa = q0 + kWaveRows * w + r32;   // the A row this lane feeds
  const bool a_ok = qa < q_end;
  const int8_t* arow = x + (a_ok ? qa : 0) * cols_pad;
  const int nch = (int)((cols_pad + kKC - 1) / kKC);
  const v4i zero4 = {0, 0, 0, 0};

  for (int64_t t0 = 0; t0 < rows; t0 += kBN) {
    __syncthreads();   // the previous tile's epilogue is done with s_bcnt and the B buffers
    if (tid < kBN) s_bcnt[tid] = t0 + tid < rows ? counts[t0 + tid] : 0;

    v4i breg[2], anext[4], acur[4];
    auto load_b = [&](int ch) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int id = tid + kThreads * i, row = id >> 3, c16 = id & 7;
        const int64_t br = t0 + row, off = (int64_t)ch * kKC + 16 * c16;
        breg[i] = (br < rows && off < cols_pad) ? *(const v4i*)(x + br * cols_pad + off) : zero4;
      }
    };
    auto load_a = [&](int ch) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t off = (int64_t)ch * kKC + 64 * h + 16 * s;
        anext[s] = (a_ok && off < cols_pad) ? *(const v4i*)(arow + off) : zero4;
      }
    };
    load_b(0);
    load_a(0);
    v16i acc0, acc1;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc0[g] = acc1[g] = 0;

    for (int ch = 0; ch < nch; ++ch) {
      int8_t* sb = s_b[ch & 1];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int id = tid + kThreads * i;
        *(v4i*)(sb + (id >> 3) * kLdsRow + 16 * (id & 7)) = breg[i];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) acur[s] = anext[s];
      __syncthreads();
      if (ch + 1 < nch) {
        load_b(ch + 1);
        load_a(ch + 1);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const v4i b0 = *(const v4i*)(sb + r32 * kLdsRow + 64 * h + 16 * s);
        const v4i b1 = *(const v4i*)(sb + (32 + r32) * kLdsRow + 64 * h + 16 * s);
        acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(acur[s], b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(acur[s], b1, acc1, 0, 0, 0);
      }
    }

    // ---- epilogue: accumulator register g of lane l is (row (g&3) + 8(g>>2) + 4h, column 32 nb + (l&31))
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int rr = (g & 3) + 8 * (g >> 2) + 4 * h;
      const int a = s_qcnt[kWaveRows * w + rr];
      const u64 thr = s_list[w][rr][kk - 1];
      const float tsim = __uint_as_float((uint32_t)(thr >> 32));
      const u64 e0 = cf_candidate(acc0[g], a, s_bcnt[r32], t0 + r32, rows, thr, tsim);
      const u64 e1 = cf_candidate(acc1[g], a, s_bcnt[32 + r32], t0 + 32 + r32, rows, thr, tsim);
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int row = (g & 3) + 8 * (g >> 2) + 4 * hh;
        if (q0 + kWaveRows * w + row >= q_end) continue;   // wave-uniform
        // lane l takes column l of this row: columns 0..31 from acc0, 32..63 from acc1 of the row's lane half
        const u64 x0 = shfl64(e0, 32 * hh + r32), x1 = shfl64(e1, 32 * hh + r32);
        u64 v = lane < 32 ? x0 : x1;
        if (__ballot(v != 0ull) == 0ull) continue;
        v = wave_sort_desc(v, lane);
        const u64 rev = shfl64(v, 63 - lane);
        const u64 m = umax64(s_list[w][row][lane], rev);
        s_list[w][row][lane] = wave_merge_desc(m, lane);
      }
    }
  }

  for (int row = 0; row < kWaveRows; ++row) {
    const int64_t q = q0 + kWaveRows * w + row;
    if (q >= q_end) break;
    for (int j = lane; j < kk; j += 64) {
      const u64 e = s_list[w][row][j];
      const int64_t o = (q - q_begin) * kk + j;
      idx_out[o] = e ? (int64_t)(uint32_t)~(uint32_t)e : -1;
      sim_out[o] = e ? __uint_as_float((uint32_t)(e >> 32)) : 0.0f;
    }
  }
}

// ---- predictions ----------------------------------------------------------------------------------------------

constexpr int kScoreItemsPerThread = 4;

// one workgroup per (user, block of 1024 items); four items per thread from one 32-bit load per neighbour row
__global__ void __launch_bounds__(kThreads)
usercf_scores_kernel(const int8_t* __restrict__ x, int64_t num_users, int64_t cols_pad, int64_t num_items,
                     const int64_t* __restrict__ nbr, const float* __restrict__ nsim, int k,
                     const int64_t* __restrict__ users, float* __restrict__ out, int64_t ldo) {
  __shared__ int64_t s_v[CTR_CF_KNN_MAX_K];
  __shared__ float s_s[CTR_CF_KNN_MAX_K];
  const int64_t b = blockIdx.y;
  const int64_t u = users[b];
  const bool u_ok = u >= 0 && u < num_users;
  if (threadIdx.x < k) {
    const int64_t v = u_ok ? nbr[u * k + threadIdx.x] : -1;
    s_v[threadIdx.x] = (v >= 0 && v < num_users) ? v : -1;
    s_s[threadIdx.x] = u_ok ? nsim[u * k + threadIdx.x] : 0.0f;
  }
  __syncthreads();
  const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kScoreItemsPerThread;
  if (i0 >= num_items) return;
  float* orow = out + b * ldo;
  if (!u_ok) {
    for (int t = 0; t < kScoreItemsPerThread && i0 + t < num_items; ++t) orow[i0 + t] = -INFINITY;
    return;
  }
  float num[kScoreItemsPerThread] = {0.0f, 0.0f, 0.0f, 0.0f};
  float den = 0.0f;
  for (int j = 0; j < k; ++j) {
    const int64_t v = s_v[j];
    if (v < 0) continue;
    const float s = s_s[j];
    const uint32_t r = *(const uint32_t*)(x + v * cols_pad + i0);   // cols_pad % 64 == 0: in the padded row
#pragma unroll
    for (int t = 0; t < kScoreItemsPerThread; ++t) num[t] = num[t] + (((r >> (8 * t)) & 0xffu) ? s : 0.0f);
    den = den + s;
  }
  const uint32_t mine = *(const uint32_t*)(x + u * cols_pad + i0);
#pragma unroll
  for (int t = 0; t < kScoreItemsPerThread; ++t) {
    if (i0 + t >= num_items) break;
    orow[i0 + t] = ((mine >> (8 * t)) & 0xffu) ? -INFINITY : (den != 0.0f ? num[t] / den : 0.0f);
  }
}

constexpr int kItemBlock = 2048;    // items per workgroup of ctr_itemcf_scores
constexpr int kMaxUsersPerGroup = 16;
constexpr int kBitmapBytes = 65536; // LDS for the users' rows as bitmaps

// one workgroup per (group of up to 16 users, block of 2048 items): the users' rows as bitmaps in LDS, the item
// neighbour table streamed once per group
__global__ void __launch_bounds__(kThreads)
itemcf_scores_kernel(const int8_t* __restrict__ x, int64_t num_users, int64_t cols_pad, int64_t num_items,
                     const int64_t* __restrict__ nbr, const float* __restrict__ nsim, int k,
                     const int64_t* __restrict__ users, int64_t batch, int ub, float* __restrict__ out, int64_t ldo) {
  extern __shared__ uint32_t s_bits[];   // [ub][words]
  const int64_t words = cols_pad / 32;
  const int64_t b0 = (int64_t)blockIdx.y * ub;
  const int nu = (int)(batch - b0 < ub ? batch - b0 : ub);
  for (int64_t wi = threadIdx.x; wi < (int64_t)nu * words; wi += kThreads) {
    const int ul = (int)(wi / words);
    const int64_t word = wi - (int64_t)ul * words;
    const int64_t u = users[b0 + ul];
    uint32_t bits = 0;
    if (u >= 0 && u < num_users) {
      const v4i* p = (const v4i*)(x + u * cols_pad + 32 * word);
      const v4i lo = p[0], hi = p[1];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int by = 0; by < 4; ++by) {
          bits |= (((uint32_t)lo[q] >> (8 * by)) & 0xffu ? 1u : 0u) << (4 * q + by);
          bits |= (((uint32_t)hi[q] >> (8 * by)) & 0xffu ? 1u : 0u) << (16 + 4 * q + by);
        }
      }
    }
    s_bits[wi] = bits;
  }
  __syncthreads();
  const int64_t iend = ((int64_t)blockIdx.x + 1) * kItemBlock < num_items ? ((int64_t)blockIdx.x + 1) * kItemBlock
                                                                           : num_items;
  for (int64_t i = (int64_t)blockIdx.x * kItemBlock + threadIdx.x; i < iend; i += kThreads) {
    float num[kMaxUsersPerGroup];
#pragma unroll
    for (int t = 0; t < kMaxUsersPerGroup; ++t) num[t] = 0.0f;
    float den = 0.0f;
    for (int j = 0; j < k; ++j) {
      const int64_t jj = nbr[i * k + j];
      if (jj < 0 || jj >= num_items) continue;
      const float s = nsim[i * k + j];
      const int64_t wd = jj >> 5;
      const int bit = (int)(jj & 31);
#pragma unroll
      for (int t = 0; t < kMaxUsersPerGroup; ++t)
        if (t < nu) num[t] = num[t] + (((s_bits[t * words + wd] >> bit) & 1u) ? s : 0.0f);
      den = den + s;
    }
#pragma unroll
    for (int t = 0; t < kMaxUsersPerGroup; ++t) {
      if (t >= nu) break;
      const int64_t u = users[b0 + t];
      float p;
      if (u < 0 || u >= num_users || ((s_bits[t * words + (i >> 5)] >> (i & 31)) & 1u)) p = -INFINITY;
      else p = den != 0.0f ? num[t] / den : 0.0f;
      out[(b0 + t) * ldo + i] = p;
    }
  }
}

}  // namespace

extern "C" int ctr_cf_knn(const int8_t* x, int64_t rows, int64_t cols_pad, const int32_t* counts, int64_t q_begin,
                          int64_t q_count, int kk, int64_t* idx_out, float* sim_out, void* stream) {
  CTR_REQUIRE(rows >= 1 && cols_pad >= 64 && cols_pad % 64 == 0 && kk >= 1, CTR_EINVAL);
  CTR_REQUIRE(q_begin >= 0 && q_count >= 0 && q_begin <= rows && q_count <= rows - q_begin, CTR_EINVAL);
  CTR_REQUIRE(kk <= CTR_CF_KNN_MAX_K && rows < (1ll << 31), CTR_ELIMIT);
  if (q_count == 0) return CTR_OK;
  CTR_REQUIRE(x && counts && idx_out && sim_out, CTR_EINVAL);
  CTR_REQUIRE(ctr_aligned16(x), CTR_EALIGN);
  hipLaunchKernelGGL(cf_knn_kernel, dim3((unsigned)ctr_ceil_div(q_count, kBM)), dim3(kThreads), 0, (hipStream_t)stream,
                     x, rows, cols_pad, counts, q_begin, q_begin + q_count, kk, idx_out, sim_out);
  return ctr_launch_status();
}

extern "C" int ctr_usercf_scores(const int8_t* x, int64_t num_users, int64_t cols_pad, int64_t num_items,
                                 const int64_t* nbr, const float* nsim, int k, const int64_t* users, int64_t batch,
                                 float* out, int64_t ldo, void* stream) {
  CTR_REQUIRE(num_users >= 1 && num_items >= 1 && cols_pad >= num_items && cols_pad % 64 == 0, CTR_EINVAL);
  CTR_REQUIRE(k >= 0 && batch >= 0 && ldo >= num_items, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_CF_KNN_MAX_K && batch <= 65535, CTR_ELIMIT);
  if (batch == 0) return CTR_OK;
  CTR_REQUIRE(x && users && out && (k == 0 || (nbr && nsim)), CTR_EINVAL);
  CTR_REQUIRE(ctr_aligned16(x), CTR_EALIGN);
  const int64_t gx = ctr_ceil_div(num_items, (int64_t)kThreads * kScoreItemsPerThread);
  hipLaunchKernelGGL(usercf_scores_kernel, dim3((unsigned)gx, (unsigned)batch), dim3(kThreads), 0,
                     (hipStream_t)stream, x, num_users, cols_pad, num_items, nbr, nsim, k, users, out, ldo);
  return ctr_launch_status();
}

extern "C" int ctr_itemcf_scores(const int8_t* x, int64_t num_users, int64_t cols_pad, int64_t num_items,
                                 const int64_t* nbr, const float* nsim, int k, const int64_t* users, int64_t batch,
                                 float* out, int64_t ldo, void* stream) {
  CTR_REQUIRE(num_users >= 1 && num_items >= 1 && cols_pad >= num_items && cols_pad % 64 == 0, CTR_EINVAL);
  CTR_REQUIRE(k >= 0 && batch >= 0 && ldo >= num_items, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_CF_KNN_MAX_K && cols_pad / 8 <= kBitmapBytes, CTR_ELIMIT);
  if (batch == 0) return CTR_OK;
  CTR_REQUIRE(x && users && out && (k == 0 || (nbr && nsim)), CTR_EINVAL);
  CTR_REQUIRE(ctr_aligned16(x), CTR_EALIGN);
  int64_t ub = kBitmapBytes / (cols_pad / 8);
  if (ub > kMaxUsersPerGroup) ub = kMaxUsersPerGroup;
  if (ub > batch) ub = batch;
  const int64_t gy = ctr_ceil_div(batch, ub);
  CTR_REQUIRE(gy <= 65535, CTR_ELIMIT);
  const size_t lds = (size_t)ub * (size_t)(cols_pad / 8);
  hipLaunchKernelGGL(itemcf_scores_kernel, dim3((unsigned)ctr_ceil_div(num_items, kItemBlock), (unsigned)gy),
                     dim3(kThreads), lds, (hipStream_t)stream, x, num_users, cols_pad, num_items, nbr, nsim, k, users,
                     batch, (int)ub, out, ldo);
  return ctr_launch_status();
}
