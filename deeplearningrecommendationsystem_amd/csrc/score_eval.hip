// Score-level evaluation of a CTR model: the pointwise numbers (log-loss, confusion counts, calibration, RMSE) in one
// pass, and the integer counts behind every user's own AUC, from which GAUC follows (the impression-weighted mean of
// the per-user AUCs, the DIN paper's metric).  The reference has neither: its "ROC AUC" is the balanced accuracy of the
// thresholded predictions (evaluator/evaluator.py).  tests/score_numpy.py restates both entry points.
//
// Class rule, everywhere: a sample is POSITIVE iff target > 0.5f (a NaN target is negative); a prediction is HARD
// iff prob >= 0.5f (a NaN prediction is not).
//
// ctr_score_counts.  counts = {positives, negatives, tp, fp, fn, tn, bad, 0} with bad = #{prob NaN or outside [0, 1]},
// ADDED by 64-bit integer atomics.  sums[c] = the four sums over chunk c = samples [c 65536, min(n, (c + 1) 65536)):
//     sums[c][0] = sum (double) -(y max(logf(p), -100) + (1 - y) max(logf(1.0f - p), -100))      bce_fwd_kernel's fp32 term;
//                                                               fmaxf drops a NaN, so a NaN logarithm counts as -100
//     sums[c][1] = sum (double) p        sums[c][2] = sum ((double) p - (double) y)^2        sums[c][3] = sum (double) y
// One workgroup sums one chunk: thread t adds the elements t, t + 256, .. of the chunk in that order in double, an xor
// butterfly over 32, 16, .. 1 lanes follows, then thread 0 adds the four waves in order and STORES the row.  A row is a
// function of its chunk's data alone -- not of n, of the grid, or of the workgroup that drew the chunk -- and the host
// adds the rows in chunk order: the log-loss is bitwise reproducible.  Bytes moved: 8 per sample read, 32 per chunk
// written.
//
// ctr_gauc_groups.  Group g = the samples order[offsets[g] .. offsets[g + 1]).  With i over its positives and j over
// its negatives,
//     pos_out[g] = #positives     neg_out[g] = #negatives
//     u2_out[g] += sum_i sum_j ( 2 [prob_j < prob_i] + [prob_j == prob_i] )              AUC_g = u2 / (2 pos neg)
// IEEE comparisons and nothing else: a NaN on either side adds 0 (it counts against the positive, as in
// ctr_group_rank), -0.0 == 0.0.  Integers only, u2 <= 2 pos neg < 2^62: the result is exact and does not depend on the
// launch geometry or on the order of the atomics.  An order entry outside [0, n) is skipped (neither class) and raises
// *err_flag; so does a work item that names a group outside [0, num_groups), offsets outside 0 <= lo <= hi <= n, a
// small group longer than 64 or a slab that starts outside its group, and that item is skipped whole.
// Work split, from the plan the caller builds once per evaluation set (evaluator.score.UserGroups):
//   small arm  one wave per group of <= CTR_GAUC_SMALL samples: lane l holds sample l, the loop over j < size
//              broadcasts sample j from its lane, the class counts are ballots.
//   slab arm   one 256-thread workgroup per (group, first): each thread keeps 4 of the slab's CTR_GAUC_SLAB samples in
//              registers (NaN in place of every score that is not a positive's), the WHOLE group streams through LDS in
//              tiles of 1024 scores (NaN in place of every score that is not a negative's), and every thread reads the
//              same LDS address at a time: a broadcast, no bank conflict.  2 (t < s) + (t == s) is then zero for every
//              pair that must not count, and the inner loop has no branch.  The slab with first == 0 also stores the
//              class counts; it sees the whole group anyway.  32-bit sums per tile, 64-bit per slab, one 64-bit
//              integer vector atomic per slab into u2_out.
// Pairs evaluated: sum over groups of size x (size rounded up to slabs; small groups: size x size).  Bytes moved:
// 12 per sample in the small arm; 12 x size per slab in the slab arm (a group of s samples is read ceil(s / 1024)
// times, from L2 after the first).
#include "ctr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxGrid = kCtrCUs * 8;
constexpr int64_t kChunk = CTR_SCORE_CHUNK;
constexpr int kSmall = CTR_GAUC_SMALL;
constexpr int kSlab = CTR_GAUC_SLAB;
constexpr int kPer = kSlab / kBlock;   // samples a thread keeps; a tile is as long as a slab

static_assert(kSmall == 64, "the small arm holds one sample per lane");
static_assert(kPer == 4 && kPer * kBlock == kSlab, "the slab arm keeps 4 samples per thread");
static_assert(kChunk % kBlock == 0, "a chunk is whole passes of the workgroup");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kBlock)
score_counts_kernel(const float* __restrict__ prob, const float* __restrict__ target, int64_t n, int64_t chunks,
                    unsigned long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ double s_sum[kWaves][4];
  __shared__ int s_cnt[kWaves][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int npos = 0, ntp = 0, nfp = 0, nfn = 0, nbad = 0, nall = 0;   // a thread sees far fewer than 2^31 samples (n < 2^62 / grid)
  for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    const int64_t base = c * kChunk;
    const int len = (int)(n - base < kChunk ? n - base : kChunk);
    const float* p = prob + base;
    const float* y = target + base;
    double bce = 0.0, sp = 0.0, se = 0.0, sy = 0.0;
    for (int i0 = threadIdx.x; i0 < len; i0 += kBlock * 4) {
      float pv[4], yv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {   // four loads in flight; the additions below keep the order t, t + 256, ..
        const int i = i0 + r * kBlock;
        pv[r] = i < len ? p[i] : 0.0f;
        yv[r] = i < len ? y[i] : 0.0f;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (i0 + r * kBlock < len) {
          const float lp = fmaxf(logf(pv[r]), -100.0f), l1p = fmaxf(logf(1.0f - pv[r]), -100.0f);
          const float term = -(yv[r] * lp + (1.0f - yv[r]) * l1p);
          const double d = (double)pv[r] - (double)yv[r];
          bce += (double)term;
          sp += (double)pv[r];
          se = __dadd_rn(se, __dmul_rn(d, d));   // the rounded square, then the rounded sum: no fused multiply-add
          sy += (double)yv[r];
          const bool pos = yv[r] > 0.5f, hard = pv[r] >= 0.5f;
          nall += 1;
          npos += pos ? 1 : 0;
          ntp += (pos && hard) ? 1 : 0;
          nfp += (!pos && hard) ? 1 : 0;
          nfn += (pos && !hard) ? 1 : 0;
          nbad += !(pv[r] >= 0.0f && pv[r] <= 1.0f) ? 1 : 0;
        }
      }
    }
    bce = wave_sum_f64(bce);
    sp = wave_sum_f64(sp);
    se = wave_sum_f64(se);
    sy = wave_sum_f64(sy);
    if (lane == 0) {
      s_sum[wave][0] = bce;
      s_sum[wave][1] = sp;
      s_sum[wave][2] = se;
      s_sum[wave][3] = sy;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      double v = s_sum[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v += s_sum[w][threadIdx.x];
      sums[c * 4 + threadIdx.x] = v;
    }
    __syncthreads();
  }
  npos = wave_sum_i32(npos);
  ntp = wave_sum_i32(ntp);
  nfp = wave_sum_i32(nfp);
  nfn = wave_sum_i32(nfn);
  nbad = wave_sum_i32(nbad);
  nall = wave_sum_i32(nall);
  if (lane == 0) {
    s_cnt[wave][0] = npos;
    s_cnt[wave][1] = ntp;
    s_cnt[wave][2] = nfp;
    s_cnt[wave][3] = nfn;
    s_cnt[wave][4] = nbad;
    s_cnt[wave][5] = nall;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t[6];
    for (int k = 0; k < 6; ++k) {
      t[k] = 0;
      for (int w = 0; w < kWaves; ++w) t[k] += s_cnt[w][k];
    }
    const long long pos = t[0], tp = t[1], fp = t[2], fn = t[3], bad = t[4], all = t[5];
    const long long neg = all - pos, tn = neg - fp;
    if (pos) atomicAdd(counts + 0, (unsigned long long)pos);
    if (neg) atomicAdd(counts + 1, (unsigned long long)neg);
    if (tp) atomicAdd(counts + 2, (unsigned long long)tp);
    if (fp) atomicAdd(counts + 3, (unsigned long long)fp);
    if (fn) atomicAdd(counts + 4, (unsigned long long)fn);
    if (tn) atomicAdd(counts + 5, (unsigned long long)tn);
    if (bad) atomicAdd(counts + 6, (unsigned long long)bad);
  }
}

struct GaucArgs {
  const float* prob;
  const float* target;
  const int32_t* order;
  const int64_t* offsets;
  const int32_t* small_groups;
  const int32_t* slab_group;
  const int32_t* slab_first;
  int32_t* pos_out;
  int32_t* neg_out;
  unsigned long long* u2_out;
  int32_t* err_flag;
  int64_t n, num_groups, num_small, num_slabs;
};

__device__ __forceinline__ void raise(const GaucArgs& a) {
  if (a.err_flag) *(CTR_GLOBAL int32_t*)a.err_flag = 1;
}

// [lo, hi) of group g, or false (flag raised) when the plan is not one over n samples
__device__ __forceinline__ bool group_range(const GaucArgs& a, int64_t g, int64_t& lo, int64_t& hi) {
  if (g < 0 || g >= a.num_groups) {
    raise(a);
    return false;
  }
  lo = ctr_ldg(a.offsets + g);
  hi = ctr_ldg(a.offsets + g + 1);
  if (lo < 0 || hi < lo || hi > a.n) {
    raise(a);
    return false;
  }
  return true;
}

// sample at position `at` of order (at inside [0, n)): its score and class, cls = 1 positive, 0 negative, -1 skipped
__device__ __forceinline__ void load_sample(const GaucArgs& a, int64_t at, float& p, int& cls) {
  const int64_t idx = a.order[at];
  p = 0.0f;
  cls = -1;
  if (idx < 0 || idx >= a.n) {
    raise(a);
    return;
  }
  p = a.prob[idx];
  cls = a.target[idx] > 0.5f ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) gauc_small_kernel(const GaucArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const float nanf_ = __builtin_nanf("");
  for (int64_t w = wave0; w < a.num_small; w += nwaves) {
    const int64_t g = a.small_groups[w];
    int64_t lo = 0, hi = 0;
    if (!group_range(a, g, lo, hi)) continue;   // wave-uniform
    if (hi - lo > kSmall) {
      raise(a);
      continue;
    }
    const int size = (int)(hi - lo);
    float p = 0.0f;
    int cls = -1;
    if (lane < size) load_sample(a, lo + lane, p, cls);
    const float s = cls == 1 ? p : nanf_;   // this lane's positive
    const float t = cls == 0 ? p : nanf_;   // this lane's negative, broadcast below
    int u = 0;
    for (int j = 0; j < size; ++j) {
      const float tj = __shfl(t, j, 64);
      u += 2 * (tj < s ? 1 : 0) + (tj == s ? 1 : 0);
    }
    u = wave_sum_i32(u);   // <= 2 * 64 * 64
    const unsigned long long mpos = __ballot(cls == 1), mneg = __ballot(cls == 0);
    if (lane == 0) {
      a.pos_out[g] = __popcll(mpos);
      a.neg_out[g] = __popcll(mneg);
      if (u) atomicAdd(a.u2_out + g, (unsigned long long)u);
    }
  }
}

__global__ void __launch_bounds__(kBlock) gauc_slab_kernel(const GaucArgs a) {
  __shared__ __attribute__((aligned(16))) float s_tile[kSlab];
  __shared__ long long s_u[kWaves];
  __shared__ int s_cls[kWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float nanf_ = __builtin_nanf("");
  for (int64_t w = blockIdx.x; w < a.num_slabs; w += gridDim.x) {
    const int64_t g = a.slab_group[w];
    const int64_t first = a.slab_first[w];
    int64_t lo = 0, hi = 0;
    if (!group_range(a, g, lo, hi)) continue;   // block-uniform
    const int64_t size = hi - lo;
    if (first < 0 || first >= size) {
      raise(a);
      continue;
    }
    float s[kPer];   // the slab's positives, NaN elsewhere
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const int64_t at = first + threadIdx.x + r * kBlock;
      float p = 0.0f;
      int cls = -1;
      if (at < size) load_sample(a, lo + at, p, cls);
      s[r] = cls == 1 ? p : nanf_;
    }
    long long u = 0;
    int npos = 0, nneg = 0;
    for (int64_t tile = 0; tile < size; tile += kSlab) {
      __syncthreads();   // the previous tile has been read
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        const int64_t at = tile + threadIdx.x + r * kBlock;
        float p = 0.0f;
        int cls = -1;
        if (at < size) load_sample(a, lo + at, p, cls);
        s_tile[threadIdx.x + r * kBlock] = cls == 0 ? p : nanf_;
        npos += cls == 1 ? 1 : 0;
        nneg += cls == 0 ? 1 : 0;
      }
      __syncthreads();
      const int64_t left = size - tile;
      const int len4 = (int)(left < kSlab ? (left + 3) & ~(int64_t)3 : kSlab);   // the slots past `left` hold NaN
      int acc = 0;   // <= 2 * 4 * 1024 per tile
      for (int j = 0; j < len4; j += 4) {
        const float4 t = *(const float4*)(s_tile + j);   // every lane the same address: a broadcast
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
          acc += 2 * (t.x < s[r] ? 1 : 0) + (t.x == s[r] ? 1 : 0);
          acc += 2 * (t.y < s[r] ? 1 : 0) + (t.y == s[r] ? 1 : 0);
          acc += 2 * (t.z < s[r] ? 1 : 0) + (t.z == s[r] ? 1 : 0);
          acc += 2 * (t.w < s[r] ? 1 : 0) + (t.w == s[r] ? 1 : 0);
        }
      }
      u += acc;
    }
    u = wave_sum_i64(u);
    npos = wave_sum_i32(npos);
    nneg = wave_sum_i32(nneg);
    if (lane == 0) {
      s_u[wave] = u;
      s_cls[wave][0] = npos;
      s_cls[wave][1] = nneg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long long total = 0;
      int tp = 0, tn = 0;
      for (int k = 0; k < kWaves; ++k) {
        total += s_u[k];
        tp += s_cls[k][0];
        tn += s_cls[k][1];
      }
      if (first == 0) {
        a.pos_out[g] = tp;
        a.neg_out[g] = tn;
      }
      if (total) atomicAdd(a.u2_out + g, (unsigned long long)total);
    }
    __syncthreads();   // s_u / s_cls are free again
  }
}

}  // namespace

extern "C" int ctr_score_counts(const float* prob, const float* target, int64_t n, int64_t* counts, double* sums,
                                void* stream) {
  CTR_REQUIRE(n >= 0, CTR_EINVAL);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(prob && target && counts && sums, CTR_EINVAL);
  CTR_REQUIRE(n < (1ll << 48), CTR_ELIMIT);   // a thread's 32-bit counters: n / 2048 workgroups / 256 threads < 2^31
  const int64_t chunks = ctr_ceil_div(n, kChunk);
  const int64_t grid = chunks < kMaxGrid ? chunks : kMaxGrid;
  hipLaunchKernelGGL(score_counts_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, prob, target, n,
                     chunks, (unsigned long long*)counts, sums);
  return ctr_launch_status();
}

extern "C" int ctr_gauc_groups(const float* prob, const float* target, int64_t n, const int32_t* order,
                               const int64_t* offsets, int64_t num_groups, const int32_t* small_groups,
                               int64_t num_small, const int32_t* slab_group, const int32_t* slab_first,
                               int64_t num_slabs, int32_t* pos_out, int32_t* neg_out, int64_t* u2_out,
                               int32_t* err_flag, void* stream) {
  CTR_REQUIRE(n >= 0 && num_groups >= 0 && num_small >= 0 && num_slabs >= 0, CTR_EINVAL);
  if (num_groups == 0) return CTR_OK;
  CTR_REQUIRE(n < (1ll << 31) && num_groups < (1ll << 31), CTR_ELIMIT);
  CTR_REQUIRE(offsets && pos_out && neg_out && u2_out, CTR_EINVAL);
  CTR_REQUIRE(n == 0 || (prob && target && order), CTR_EINVAL);
  CTR_REQUIRE(num_small == 0 || small_groups, CTR_EINVAL);
  CTR_REQUIRE(num_slabs == 0 || (slab_group && slab_first), CTR_EINVAL);
  GaucArgs a;
  a.prob = prob;
  a.target = target;
  a.order = order;
  a.offsets = offsets;
  a.small_groups = small_groups;
  a.slab_group = slab_group;
  a.slab_first = slab_first;
  a.pos_out = pos_out;
  a.neg_out = neg_out;
  a.u2_out = (unsigned long long*)u2_out;
  a.err_flag = err_flag;
  a.n = n;
  a.num_groups = num_groups;
  a.num_small = num_small;
  a.num_slabs = num_slabs;
  hipStream_t st = (hipStream_t)stream;
  if (num_small > 0) {
    int64_t grid = ctr_ceil_div(num_small, kWaves);
    if (grid > kMaxGrid) grid = kMaxGrid;
    hipLaunchKernelGGL(gauc_small_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, a);
  }
  if (num_slabs > 0) {
    const int64_t grid = num_slabs < kMaxGrid * 4 ? num_slabs : kMaxGrid * 4;
    hipLaunchKernelGGL(gauc_slab_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, a);
  }
  return ctr_launch_status();
}
