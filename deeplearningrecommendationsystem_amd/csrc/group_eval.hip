// Sampled leave-one-out evaluation: each held-out positive ranked against k sampled negatives ("1 positive + 99
// negatives, HR@10 / NDCG@10").  The reference has no such stage (its evaluator/ranking.py ranks whole catalogues);
// the metrics that follow from the rank histogram are its Ranking's numbers on one-item ground truths.
//
// ctr_eval_candidates: the k DISTINCT unobserved items of every group.  Row s of cand (uint64 arithmetic, wrapping;
// mix64 and perm as loader.hip's header comment):
//     cand[s, 0]    = items[s]
//     gseed_s       = mix64(seed ^ mix64(s * 0x100000001B3 + 5))               (index 5: the loader uses 0..4)
//     q_t           = perm_{num_items}(gseed_s, 0, t),  t = 0 .. num_items - 1
//     cand[s, 1..k] = the first k of q_0, q_1, .. that are neither items[s] nor observed for users[s], in that order
// perm is a bijection of [0, num_items): the negatives are distinct, the scan ends after num_items values, and the
// draw with k' < k is a prefix of the draw with k.  Fewer than k eligible items: the rest is -1 and *fail_flag is
// raised.  A user id outside [0, num_users) writes 0 to the k slots and raises *err_flag; an inconsistent CSR row is
// read as empty and raises *err_flag (rank_eval.hip's csr_row).  tests/group_eval_numpy.py restates it.
// One wave per group: lane l of chunk c takes t = 64 c + l, computes q_t (fewer than four network evaluations on
// average) and probes the user's row by binary search; a ballot and the popcount of the lower lanes give the slot.
// The chain users[s] -> indptr -> probes is per group and cannot be shortened; the other resident waves cover it
// (loader.hip's last header paragraph).  At ml-100k shape a group scans 2.5 chunks on average.
//
// ctr_group_rank: rank[g] = #{ j in 1..k : !(scores[g, j] < scores[g, 0]) };  hist[r] += #{ g : rank[g] == r }.
// The one comparison puts ties and NaN (on either side) against the positive: a constant-output model ranks k, not 0.
// topk.hip's "lower index first" would let the positive, which sits at slot 0, win every tie, and saturated sigmoids
// tie often.  G lanes per group, G the smallest power of two >= 1 + k (2..64); rows are only 4-byte aligned in
// general, so every load is a dword and consecutive lanes read consecutive floats.  Counts go to an LDS histogram per
// workgroup and from there by 64-bit integer atomics into hist: exact, whatever the launch geometry is.  Bytes moved:
// 4 (1 + k) per group read, 4 per group written when ranks_out is given.
#include "ctr_common.h"
#include "loader_perm.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxK = CTR_GROUP_MAX_K;
constexpr int kMaxGrid = kCtrCUs * 8;

struct CandArgs {
  const int64_t* users;
  const int64_t* items;
  const int64_t* indptr;
  const int32_t* indices;
  int64_t n, nnz, num_users, num_items;
  int64_t* cand;
  int64_t ld;
  int32_t* err_flag;
  int32_t* fail_flag;
  uint64_t seed;
  int32_t k;
};

__global__ void __launch_bounds__(kBlock) eval_candidates_kernel(const CandArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * kWaves;
  const CTR_GLOBAL int32_t* ind = (const CTR_GLOBAL int32_t*)a.indices;
  for (int64_t s = wave; s < a.n; s += nwaves) {
    CTR_GLOBAL int64_t* row = (CTR_GLOBAL int64_t*)a.cand + s * a.ld;
    const int64_t u = ctr_ldg(a.users + s), pos = ctr_ldg(a.items + s);
    if (lane == 0) row[0] = pos;
    if (u < 0 || u >= a.num_users) {
      for (int j = lane; j < a.k; j += 64) row[1 + j] = 0;
      if (lane == 0 && a.err_flag) *(CTR_GLOBAL int32_t*)a.err_flag = 1;
      continue;
    }
    int64_t lo = ctr_ldg(a.indptr + u), hi = ctr_ldg(a.indptr + u + 1);
    if (lo < 0 || hi < lo || hi > a.nnz) {
      if (lane == 0 && a.err_flag) *(CTR_GLOBAL int32_t*)a.err_flag = 1;
      lo = hi = 0;
    }
    const uint64_t gseed = mix64(a.seed ^ mix64((uint64_t)s * 0x100000001B3ull + 5));
    const LoaderPerm pm = make_perm(a.num_items, gseed, 0, 1);
    int filled = 0;  // the same in every lane
    for (int64_t base = 0; base < a.num_items && filled < a.k; base += 64) {
      const int64_t t = base + lane;
      int64_t q = -1;
      bool ok = false;
      if (t < a.num_items) {
        q = loader_index(pm, t);
        int64_t x = lo, y = hi;
        while (x < y) {  // first entry of the row that is >= q
          const int64_t mid = x + ((y - x) >> 1);
          if (ind[mid] < (int32_t)q) x = mid + 1;
          else y = mid;
        }
        ok = q != pos && (x == hi || ind[x] != (int32_t)q);
      }
      const unsigned long long m = __ballot(ok);
      const int slot = filled + __popcll(m & ((1ull << lane) - 1ull));
      if (ok && slot < a.k) row[1 + slot] = q;
      filled += __popcll(m);
    }
    if (filled < a.k) {
      for (int j = filled + lane; j < a.k; j += 64) row[1 + j] = -1;
      if (lane == 0 && a.fail_flag) *(CTR_GLOBAL int32_t*)a.fail_flag = 1;
    }
  }
}

// G lanes per group, kBlock / G groups per workgroup pass
template <int G>
__global__ void __launch_bounds__(kBlock)
group_rank_kernel(const float* __restrict__ scores, int64_t ld, int64_t n, int k, int32_t* __restrict__ ranks_out,
                  unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_hist[kMaxK + 1];
  constexpr int kPer = kBlock / G;
  for (int r = threadIdx.x; r <= k; r += kBlock) s_hist[r] = 0;
  __syncthreads();
  const int sub = threadIdx.x & (G - 1);
  const int64_t tiles = (n + kPer - 1) / kPer;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t g = tile * kPer + threadIdx.x / G;
    const bool live = g < n;
    int cnt = 0;
    if (live) {
      const float* row = scores + g * ld;
      const float pos = row[0];
      for (int j = 1 + sub; j <= k; j += G) cnt += !(row[j] < pos) ? 1 : 0;
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (live && sub == 0) {
      if (ranks_out) ranks_out[g] = cnt;
      atomicAdd(&s_hist[cnt], 1u);
    }
  }
  __syncthreads();
  for (int r = threadIdx.x; r <= k; r += kBlock) {
    const uint32_t c = s_hist[r];
    if (c) atomicAdd(hist + r, (unsigned long long)c);
  }
}

template <int G>
void launch_rank(const float* scores, int64_t ld, int64_t n, int k, int32_t* ranks_out, int64_t* hist, hipStream_t st) {
  int64_t grid = ctr_ceil_div(n, kBlock / G);
  if (grid > kMaxGrid) grid = kMaxGrid;
  hipLaunchKernelGGL(group_rank_kernel<G>, dim3((unsigned)grid), dim3(kBlock), 0, st, scores, ld, n, k, ranks_out,
                     (unsigned long long*)hist);
}

}  // namespace

extern "C" int ctr_eval_candidates(const int64_t* users, const int64_t* items, int64_t n, const int64_t* indptr,
                                   const int32_t* indices, int64_t nnz, int64_t num_users, int64_t num_items, int k,
                                   uint64_t seed, int64_t* cand, int64_t ld, int32_t* err_flag, int32_t* fail_flag,
                                   void* stream) {
  CTR_REQUIRE(n >= 0 && k >= 1 && k <= kMaxK && ld >= 1 + (int64_t)k && nnz >= 0 && num_users >= 1 && num_items >= 1 &&
                  num_items < (1ll << 31),
              CTR_EINVAL);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(users && items && indptr && cand && (nnz == 0 || indices), CTR_EINVAL);
  CandArgs a;
  a.users = users;
  a.items = items;
  a.indptr = indptr;
  a.indices = indices;
  a.n = n;
  a.nnz = nnz;
  a.num_users = num_users;
  a.num_items = num_items;
  a.cand = cand;
  a.ld = ld;
  a.err_flag = err_flag;
  a.fail_flag = fail_flag;
  a.seed = seed;
  a.k = k;
  int64_t grid = ctr_ceil_div(n, kWaves);
  if (grid > kMaxGrid) grid = kMaxGrid;
  hipLaunchKernelGGL(eval_candidates_kernel, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream, a);
  return ctr_launch_status();
}

extern "C" int ctr_group_rank(const float* scores, int64_t ld, int64_t n, int k, int32_t* ranks_out, int64_t* hist,
                              void* stream) {
  CTR_REQUIRE(n >= 0 && k >= 1 && k <= kMaxK && ld >= 1 + (int64_t)k, CTR_EINVAL);
  if (n == 0) return CTR_OK;
  CTR_REQUIRE(scores && hist, CTR_EINVAL);
  CTR_REQUIRE(n <= (1ll << 40), CTR_ELIMIT);   // a workgroup's LDS counts stay far inside 32 bits
  hipStream_t st = (hipStream_t)stream;
  const int w = 1 + k;
  if (w <= 2) launch_rank<2>(scores, ld, n, k, ranks_out, hist, st);
  else if (w <= 4) launch_rank<4>(scores, ld, n, k, ranks_out, hist, st);
  else if (w <= 8) launch_rank<8>(scores, ld, n, k, ranks_out, hist, st);
  else if (w <= 16) launch_rank<16>(scores, ld, n, k, ranks_out, hist, st);
  else if (w <= 32) launch_rank<32>(scores, ld, n, k, ranks_out, hist, st);
  else launch_rank<64>(scores, ld, n, k, ranks_out, hist, st);
  return ctr_launch_status();
}
