// Top-k ranking evaluation: the reference's evaluator/ranking.py (Ranking: P/R/F1@k, MAP@k, NDCG@k, MRR) and
// data/reader.py:137-159 (remove_itemid), on the device.  Every per-user quantity is computed by one workgroup,
// integers exactly and the float sums in float64 in the reference's order, and written to a (rows, 7) float64
// partials row: same, rec, real, ap, dcg, idcg, rr.  No float atomics; the host reduces the partials in a fixed order.
//
// Id sets are CSRs (offsets, ids sorted ascending per row) in global memory, probed by binary search.  A CSR row whose
// offsets are not monotone or leave [0, nnz) is read as empty and raises bit CTR_RANK_ERR_OFFSETS of *err_flag, so a
// bad CSR never reads out of bounds.
//
//   ctr_rank_filter          per-row stream compaction of a ranking against an exclusion set (order kept)
//   ctr_rank_metrics_lists   partials from explicit predicted rows; |set(p[:k])| through a per-user hash set in a
//                            caller-given workspace (any k, any ids but INT64_MIN)
//   ctr_rank_mask            writes CTR_RANK_MASK_BITS over the excluded items of a score chunk (key 0 in topk.hip's
//                            order: below every other float, -inf and NaN included)
//   ctr_rank_metrics_scores  partials from masked score rows + their top-k, never materialising the full ranking
#include "ctr_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kListsMaxGrid = 8192;
constexpr unsigned long long kEmpty = 0x8000000000000000ull;   // INT64_MIN: the hash set's empty slot

struct Partials {
  double same, rec, real, ap, dcg, idcg, rr;
};

__device__ __forceinline__ uint32_t ordered_key(float v) {   // topk.hip's key: ascending in the float order
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long entry(uint32_t key, uint32_t idx) {
  return ((unsigned long long)key << 32) | (uint32_t)~idx;     // larger = ranked earlier (topk.hip's entry())
}

// row u of a CSR; an inconsistent row is empty and flagged
__device__ __forceinline__ void csr_row(const int64_t* off, int64_t u, int64_t nnz, int32_t* err, int64_t& lo,
                                        int64_t& hi) {
  lo = off[u];
  hi = off[u + 1];
  if (lo < 0 || hi < lo || hi > nnz) {
    if (threadIdx.x == 0) atomicOr(err, CTR_RANK_ERR_OFFSETS);
    lo = hi = 0;
  }
}

// lower_bound membership test
__device__ __forceinline__ bool member(const int64_t* ids, int64_t lo, int64_t hi, int64_t v) {
  int64_t a = lo, b = hi;
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (ids[mid] < v) a = mid + 1;
    else b = mid;
  }
  return a < hi && ids[a] == v;
}

// number of distinct values of a sorted CSR row
__device__ __forceinline__ int64_t distinct_local(const int64_t* ids, int64_t lo, int64_t hi) {
  int64_t c = 0;
  for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) c += (j == lo || ids[j] != ids[j - 1]) ? 1 : 0;
  return c;
}

// workgroup sum of a per-thread integer (exact; s_red holds kWaves entries)
__device__ __forceinline__ long long block_sum(long long v, long long* s_red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += s_red[w];
  return t;
}

// Walks hit flags of positions [0, len) in order, kThreads at a time.  flag(j) gives the flag of position j < len.
// Thread 0 accumulates AP's score and dcg over positions < kk (the reference's order), counts every hit and records
// the first hit position.
struct Walk {
  double score = 0.0, dcg = 0.0;
  long long hits_k = 0, hits = 0, first = -1;
};

template <class Flag>
__device__ void walk(int64_t len, int64_t kk, Flag flag, unsigned long long* s_mask, Walk& w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t base = 0; base < len; base += kThreads) {
    const int64_t j = base + threadIdx.x;
    const bool hit = j < len && flag(j);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_mask[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int wv = 0; wv < kWaves; ++wv) {
        unsigned long long mm = s_mask[wv];
        if (mm && w.first < 0) w.first = base + wv * 64 + __ffsll((long long)mm) - 1;
        w.hits += __popcll(mm);
        while (mm) {
          const int64_t pos = base + wv * 64 + __ffsll((long long)mm) - 1;
          if (pos >= kk) break;
          w.hits_k += 1;
          w.score += (double)w.hits_k / (double)(pos + 1);
          w.dcg += 1.0 / log2((double)(pos + 2));
          mm &= mm - 1ull;
        }
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double ideal_dcg(int64_t ones) {
  double s = 0.0;
  for (int64_t j = 0; j < ones; ++j) s += 1.0 / log2((double)(j + 2));
  return s;
}

__device__ __forceinline__ void store(double* out, const Partials& p) {
  out[0] = p.same;
  out[1] = p.rec;
  out[2] = p.real;
  out[3] = p.ap;
  out[4] = p.dcg;
  out[5] = p.idcg;
  out[6] = p.rr;
}

__device__ __forceinline__ uint64_t slot_hash(int64_t v) {
  uint64_t x = (uint64_t)v * 0x9e3779b97f4a7c15ull;
  return x ^ (x >> 29);
}

// true if v was not in the set before (the set never fills: cap >= 2 * inserts)
__device__ __forceinline__ bool insert(unsigned long long* tab, uint64_t cap, int64_t v) {
  uint64_t h = slot_hash(v) & (cap - 1);
  for (;;) {
    const unsigned long long prev = atomicCAS(&tab[h], kEmpty, (unsigned long long)v);
    if (prev == kEmpty) return true;
    if (prev == (unsigned long long)v) return false;
    h = (h + 1) & (cap - 1);
  }
}

// ------------------------------------------------------------------------------------------------ remove_itemid
__global__ void __launch_bounds__(kThreads)
rank_filter_kernel(const int64_t* __restrict__ rec, int64_t ld_rec, int64_t len, const int64_t* __restrict__ ex_off,
                   const int64_t* __restrict__ ex_ids, int64_t ex_nnz, int64_t* __restrict__ out, int64_t ld_out,
                   int64_t* __restrict__ out_len, int32_t* err) {
  __shared__ int s_wave[kWaves];
  const int64_t u = blockIdx.x;
  int64_t lo, hi;
  csr_row(ex_off, u, ex_nnz, err, lo, hi);
  const int64_t* row = rec + u * ld_rec;
  int64_t* dst = out + u * ld_out;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t kept = 0;   // identical in every thread
  for (int64_t base = 0; base < len; base += kThreads) {
    const int64_t j = base + threadIdx.x;
    int64_t v = 0;
    bool keep = false;
    if (j < len) {
      v = row[j];
      keep = !member(ex_ids, lo, hi, v);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? s_wave[w] : 0;
      total += s_wave[w];
    }
    if (keep) dst[kept + before + __popcll(m & ((1ull << lane) - 1ull))] = v;
    kept += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) out_len[u] = kept;
}

// ------------------------------------------------------------------------------------------------ lists
__global__ void __launch_bounds__(kThreads)
rank_lists_kernel(const int64_t* __restrict__ pred, int64_t ld_pred, const int64_t* __restrict__ pred_len,
                  int64_t rows, int64_t len, const int64_t* __restrict__ act_off, const int64_t* __restrict__ act_ids,
                  int64_t act_nnz, const int64_t* __restrict__ act_len, int64_t k, unsigned long long* table,
                  int64_t cap, double* __restrict__ partials, int32_t* err) {
  __shared__ unsigned long long s_mask[kWaves];
  __shared__ long long s_red[kWaves];
  unsigned long long* tab = table + (int64_t)blockIdx.x * cap;
  for (int64_t u = blockIdx.x; u < rows; u += gridDim.x) {
    int64_t lo, hi;
    csr_row(act_off, u, act_nnz, err, lo, hi);
    int64_t plen = pred_len ? pred_len[u] : len;
    if (plen < 0 || plen > len) {
      if (threadIdx.x == 0) atomicOr(err, CTR_RANK_ERR_LENGTH);
      plen = 0;
    }
    const int64_t kk = k < plen ? k : plen;
    const int64_t* p = pred + u * ld_pred;
    for (int64_t i = threadIdx.x; i < cap; i += kThreads) tab[i] = kEmpty;
    __syncthreads();   // the clearing stores are complete (vmcnt) before any wave's CAS reaches L2
    long long rec = 0, same = 0;
    for (int64_t i = threadIdx.x; i < kk; i += kThreads) {
      const int64_t v = p[i];
      if (insert(tab, (uint64_t)cap, v)) {
        ++rec;
        same += member(act_ids, lo, hi, v) ? 1 : 0;
      }
    }
    const long long real = block_sum(distinct_local(act_ids, lo, hi), s_red);
    rec = block_sum(rec, s_red);
    same = block_sum(same, s_red);
    Walk w;
    walk(plen, kk, [&](int64_t j) { return member(act_ids, lo, hi, p[j]); }, s_mask, w);
    if (threadIdx.x == 0) {
      const int64_t ones = w.hits < kk ? w.hits : kk;
      Partials r;
      r.same = (double)same;
      r.rec = (double)rec;
      r.real = (double)real;
      r.ap = w.score / (double)act_len[u];
      r.dcg = w.dcg;
      r.idcg = ideal_dcg(ones);
      r.rr = w.first >= 0 ? 1.0 / (double)(w.first + 1) : 0.0;
      store(partials + u * 7, r);
    }
    __syncthreads();   // the table is cleared for the next user only after every insert of this one
  }
}

// ------------------------------------------------------------------------------------------------ scores
__global__ void __launch_bounds__(kThreads)
rank_mask_kernel(float* __restrict__ scores, int64_t ld, int64_t n, const int64_t* __restrict__ ex_off,
                 const int64_t* __restrict__ ex_ids, int64_t ex_nnz, int32_t* err) {
  const int64_t u = blockIdx.x;
  int64_t lo, hi;
  csr_row(ex_off, u, ex_nnz, err, lo, hi);
  float* row = scores + u * ld;
  for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
    const int64_t id = ex_ids[j];
    if (id >= 0 && id < n) row[id] = __uint_as_float(CTR_RANK_MASK_BITS);
  }
}

__global__ void __launch_bounds__(kThreads)
rank_scores_kernel(const float* __restrict__ scores, int64_t ld, int64_t n, const int64_t* __restrict__ topk,
                   int64_t kt, int64_t k, const int64_t* __restrict__ act_off, const int64_t* __restrict__ act_ids,
                   int64_t act_nnz, const int64_t* __restrict__ act_len, const int64_t* __restrict__ n_real,
                   const int64_t* __restrict__ pad, double* __restrict__ partials, int32_t* err) {
  __shared__ unsigned long long s_mask[kWaves];
  __shared__ long long s_red[kWaves];
  __shared__ unsigned long long s_best;
  const int64_t u = blockIdx.x;
  const float* row = scores + u * ld;
  const int64_t* top = topk + u * kt;
  int64_t lo, hi;
  csr_row(act_off, u, act_nnz, err, lo, hi);
  int64_t nr = n_real[u], pd = pad[u];
  if (nr < 0 || nr > n || pd < 0) {
    if (threadIdx.x == 0) atomicOr(err, CTR_RANK_ERR_LENGTH);
    nr = pd = 0;
  }
  if (threadIdx.x == 0) s_best = 0ull;
  __syncthreads();
  const int64_t plen = nr + pd;                 // the filtered row: nr survivors in ranking order, then pd times -1
  const int64_t kk = k < plen ? k : plen;
  const int64_t ks = kk < nr ? kk : nr;         // survivors inside p[:k] (<= kt)
  const bool minus1 = member(act_ids, lo, hi, -1);
  // distinct ids of a; those that are survivors of this row, and the best of them in topk.hip's order
  long long real = 0, rel = 0;
  for (int64_t j = lo + threadIdx.x; j < hi; j += kThreads) {
    const int64_t x = act_ids[j];
    if (j != lo && act_ids[j - 1] == x) continue;
    ++real;
    if (x >= 0 && x < n) {
      const float s = row[x];
      if (__float_as_uint(s) != CTR_RANK_MASK_BITS) {
        ++rel;
        atomicMax(&s_best, entry(ordered_key(s), (uint32_t)x));
      }
    }
  }
  real = block_sum(real, s_red);
  rel = block_sum(rel, s_red);          // its barriers also publish s_best
  const unsigned long long best = s_best;
  // p[:k] in order: survivors from the top-k, then pads
  Walk w;
  walk(kk, kk, [&](int64_t j) { return j < nr ? member(act_ids, lo, hi, top[j]) : minus1; }, s_mask, w);
  // one streaming pass over the row: survivors ranked above the best relevant one; survivor count and validity
  long long above = 0, alive = 0, bad = 0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const float s = row[i];
    const uint32_t b = __float_as_uint(s);
    if (b == CTR_RANK_MASK_BITS) continue;
    ++alive;
    bad += (s != s || s == -INFINITY) ? 1 : 0;
    above += entry(ordered_key(s), (uint32_t)i) > best ? 1 : 0;
  }
  above = block_sum(above, s_red);
  alive = block_sum(alive, s_red);
  bad = block_sum(bad, s_red);
  if (threadIdx.x == 0) {
    if (bad) atomicOr(err, CTR_RANK_ERR_SURVIVOR);
    if (alive != nr) atomicOr(err, CTR_RANK_ERR_COUNT);
    const int64_t sum_r = rel + (minus1 ? pd : 0);
    Partials r;
    r.same = (double)(w.hits_k - (kk > nr && minus1 ? (kk - nr) - 1 : 0));   // the pads count once in the set
    r.rec = (double)(ks + (kk > nr ? 1 : 0));
    r.real = (double)real;
    r.ap = w.score / (double)act_len[u];
    r.dcg = w.dcg;
    r.idcg = ideal_dcg(sum_r < kk ? sum_r : kk);
    r.rr = rel > 0 ? 1.0 / (double)(above + 1) : (minus1 && pd > 0 ? 1.0 / (double)(nr + 1) : 0.0);
    store(partials + u * 7, r);
  }
}

}  // namespace

extern "C" int ctr_rank_filter(const int64_t* rec, int64_t ld_rec, int64_t rows, int64_t len, const int64_t* ex_off,
                               const int64_t* ex_ids, int64_t ex_nnz, int64_t* out, int64_t ld_out, int64_t* out_len,
                               int32_t* err_flag, void* stream) {
  CTR_REQUIRE(rows >= 0 && len >= 0 && ex_nnz >= 0 && ld_rec >= len && ld_out >= len, CTR_EINVAL);
  if (rows == 0) return CTR_OK;
  CTR_REQUIRE(ex_off && out_len && err_flag && (ex_nnz == 0 || ex_ids) && (len == 0 || (rec && out)), CTR_EINVAL);
  CTR_REQUIRE(rows <= CTR_RANK_MAX_ROWS, CTR_ELIMIT);
  hipLaunchKernelGGL(rank_filter_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, rec, ld_rec, len,
                     ex_off, ex_ids, ex_nnz, out, ld_out, out_len, err_flag);
  return ctr_launch_status();
}

static int64_t table_slots_for(int64_t k, int64_t len) {
  const int64_t kk = k < len ? k : len;
  int64_t cap = 64;
  while (cap < 2 * kk) cap <<= 1;
  return cap;
}

extern "C" int ctr_rank_table_slots(int64_t k, int64_t len, int64_t* slots) {
  CTR_REQUIRE(k >= 1 && len >= 0 && slots, CTR_EINVAL);
  *slots = table_slots_for(k, len);
  return CTR_OK;
}

extern "C" int ctr_rank_metrics_lists(const int64_t* pred, int64_t ld_pred, const int64_t* pred_len, int64_t rows,
                                      int64_t len, const int64_t* act_off, const int64_t* act_ids, int64_t act_nnz,
                                      const int64_t* act_len, int64_t k, int64_t* table, int64_t table_slots,
                                      double* partials, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(k >= 1 && rows >= 0 && len >= 0 && act_nnz >= 0 && ld_pred >= len && table_slots >= 0, CTR_EINVAL);
  if (rows == 0) return CTR_OK;
  CTR_REQUIRE(act_off && act_len && partials && err_flag && table && (act_nnz == 0 || act_ids) && (len == 0 || pred),
              CTR_EINVAL);
  const int64_t cap = table_slots_for(k, len);
  CTR_REQUIRE(table_slots >= cap, CTR_EINVAL);
  int64_t grid = table_slots / cap;
  if (grid > rows) grid = rows;
  if (grid > kListsMaxGrid) grid = kListsMaxGrid;
  hipLaunchKernelGGL(rank_lists_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, pred, ld_pred,
                     pred_len, rows, len, act_off, act_ids, act_nnz, act_len, k, (unsigned long long*)table, cap,
                     partials, err_flag);
  return ctr_launch_status();
}

extern "C" int ctr_rank_mask(float* scores, int64_t ld, int64_t rows, int64_t n, const int64_t* ex_off,
                             const int64_t* ex_ids, int64_t ex_nnz, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(rows >= 0 && n >= 1 && ld >= n && ex_nnz >= 0, CTR_EINVAL);
  if (rows == 0) return CTR_OK;
  CTR_REQUIRE(scores && ex_off && err_flag && (ex_nnz == 0 || ex_ids), CTR_EINVAL);
  CTR_REQUIRE(rows <= CTR_RANK_MAX_ROWS && n < (1ll << 31), CTR_ELIMIT);
  hipLaunchKernelGGL(rank_mask_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, scores, ld, n,
                     ex_off, ex_ids, ex_nnz, err_flag);
  return ctr_launch_status();
}

extern "C" int ctr_rank_metrics_scores(const float* scores, int64_t ld, int64_t rows, int64_t n, const int64_t* topk,
                                       int64_t kt, int64_t k, const int64_t* act_off, const int64_t* act_ids,
                                       int64_t act_nnz, const int64_t* act_len, const int64_t* n_real,
                                       const int64_t* pad, double* partials, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(k >= 1 && rows >= 0 && n >= 1 && ld >= n && act_nnz >= 0 && kt == (k < n ? k : n), CTR_EINVAL);
  if (rows == 0) return CTR_OK;
  CTR_REQUIRE(scores && topk && act_off && act_len && n_real && pad && partials && err_flag && (act_nnz == 0 || act_ids),
              CTR_EINVAL);
  CTR_REQUIRE(rows <= CTR_RANK_MAX_ROWS && n < (1ll << 31), CTR_ELIMIT);
  hipLaunchKernelGGL(rank_scores_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, scores, ld, n,
                     topk, kt, k, act_off, act_ids, act_nnz, act_len, n_real, pad, partials, err_flag);
  return ctr_launch_status();
}
