// Mini-batch loader: every tensor of one batch of a shuffled epoch in one launch (ctr_load_batch), and the shuffled
// index on its own (ctr_loader_indices).  The reference trains full-batch (trainer/trainer.py:23-40: the same tensors
// every epoch) and leaves data/dataloader.py and data/dataset.py empty; this is the layer a sample set larger than one
// step needs.
//
// The shuffled index.  Position p (0 <= p < N) of epoch e under `seed` reads sample perm(seed, e, p):
//     bits  = the smallest even number >= 2 with 2^bits >= N;   half = bits / 2;   mask = 2^half - 1
//     key_r = mix64(seed ^ mix64(e * 0x100000001B3 + r)),  r = 0..3        (uint64, wrapping; mix64 as sampler.hip)
//     E(x):   (L, R) = (x >> half, x & mask);  for r = 0..3:  (L, R) = (R, L ^ ((mix64(key_r ^ R) >> 32) & mask));
//             E = (L << half) | R
//     x = E(p);  while (x >= N) x = E(x);  perm = x
// E is a balanced Feistel network, so a bijection of [0, 2^bits) whatever the round function is; following a
// position's cycle until it re-enters [0, N) ("cycle walking") restricts it to a bijection of [0, N), and the walk
// ends because p itself is below N.  2^bits < 4 N: fewer than 4 evaluations per element on average, for every N.
// No permutation array, no sort, no state: the index of a position depends on (seed, e, p, N) only, not on the launch
// geometry or on which batch asks for it.  tests/loader_numpy.py restates it.
//
// Integer and copy work only, bit-exact (the one conversion is the feature join's int -> float of the two id columns,
// as assemble_kernel).  A workgroup takes 64 positions at a time: one wave computes their sample indices (and reads the
// join ids) into LDS, then all four waves copy -- consecutive lanes take consecutive elements of a row, so a history
// row (L int64) or a feature row is read and written in whole cache lines, and rows of 16-byte multiples move as
// 16-byte pieces.
//
// Drawn negatives (ctr_load_batch_neg).  N positives, k = negatives >= 1; an epoch has M = N * (1 + k) positions and
// position p of epoch e holds
//     v = perm_M(seed, e, p)             the permutation above over M instead of N;  v = p when shuffle == 0
//     s = v / (1 + k);  j = v % (1 + k)
//     j == 0:  the positive s, every output exactly as ctr_load_batch writes sample s
//     j >= 1:  a negative of user u = users[s]:
//         nkey    = mix64(seed ^ mix64(e * 0x100000001B3 + 4))             (round index 4: the permutation uses 0..3)
//         draw_t  = ((mix64(nkey ^ mix64(v * 0x100000001B3 + t)) >> 32) * num_items) >> 32,    t = 0, 1, ...
//         item    = draw_t for the first t < 2^14 with (u, draw_t) not observed
//         outputs = those of sample s, with the item id replaced by `item` and the rating by 0.0f (the replaced id is
//                   what the feature join reads; the history row stays user u's)
// uint64 arithmetic, wrapping.  Slots draw independently, so one positive's negatives may repeat.  Unshuffled, every
// positive is followed by its k negatives.  If all 2^14 draws are observed the last one is written and *fail_flag is
// raised; a user id outside [0, num_users) makes no draw, writes item 0 and raises *err_flag.  The observed set is a
// CSR over users (indptr int64, item ids int32 ascending and distinct within a row), membership a binary search: 4 B
// per observed pair whatever num_items is, where the sampler's bitmap is num_users * num_items / 8 B.
// tests/loader_neg_numpy.py restates this.
//
// Grouped epochs (ctr_load_batch_groups).  The shuffle above scatters a positive and its negatives over the epoch; a
// loss over the group (group_loss.hip) needs them side by side.  With N positives and k = negatives, position p of
// epoch e holds
//     g = p / (1 + k);  j = p % (1 + k)
//     s = perm_N(seed, e, g)             the permutation over N, not over M;  s = g when shuffle == 0
//     v = s * (1 + k) + j
//     outputs = exactly what ctr_load_batch_neg defines for virtual index v
//               (j == 0: positive s;  j >= 1: the draw keyed by (seed, e, v))
// Every batch whose first position and count are multiples of 1 + k is a run of whole groups, positive first.
// Unshuffled the output equals ctr_load_batch_neg's bit for bit; shuffled, the epoch emits the same multiset of
// samples as ctr_load_batch_neg does for the same (seed, e), because the draws depend on (seed, e, v) only and
// (g, j) -> v is a bijection of [0, M); the order of groups is a bijection of [0, N).  A 64-position tile usually
// cuts a group (1 + k seldom divides 64), so every position derives its own g and j.
// tests/loader_group_numpy.py restates this.
//
// Weighted negatives (ctr_load_batch_neg_pop, ctr_load_batch_groups_pop).  The uniform draw makes almost every negative
// of a long-tailed catalogue an item nobody interacts with; these two arms draw from a distribution q over the items,
// given as an alias table of num_items 64-bit words built on the host (data/sampler.py):
//     table[c] = (thresh_c << 32) | alias_c        thresh_c a uint32, alias_c an item id; a column that always keeps
//                                                  itself has alias_c == c (2^32 does not fit the threshold)
// Everything above stands, with draw_t replaced by item_t: the same hash stream picks a column with its high half and
// keeps it or takes its alias with its low half,
//     h      = mix64(nkey ^ mix64(v * 0x100000001B3 + t))                       nkey as above (round index 4)
//     col    = ((h >> 32) * num_items) >> 32
//     word   = table[col]
//     item_t = (h & 0xffffffff) < (word >> 32) ? col : (int32)word              (alias_col == col: col either way)
//     item   = item_t for the first t < 2^14 with (u, item_t) not observed
// and the last try with *fail_flag when all are observed, item 0 with *err_flag for a bad user id, as above.  The table
// draws item i with probability
//     q_i = (kept_i + sum over c != i with alias_c == i of (2^32 - thresh_c)) / (num_items * 2^32),
//     kept_i = 2^32 if alias_i == i, else thresh_i
// (up to the 2^-32 granularity of the two halves), so user u's negatives follow q_i / (1 - Q_u) over the items u has
// not observed, Q_u the q-mass of the observed ones; an item with q_i == 0 is never drawn, and a user whose unobserved
// items all have q == 0 fails like one who has observed everything.  Grouped or not as above: the draw depends on
// (seed, e, v) only, so the two epochs of one (seed, e) still emit the same multiset.
// The log-q column.  A sampled softmax over such negatives subtracts log q(item) from every logit (group_loss.hip).
// When logq_out is set, position b of the batch also writes
//     logq_out[b * logq_ldo] = log_q[item]        item = pos_items[s] for a positive, the drawn item for a negative
//                                                 (item 0 for a bad user id)
// a bitwise copy of the float; an item outside [0, num_items) -- a positive's, or an alias of a corrupt table -- raises
// *err_flag and writes 0.0f.  The features family has no item column in its batch, which is why the loader writes it.
// The table is 8 B per item (214 KB at 26 744 items: L2-resident); a try is one more dependent load in front of the
// binary search.  The uniform arms are compiled without any of this: kernels of their own, as for the grouped arm.
// tests/loader_pop_numpy.py restates this.
//
// The draw is a chain of dependent loads per position: users[s] -> indptr[u], indptr[u + 1] -> about log2(row length)
// probes per try.  Spreading a tile's 64 chains over the four waves would not shorten any of them, and a batch of
// 65536 positions is 1024 workgroups of 2 KiB LDS and few registers, all resident at once (4 per CU), so every chain of
// the batch is in flight from the start either way: the draw stays in the index stage's one wave, and the other
// workgroups on the CU cover its latency.  The output does not depend on that choice.
#include "ctr_common.h"
#include "loader_perm.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 64;  // positions per workgroup pass

typedef uint32_t ctr_u32x4 __attribute__((ext_vector_type(4)));

// row rows[s] of src -> row base + s of dst, s < cnt, w units of type T per row
template <typename T>
__device__ __forceinline__ void copy_rows(const void* src, int64_t lds, void* dst, int64_t ldd, int w, int cnt,
                                          const int64_t* rows, int64_t base) {
  const CTR_GLOBAL T* s = (const CTR_GLOBAL T*)src;
  CTR_GLOBAL T* d = (CTR_GLOBAL T*)dst;
  if (w == 1) {
    for (int r = threadIdx.x; r < cnt; r += kBlock) d[(base + r) * ldd] = s[rows[r] * lds];
    return;
  }
  const int total = cnt * w;
  for (int g = threadIdx.x; g < total; g += kBlock) {
    const int r = g / w;
    const int j = g - r * w;
    d[(base + r) * ldd + j] = s[rows[r] * lds + j];
  }
}

// the feature join and the history join of one tile, from the ids the index stage left in LDS
__device__ __forceinline__ void write_joins(const ctr_loader_t& d, int cnt, int64_t base, int hist16, const int64_t* s_fu,
                                            const int64_t* s_fi, const int64_t* s_hu) {
  if (d.feat_out) {
    const int uw = d.user_width, width = 2 + d.user_width + d.item_width;
    const int total = cnt * width;
    for (int g = threadIdx.x; g < total; g += kBlock) {
      const int r = g / width;
      const int c = g - r * width;
      const int64_t u = s_fu[r], i = s_fi[r];
      float v;
      if (c == 0) v = (float)u;
      else if (c == 1) v = (float)i;
      else if (c < 2 + uw) v = ctr_ldg(d.user_feat + (u < 0 || u >= d.num_users ? 0 : u) * uw + (c - 2));
      else v = ctr_ldg(d.item_feat + (i < 0 || i >= d.num_items ? 0 : i) * d.item_width + (c - 2 - uw));
      ctr_stg(d.feat_out + (base + r) * d.feat_ldo + c, v);
    }
  }
  if (d.hist_out) {
    if (hist16)
      copy_rows<ctr_u32x4>(d.history, d.ld_history / 2, d.hist_out, d.hist_ldo / 2, (int)(d.hist_len / 2), cnt, s_hu, base);
    else
      copy_rows<uint64_t>(d.history, d.ld_history, d.hist_out, d.hist_ldo, (int)d.hist_len, cnt, s_hu, base);
  }
}

__global__ void __launch_bounds__(kBlock)
load_batch_kernel(const ctr_loader_t d, const LoaderPerm pm, int64_t first, int64_t count, int hist16) {
  __shared__ int64_t s_idx[kTile], s_fu[kTile], s_fi[kTile], s_hu[kTile];
  const int64_t tiles = (count + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile;
    const int cnt = (int)(count - base < kTile ? count - base : kTile);
    if ((int)threadIdx.x < cnt) {
      const int64_t idx = loader_index(pm, first + base + threadIdx.x);
      s_idx[threadIdx.x] = idx;
      bool bad = false;
      if (d.feat_out) {
        const int64_t u = ctr_ldg(d.feat_users + idx), i = ctr_ldg(d.feat_items + idx);
        bad = u < 0 || u >= d.num_users || i < 0 || i >= d.num_items;
        s_fu[threadIdx.x] = u;
        s_fi[threadIdx.x] = i;
      }
      if (d.hist_out) {
        int64_t u = ctr_ldg(d.hist_users + idx);
        if (u < 0 || u >= d.hist_rows) {
          bad = true;
          u = 0;
        }
        s_hu[threadIdx.x] = u;
      }
      if (bad && d.err_flag) *(CTR_GLOBAL int32_t*)d.err_flag = 1;
    }
    __syncthreads();
    for (int c = 0; c < d.ncols; ++c) {
      const ctr_loader_col_t& col = d.cols[c];
      if (col.elem_bytes == 8) copy_rows<uint64_t>(col.src, col.lds, col.dst, col.ldd, col.width, cnt, s_idx, base);
      else copy_rows<uint32_t>(col.src, col.lds, col.dst, col.ldd, col.width, cnt, s_idx, base);
    }
    write_joins(d, cnt, base, hist16, s_fu, s_fi, s_hu);
    __syncthreads();  // the next pass rewrites the LDS rows
  }
}

constexpr int kMaxTries = 1 << 14;

struct LoaderDraw {
  uint64_t nkey;
  uint64_t per;  // 1 + negatives
  const int64_t* users;
  const int64_t* indptr;
  const int32_t* indices;
  int64_t num_users;
  uint64_t num_items;
  int32_t* fail_flag;
  int32_t item_col, rating_col;
};

// what the weighted arm adds to LoaderDraw (header comment: weighted negatives); the uniform kernels never see it
struct LoaderPop {
  const uint64_t* table;     // num_items words (thresh << 32) | alias
  const int64_t* pos_items;  // item id of each positive
  const float* log_q;        // num_items
  float* logq_out;           // nullable
  int64_t logq_ldo;
};

// the item of negative slot v of user u (header comment); u inside [0, num_users).  kWeighted: the uniform draw picks
// a column of `table`, the low half of the same hash keeps it or takes its alias.
template <bool kWeighted>
__device__ __forceinline__ int64_t draw_negative(const LoaderDraw& nd, const uint64_t* table, uint64_t v, int64_t u) {
  const int64_t lo = ctr_ldg(nd.indptr + u), hi = ctr_ldg(nd.indptr + u + 1);
  const CTR_GLOBAL int32_t* ind = (const CTR_GLOBAL int32_t*)nd.indices;
  const uint64_t slot = v * 0x100000001B3ull;
  uint64_t item = 0;
  for (int t = 0; t < kMaxTries; ++t) {
    const uint64_t h = mix64(nd.nkey ^ mix64(slot + (uint64_t)t));
    item = ((h >> 32) * nd.num_items) >> 32;
    if constexpr (kWeighted) {
      const uint64_t word = ((const CTR_GLOBAL uint64_t*)table)[item];
      if ((uint32_t)h >= (uint32_t)(word >> 32)) item = (uint32_t)word;
    }
    int64_t a = lo, b = hi;
    while (a < b) {  // first entry of the row that is >= item
      const int64_t mid = a + ((b - a) >> 1);
      if (ind[mid] < (int32_t)item) a = mid + 1;
      else b = mid;
    }
    if (a == hi || ind[a] != (int32_t)item) return (int64_t)item;
  }
  if (nd.fail_flag) *(CTR_GLOBAL int32_t*)nd.fail_flag = 1;
  return (int64_t)item;
}

// ctr_load_batch_neg / ctr_load_batch_groups: load_batch_kernel over the virtual epoch.  The index stage also decides
// positive or negative and draws; s_neg holds the drawn item, -1 for a positive.  kGrouped: pm permutes the N groups
// and the position keeps its slot (header comment); otherwise pm permutes the M positions.  One body, a kernel per
// arm, so that the plain loader and the ungrouped arm keep their registers.  kWeighted: the draw goes through the alias
// table and the index stage also writes the log-q column; pop is null in the uniform arms and never read there.
template <bool kGrouped, bool kWeighted>
__device__ __forceinline__ void load_neg_tiles(const ctr_loader_t& d, const LoaderPerm& pm, const LoaderDraw& nd,
                                               const LoaderPop* pop, int64_t first, int64_t count, int hist16) {
  __shared__ int64_t s_idx[kTile], s_fu[kTile], s_fi[kTile], s_hu[kTile], s_neg[kTile];
  const int64_t tiles = (count + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile;
    const int cnt = (int)(count - base < kTile ? count - base : kTile);
    if ((int)threadIdx.x < cnt) {
      uint64_t v;
      int64_t idx;
      if constexpr (kGrouped) {
        const uint64_t p = (uint64_t)(first + base + threadIdx.x);
        const uint64_t g = p / nd.per;
        idx = loader_index(pm, (int64_t)g);
        v = (uint64_t)idx * nd.per + (p - g * nd.per);
      } else {
        v = (uint64_t)loader_index(pm, first + base + threadIdx.x);
        idx = (int64_t)(v / nd.per);
      }
      s_idx[threadIdx.x] = idx;
      bool bad = false;
      int64_t item = -1;
      if (v - (uint64_t)idx * nd.per != 0) {
        const int64_t u = ctr_ldg(nd.users + idx);
        if (u < 0 || u >= nd.num_users) {
          bad = true;
          item = 0;
        } else {
          if constexpr (kWeighted) item = draw_negative<true>(nd, pop->table, v, u);
          else item = draw_negative<false>(nd, nullptr, v, u);
        }
      }
      s_neg[threadIdx.x] = item;
      if constexpr (kWeighted) {
        const int64_t at = item >= 0 ? item : ctr_ldg(pop->pos_items + idx);
        const bool inside = at >= 0 && (uint64_t)at < nd.num_items;
        bad = bad || !inside;
        if (pop->logq_out)   // a copy, bitwise; 0.0f for an id outside the table
          ctr_stg(pop->logq_out + (base + threadIdx.x) * pop->logq_ldo, inside ? ctr_ldg(pop->log_q + at) : 0.0f);
      }
      if (d.feat_out) {
        const int64_t u = ctr_ldg(d.feat_users + idx), i = item >= 0 ? item : ctr_ldg(d.feat_items + idx);
        bad = bad || u < 0 || u >= d.num_users || i < 0 || i >= d.num_items;
        s_fu[threadIdx.x] = u;
        s_fi[threadIdx.x] = i;
      }
      if (d.hist_out) {
        int64_t u = ctr_ldg(d.hist_users + idx);
        if (u < 0 || u >= d.hist_rows) {
          bad = true;
          u = 0;
        }
        s_hu[threadIdx.x] = u;
      }
      if (bad && d.err_flag) *(CTR_GLOBAL int32_t*)d.err_flag = 1;
    }
    __syncthreads();
    for (int c = 0; c < d.ncols; ++c) {
      const ctr_loader_col_t& col = d.cols[c];
      if (c == nd.item_col) {  // int64, width 1 (checked by the entry point)
        const CTR_GLOBAL int64_t* s = (const CTR_GLOBAL int64_t*)col.src;
        CTR_GLOBAL int64_t* o = (CTR_GLOBAL int64_t*)col.dst;
        for (int r = threadIdx.x; r < cnt; r += kBlock) o[(base + r) * col.ldd] = s_neg[r] >= 0 ? s_neg[r] : s[s_idx[r] * col.lds];
      } else if (c == nd.rating_col) {  // float32, width 1
        const CTR_GLOBAL float* s = (const CTR_GLOBAL float*)col.src;
        CTR_GLOBAL float* o = (CTR_GLOBAL float*)col.dst;
        for (int r = threadIdx.x; r < cnt; r += kBlock) o[(base + r) * col.ldd] = s_neg[r] >= 0 ? 0.0f : s[s_idx[r] * col.lds];
      } else if (col.elem_bytes == 8) {
        copy_rows<uint64_t>(col.src, col.lds, col.dst, col.ldd, col.width, cnt, s_idx, base);
      } else {
        copy_rows<uint32_t>(col.src, col.lds, col.dst, col.ldd, col.width, cnt, s_idx, base);
      }
    }
    write_joins(d, cnt, base, hist16, s_fu, s_fi, s_hu);
    __syncthreads();  // the next pass rewrites the LDS rows
  }
}

__global__ void __launch_bounds__(kBlock)
load_batch_neg_kernel(const ctr_loader_t d, const LoaderPerm pm, const LoaderDraw nd, int64_t first, int64_t count,
                      int hist16) {
  load_neg_tiles<false, false>(d, pm, nd, nullptr, first, count, hist16);
}

__global__ void __launch_bounds__(kBlock)
load_batch_groups_kernel(const ctr_loader_t d, const LoaderPerm pm, const LoaderDraw nd, int64_t first, int64_t count,
                         int hist16) {
  load_neg_tiles<true, false>(d, pm, nd, nullptr, first, count, hist16);
}

__global__ void __launch_bounds__(kBlock)
load_batch_neg_pop_kernel(const ctr_loader_t d, const LoaderPerm pm, const LoaderDraw nd, const LoaderPop pop,
                          int64_t first, int64_t count, int hist16) {
  load_neg_tiles<false, true>(d, pm, nd, &pop, first, count, hist16);
}

__global__ void __launch_bounds__(kBlock)
load_batch_groups_pop_kernel(const ctr_loader_t d, const LoaderPerm pm, const LoaderDraw nd, const LoaderPop pop,
                             int64_t first, int64_t count, int hist16) {
  load_neg_tiles<true, true>(d, pm, nd, &pop, first, count, hist16);
}

__global__ void __launch_bounds__(kBlock)
loader_indices_kernel(const LoaderPerm pm, int64_t first, int64_t count, int64_t* __restrict__ out) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x)
    out[t] = loader_index(pm, first + t);
}

constexpr int64_t kMaxRowUnits = 1 << 20;  // cnt * width stays far inside int

bool aligned_to(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

int check_range(int64_t n, int64_t epoch, int64_t first, int64_t count) {
  CTR_REQUIRE(n >= 1 && n <= (1ll << 62) && epoch >= 0 && first >= 0 && first <= n && count <= n - first, CTR_EINVAL);
  return CTR_OK;
}

// the descriptor's own checks, shared by both entry points; *hist16: history rows move as 16-byte pieces
int check_loader(const ctr_loader_t& d, int* hist16) {
  CTR_REQUIRE(d.ncols >= 0 && d.ncols <= CTR_MAX_FIELDS, CTR_EINVAL);
  for (int c = 0; c < d.ncols; ++c) {
    const ctr_loader_col_t& col = d.cols[c];
    CTR_REQUIRE(col.src && col.dst && col.width >= 1 && col.lds >= col.width && col.ldd >= col.width &&
                    (col.elem_bytes == 4 || col.elem_bytes == 8),
                CTR_EINVAL);
    CTR_REQUIRE(col.width <= kMaxRowUnits, CTR_ELIMIT);
    CTR_REQUIRE(aligned_to(col.src, col.elem_bytes) && aligned_to(col.dst, col.elem_bytes), CTR_EALIGN);
  }
  if (d.feat_out) {
    CTR_REQUIRE(d.feat_users && d.feat_items && d.user_feat && d.item_feat && d.user_width >= 0 && d.item_width >= 0 &&
                    d.num_users > 0 && d.num_items > 0 && d.feat_ldo >= 2 + (int64_t)d.user_width + d.item_width,
                CTR_EINVAL);
    CTR_REQUIRE(2 + (int64_t)d.user_width + d.item_width <= kMaxRowUnits, CTR_ELIMIT);
  }
  *hist16 = 0;
  if (d.hist_out) {
    CTR_REQUIRE(d.hist_users && d.history && d.hist_rows > 0 && d.hist_len >= 1 && d.ld_history >= d.hist_len &&
                    d.hist_ldo >= d.hist_len,
                CTR_EINVAL);
    CTR_REQUIRE(d.hist_len <= kMaxRowUnits, CTR_ELIMIT);
    CTR_REQUIRE(aligned_to(d.history, 8) && aligned_to(d.hist_out, 8), CTR_EALIGN);
    *hist16 = d.hist_len % 2 == 0 && d.ld_history % 2 == 0 && d.hist_ldo % 2 == 0 && ctr_aligned16(d.history) &&
              ctr_aligned16(d.hist_out);
  }
  return CTR_OK;
}

}  // namespace

extern "C" int ctr_load_batch(const ctr_loader_t* loader, uint64_t seed, int64_t epoch, int64_t first, int64_t count,
                              int shuffle, void* stream) {
  CTR_REQUIRE(count >= 0, CTR_EINVAL);
  if (count == 0) return CTR_OK;
  CTR_REQUIRE(loader, CTR_EINVAL);
  const ctr_loader_t& d = *loader;
  if (int rc = check_range(d.n, epoch, first, count)) return rc;
  int hist16 = 0;
  if (int rc = check_loader(d, &hist16)) return rc;
  const int grid = ctr_stream_grid(count, kTile);
  hipLaunchKernelGGL(load_batch_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, d,
                     make_perm(d.n, seed, epoch, shuffle != 0), first, count, hist16);
  return ctr_launch_status();
}

namespace {

// every arm over the virtual epoch: the checks, the draw descriptor and the launch; weighted: `pop` is required
int launch_neg(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, const ctr_loader_pop_t* pop, bool weighted,
               uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle, bool grouped, hipStream_t st) {
  CTR_REQUIRE(count >= 0, CTR_EINVAL);
  if (count == 0) return CTR_OK;
  CTR_REQUIRE(loader && neg && (pop || !weighted), CTR_EINVAL);
  const ctr_loader_t& d = *loader;
  const ctr_loader_neg_t& g = *neg;
  CTR_REQUIRE(g.negatives >= 1 && d.n >= 1 && d.n <= (1ll << 62) / (1 + (int64_t)g.negatives), CTR_EINVAL);
  const int64_t m = d.n * (1 + (int64_t)g.negatives);
  if (int rc = check_range(m, epoch, first, count)) return rc;
  int hist16 = 0;
  if (int rc = check_loader(d, &hist16)) return rc;
  CTR_REQUIRE(g.users && g.indptr && g.indices && g.num_users >= 1 && g.num_items >= 1 && g.num_items < (1ll << 31),
              CTR_EINVAL);
  CTR_REQUIRE(g.rating_col >= 0 && g.rating_col < d.ncols && g.item_col >= -1 && g.item_col < d.ncols &&
                  g.item_col != g.rating_col,
              CTR_EINVAL);
  CTR_REQUIRE(d.cols[g.rating_col].width == 1 && d.cols[g.rating_col].elem_bytes == 4, CTR_EINVAL);
  CTR_REQUIRE(g.item_col < 0 || (d.cols[g.item_col].width == 1 && d.cols[g.item_col].elem_bytes == 8), CTR_EINVAL);
  LoaderDraw nd;
  nd.nkey = mix64(seed ^ mix64((uint64_t)epoch * 0x100000001B3ull + 4));
  nd.per = 1 + (uint64_t)g.negatives;
  nd.users = g.users;
  nd.indptr = g.indptr;
  nd.indices = g.indices;
  nd.num_users = g.num_users;
  nd.num_items = (uint64_t)g.num_items;
  nd.fail_flag = g.fail_flag;
  nd.item_col = g.item_col;
  nd.rating_col = g.rating_col;
  const int grid = ctr_stream_grid(count, kTile);
  const LoaderPerm pm = make_perm(grouped ? d.n : m, seed, epoch, shuffle != 0);
  if (weighted) {
    const ctr_loader_pop_t& w = *pop;
    CTR_REQUIRE(w.table && w.pos_items && w.log_q && (!w.logq_out || w.logq_ldo >= 1), CTR_EINVAL);
    CTR_REQUIRE(aligned_to(w.table, 8) && aligned_to(w.pos_items, 8) && aligned_to(w.log_q, 4) &&
                    aligned_to(w.logq_out, 4),
                CTR_EALIGN);
    LoaderPop lp;
    lp.table = w.table;
    lp.pos_items = w.pos_items;
    lp.log_q = w.log_q;
    lp.logq_out = w.logq_out;
    lp.logq_ldo = w.logq_ldo;
    if (grouped)
      hipLaunchKernelGGL(load_batch_groups_pop_kernel, dim3(grid), dim3(kBlock), 0, st, d, pm, nd, lp, first, count, hist16);
    else
      hipLaunchKernelGGL(load_batch_neg_pop_kernel, dim3(grid), dim3(kBlock), 0, st, d, pm, nd, lp, first, count, hist16);
  } else if (grouped) {
    hipLaunchKernelGGL(load_batch_groups_kernel, dim3(grid), dim3(kBlock), 0, st, d, pm, nd, first, count, hist16);
  } else {
    hipLaunchKernelGGL(load_batch_neg_kernel, dim3(grid), dim3(kBlock), 0, st, d, pm, nd, first, count, hist16);
  }
  return ctr_launch_status();
}

}  // namespace

extern "C" int ctr_load_batch_neg_pop(const ctr_loader_t* loader, const ctr_loader_neg_t* neg,
                                      const ctr_loader_pop_t* pop, uint64_t seed, int64_t epoch, int64_t first,
                                      int64_t count, int shuffle, void* stream) {
  return launch_neg(loader, neg, pop, true, seed, epoch, first, count, shuffle, false, (hipStream_t)stream);
}

extern "C" int ctr_load_batch_groups_pop(const ctr_loader_t* loader, const ctr_loader_neg_t* neg,
                                         const ctr_loader_pop_t* pop, uint64_t seed, int64_t epoch, int64_t first,
                                         int64_t count, int shuffle, void* stream) {
  return launch_neg(loader, neg, pop, true, seed, epoch, first, count, shuffle, true, (hipStream_t)stream);
}

extern "C" int ctr_load_batch_neg(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, uint64_t seed, int64_t epoch,
                                  int64_t first, int64_t count, int shuffle, void* stream) {
  return launch_neg(loader, neg, nullptr, false, seed, epoch, first, count, shuffle, false, (hipStream_t)stream);
}

extern "C" int ctr_load_batch_groups(const ctr_loader_t* loader, const ctr_loader_neg_t* neg, uint64_t seed,
                                     int64_t epoch, int64_t first, int64_t count, int shuffle, void* stream) {
  return launch_neg(loader, neg, nullptr, false, seed, epoch, first, count, shuffle, true, (hipStream_t)stream);
}

extern "C" int ctr_loader_indices(int64_t n, uint64_t seed, int64_t epoch, int64_t first, int64_t count, int shuffle,
                                  int64_t* out, void* stream) {
  CTR_REQUIRE(count >= 0, CTR_EINVAL);
  if (count == 0) return CTR_OK;
  if (int rc = check_range(n, epoch, first, count)) return rc;
  CTR_REQUIRE(out, CTR_EINVAL);
  const int grid = ctr_stream_grid(count, kBlock);
  hipLaunchKernelGGL(loader_indices_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                     make_perm(n, seed, epoch, shuffle != 0), first, count, out);
  return ctr_launch_status();
}
