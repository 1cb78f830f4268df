// Graph propagation: a sparse-times-dense row sum over a CSR (LightGCN, He et al. 2020).  For every requested row r
//     out[j, :] = s_out[r] * sum_{e in [indptr[r], indptr[r+1])} s_in[indices[e]] * x[indices[e], :]       r = rows[j]
// The normalised adjacency is symmetric, so the backward of a propagation is this kernel over the transposed CSR: no
// activation is saved and there is no float atomic in this file.
//
//   graph_prop_kernel : ONE wave per work item, four items a workgroup, no LDS.
//     A row of x is k / 4 lanes wide in 16-byte loads, so one wave-instruction covers kEpi = 64 / (k / 4) list
//     entries (16 at k = 16, 5 at k = 48 with four idle lanes, 4 at k = 64, 1 at k = 256) and the loop keeps kUnroll
//     such instructions in flight: 16 rows per wave at k = 64.  Lane group g adds the entries g, g + kEpi, ... of its
//     segment in ascending order, one fused multiply-add each (s_in is read per entry; without s_in the factor is 1 and
//     the fma is a plain add); a lane without an entry adds nothing -- never a loaded value times zero.  The groups
//     meet in a fixed shuffle tree (g += g + 4, g += g + 2, g += g + 1 for five groups) when the segment ends.
//     A list is cut at FIXED positions, every CTR_GRAPH_SEGMENT entries from its own start, never by the launch
//     geometry.  A work item is either a whole row (the wave walks the segments in ascending order, adds their sums in
//     that order, scales and stores) or one segment of a long row (the sum goes to a slot of the workspace).
//   graph_merge_kernel: for every split row, the partials in ascending segment order, then the scale: the same chain
//     of additions as the whole-row walk, so a row's bits do not depend on whether it was split.
//
// Which rows are split and in what order the items run is the caller's plan (ops.graph_plan: rows by descending list
// length, segments of long rows as items of their own); without a plan every row is a whole-row item.  Either way a
// row is a bitwise function of its list, the source rows it names and the two scales.
//
// Guards, none of which traps: an index outside [0, x_rows) is never dereferenced, adds nothing and sets bit 1 of
// *err_flag; a row id outside the CSR or offsets that run backwards or past nnz give a zero row and bit 1; a work item
// that names an out row, a slot or a run of slots outside what the call was given is skipped and sets bit 2.  The flag
// is OR-ed with an integer atomic on the error path alone; it carries no result.
#include "ctr_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / CTR_WAVE;
constexpr int kSegment = CTR_GRAPH_SEGMENT;
constexpr int kUnroll = 4;      // wave-instructions of row loads in flight
constexpr int kErrIndex = 1, kErrPlan = 2;

struct Args {
  const float* x; int64_t x_rows, ldx;
  const int64_t* indptr; const int32_t* indices; int64_t num_rows, nnz;
  const float* s_in; const float* s_out;
  const int64_t* rows; int64_t count;
  float* out; int64_t ldo;
  float* ws; int64_t ws_slots;
  int32_t* err;
};

__device__ __forceinline__ void raise(const Args& a, int bit) {
  if (a.err) atomicOr(a.err, bit);
}

// [begin, end) of CSR row rows[j], checked; false: not a row of this CSR (then begin = end = 0)
__device__ __forceinline__ bool row_range(const Args& a, int64_t j, int64_t& r, int64_t& begin, int64_t& end) {
  r = a.rows ? a.rows[j] : j;
  begin = end = 0;
  if (r < 0 || r >= a.num_rows) return false;
  const int64_t b = a.indptr[r], e = a.indptr[r + 1];
  if (b < 0 || b > e || e > a.nnz) return false;
  begin = b;
  end = e;
  return true;
}

constexpr int pow2_at_least(int n) { return n <= 1 ? 1 : 2 * pow2_at_least((n + 1) / 2); }

// sum_{e in [begin, end)} s_in[idx_e] x[idx_e, 4 c .. 4 c + 3], complete in the lanes of group 0
template <int KB>
__device__ __forceinline__ ctr_f32x4 segment_sum(const Args& a, int64_t begin, int64_t end, int lane, bool& bad) {
  constexpr int kLpr = 4 * KB;              // lanes per row
  constexpr int kEpi = CTR_WAVE / kLpr;     // entries per wave-instruction
  const int g = lane / kLpr, c = lane - g * kLpr;
  const bool active = g < kEpi;
  ctr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t base = begin; base < end; base += kEpi * kUnroll) {
    ctr_f32x4 v[kUnroll];
    float s[kUnroll];
    bool ok[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int64_t e = base + u * kEpi + g;
      const bool valid = active && e < end;
      int64_t idx = -1;
      if (valid) idx = a.indices[e];
      ok[u] = valid && idx >= 0 && idx < a.x_rows;
      bad |= valid && !ok[u];
      s[u] = 1.0f;
      v[u] = ctr_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (ok[u]) {
        if (a.s_in) s[u] = a.s_in[idx];
        v[u] = *(const CTR_GLOBAL ctr_f32x4*)(a.x + idx * a.ldx + 4 * c);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (ok[u]) {
        acc.x = fmaf(s[u], v[u].x, acc.x);
        acc.y = fmaf(s[u], v[u].y, acc.y);
        acc.z = fmaf(s[u], v[u].z, acc.z);
        acc.w = fmaf(s[u], v[u].w, acc.w);
      }
    }
  }
  constexpr int kTop = pow2_at_least(kEpi) / 2;
  constexpr int kLevels = kTop == 0 ? 0 : 32 - __builtin_clz((unsigned)kTop);
#pragma unroll
  for (int level = 0; level < kLevels; ++level) {
    const int st = kTop >> level;
    ctr_f32x4 t;
    t.x = __shfl_down(acc.x, st * kLpr, CTR_WAVE);
    t.y = __shfl_down(acc.y, st * kLpr, CTR_WAVE);
    t.z = __shfl_down(acc.z, st * kLpr, CTR_WAVE);
    t.w = __shfl_down(acc.w, st * kLpr, CTR_WAVE);
    if (g < st && g + st < kEpi) acc += t;
  }
  return acc;
}

__device__ __forceinline__ void store_scaled(const Args& a, int64_t j, int64_t r, int c, bool row_ok, int64_t n,
                                             ctr_f32x4 total) {
  ctr_f32x4 y = {0.0f, 0.0f, 0.0f, 0.0f};      // an empty list: exact zeros whatever the scale holds
  if (row_ok && n > 0) {
    const float scale = a.s_out ? a.s_out[r] : 1.0f;
    y = total * scale;
  }
  *(CTR_GLOBAL ctr_f32x4*)(a.out + j * a.ldo + 4 * c) = y;
}

template <int KB>
__global__ __launch_bounds__(kThreads) void graph_prop_kernel(const Args a, const int32_t* __restrict__ work,
                                                              int64_t nwork) {
  const int lane = threadIdx.x & (CTR_WAVE - 1);
  const int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= nwork) return;
  int64_t j = w, seg = 0, slot = -1;      // no plan: item w is the whole of out row w
  if (work) {
    j = work[4 * w];
    seg = work[4 * w + 1];
    slot = work[4 * w + 2];
  }
  if (j < 0 || j >= a.count || seg < 0 || slot >= a.ws_slots) {
    if (lane == 0) raise(a, kErrPlan);
    return;
  }
  int64_t r, begin, end;
  const bool row_ok = row_range(a, j, r, begin, end);
  bool bad = !row_ok;
  const int64_t n = end - begin;
  const bool writer = lane < 4 * KB;      // group 0 holds the sums
  // a whole row walks its segments in ascending order; a segment item is a walk of one
  const int64_t first = slot < 0 ? 0 : seg;
  const int64_t last = slot < 0 ? (n + kSegment - 1) / kSegment : seg + 1;
  ctr_f32x4 total = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t sg = first; sg < last; ++sg) {
    const int64_t sb = begin + sg * kSegment < end ? begin + sg * kSegment : end;
    const int64_t se = sb + kSegment < end ? sb + kSegment : end;
    const ctr_f32x4 part = segment_sum<KB>(a, sb, se, lane, bad);
    total = sg == first ? part : total + part;      // the merge launch's chain: p0, then + p1, + p2, ...
  }
  if (writer) {
    if (slot < 0)
      store_scaled(a, j, r, lane, row_ok, n, total);
    else
      *(CTR_GLOBAL ctr_f32x4*)(a.ws + slot * (16 * KB) + 4 * lane) = total;
  }
  if (bad) raise(a, kErrIndex);
}

__global__ __launch_bounds__(kThreads) void graph_merge_kernel(const Args a, int k4, const int32_t* __restrict__ merge,
                                                               int64_t nmerge) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t m = t / k4;
  const int c = (int)(t - m * k4);
  if (m >= nmerge) return;
  const int64_t j = merge[2 * m], slot0 = merge[2 * m + 1];
  if (j < 0 || j >= a.count || slot0 < 0) {
    if (c == 0) raise(a, kErrPlan);
    return;
  }
  int64_t r, begin, end;
  const bool row_ok = row_range(a, j, r, begin, end);      // a bad row raised its bit in the first launch
  const int64_t n = end - begin;
  const int64_t nseg = (n + kSegment - 1) / kSegment;
  if (slot0 + nseg > a.ws_slots) {
    if (c == 0) raise(a, kErrPlan);
    return;
  }
  ctr_f32x4 total = {0.0f, 0.0f, 0.0f, 0.0f};
  const int64_t k = 4 * (int64_t)k4;
  if (nseg > 0) total = *(const CTR_GLOBAL ctr_f32x4*)(a.ws + slot0 * k + 4 * c);
  const float* next = a.ws + (slot0 + 1) * k + 4 * c;
  int64_t s = 1;
  for (; s + kUnroll <= nseg; s += kUnroll, next += kUnroll * k) {      // four loads in flight, one chain of additions
    ctr_f32x4 p[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) p[u] = *(const CTR_GLOBAL ctr_f32x4*)(next + u * k);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) total += p[u];
  }
  for (; s < nseg; ++s, next += k) total += *(const CTR_GLOBAL ctr_f32x4*)next;
  store_scaled(a, j, r, c, row_ok, n, total);
}

bool aligned_to(const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; }

bool dim_ok(int k) { return k >= 16 && k <= CTR_GRAPH_MAX_DIM && k % 16 == 0; }

constexpr int64_t kLimit = 1ll << 31;

static_assert(CTR_GRAPH_MAX_DIM == 16 * 16, "one template instance per k block of 16; a row is at most one wave wide");

}  // namespace

extern "C" int ctr_graph_propagate_workspace_bytes(int64_t partials, int k, int64_t* bytes) {
  CTR_REQUIRE(bytes && partials >= 0 && k >= 1, CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && partials < kLimit, CTR_ELIMIT);
  *bytes = partials * k * (int64_t)sizeof(float);
  return CTR_OK;
}

extern "C" int ctr_graph_propagate(const float* x, int64_t x_rows, int64_t ldx, int k, const int64_t* indptr,
                                   const int32_t* indices, int64_t num_rows, int64_t nnz, const float* s_in,
                                   const float* s_out, const int64_t* rows, int64_t count, const int32_t* work,
                                   int64_t nwork, const int32_t* merge, int64_t nmerge, float* out, int64_t ldo,
                                   void* workspace, int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(count >= 0 && x_rows >= 1 && num_rows >= 1 && k >= 1 && nnz >= 0 && nwork >= 0 && nmerge >= 0 &&
                  workspace_bytes >= 0,
              CTR_EINVAL);
  if (count == 0) return CTR_OK;
  // indices may be NULL: a CSR without a single pair
  CTR_REQUIRE(x && indptr && out && (indices || nnz == 0) && ldx >= k && ldo >= k, CTR_EINVAL);
  CTR_REQUIRE((work != nullptr) == (nwork > 0) && (merge != nullptr) == (nmerge > 0), CTR_EINVAL);
  CTR_REQUIRE(nmerge == 0 || (work && workspace), CTR_EINVAL);
  CTR_REQUIRE(dim_ok(k) && count < kLimit && x_rows < kLimit && num_rows < kLimit && nnz < kLimit && nwork < kLimit &&
                  nmerge < kLimit,
              CTR_ELIMIT);
  CTR_REQUIRE(aligned_to(x, 16) && aligned_to(out, 16) && aligned_to(workspace, 16) && ldx % 4 == 0 && ldo % 4 == 0 &&
                  aligned_to(indptr, 8) && aligned_to(indices, 4) && aligned_to(s_in, 4) && aligned_to(s_out, 4) &&
                  aligned_to(rows, 8) && aligned_to(work, 16) && aligned_to(merge, 8) && aligned_to(err_flag, 4),
              CTR_EALIGN);
  int64_t slots = workspace ? workspace_bytes / (k * (int64_t)sizeof(float)) : 0;
  if (slots >= kLimit) slots = kLimit - 1;
  const Args a{x, x_rows, ldx, indptr, indices, num_rows, nnz, s_in, s_out, rows, count, out, ldo,
               static_cast<float*>(workspace), slots, err_flag};
  hipStream_t s = (hipStream_t)stream;
  const int64_t items = work ? nwork : count;
  const dim3 grid((unsigned)ctr_ceil_div(items, kWaves));
#define GRAPH_PROP(KB) \
  case KB: hipLaunchKernelGGL((graph_prop_kernel<KB>), grid, dim3(kThreads), 0, s, a, work, items); break;
  switch (k / 16) {
    GRAPH_PROP(1) GRAPH_PROP(2) GRAPH_PROP(3) GRAPH_PROP(4) GRAPH_PROP(5) GRAPH_PROP(6) GRAPH_PROP(7) GRAPH_PROP(8)
    GRAPH_PROP(9) GRAPH_PROP(10) GRAPH_PROP(11) GRAPH_PROP(12) GRAPH_PROP(13) GRAPH_PROP(14) GRAPH_PROP(15)
    GRAPH_PROP(16)
    default: return CTR_ELIMIT;
  }
#undef GRAPH_PROP
  const int rc = ctr_launch_status();
  if (rc != CTR_OK || nmerge == 0) return rc;
  const int k4 = k / 4;
  hipLaunchKernelGGL(graph_merge_kernel, dim3((unsigned)ctr_ceil_div(nmerge * k4, kThreads)), dim3(kThreads), 0, s, a, k4,
                     merge, nmerge);
  return ctr_launch_status();
}
