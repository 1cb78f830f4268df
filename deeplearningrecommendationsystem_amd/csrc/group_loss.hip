// Pairwise and listwise ranking losses over groups of 1 positive + k drawn negatives: BPR and sampled softmax, the
// training objectives of the pipeline whose loader is ctr_load_batch_groups and whose metric is ctr_group_rank.  The
// reference trains every model with torch.nn.BCELoss (e.g. scripts/neuralcf.py) and has no loss over a group.
//
// Every model of the package returns probabilities (the reference's modules end in sigmoid), so the losses take
// probabilities, like ctr_bce_fwd, and go back to the logit first.  n groups of 1 + k samples, sample j of group g at
// prob[(g (1 + k) + j) ldp], slot 0 the positive:
//     z_i  = max(log p_i, -100) - max(log(1 - p_i), -100)            (1 - p formed in fp32, as bce_fwd_kernel; a NaN
//                                                                     stays a NaN)
//     BPR      (kind 0):  L = 1/(n k) sum_g sum_{j=1..k} softplus(z_gj - z_g0),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
//     softmax  (kind 1):  L = 1/n sum_g [ m_g + log sum_{j=0..k} exp(z_gj - m_g) - z_g0 ],   m_g = max_j z_gj
//     dL/dz:   BPR        dz_gj = sigmoid(z_gj - z_g0) / (n k)  (j >= 1),   dz_g0 = -sum_j dz_gj
//              softmax    dz_gj = (softmax_j - [j == 0]) / n
//     dL/dp_i = dz_i / max(p_i (1 - p_i), 1e-12) * gloss              (the floor ctr_bce_bwd uses; composes with the
//                                                                     model's sigmoid backward to exactly dz)
// sigmoid(x) is formed from the e = exp(-|x|) that softplus needs: 1 / (1 + e) for x >= 0, e / (1 + e) below.
//
// The logQ correction (ctr_group_loss_logq_fwd / _bwd).  Negatives drawn from a distribution q that is not uniform bias
// the sampled softmax towards the items q seldom draws; with c_i = log q(item of sample i), read at logq[i ldq] (the
// loader's log-q column), the softmax runs over
//     z'_i = z_i - c_i                      every slot, the positive's included; one fp32 subtraction before the maximum
// in place of z_i.  dL/dz' keeps its form and dz'/dz = 1, so dL/dp keeps its form and its floor.  Softmax only: kind 0
// with a logq is refused.  A null logq is the uncorrected loss, the same device code, and c == 0 everywhere gives its
// bits (z - 0.0f is z).  Only the differences of c within a group matter.  A NaN in c is a NaN loss, like a NaN in p.
//
// G lanes per group, G the smallest power of two >= 1 + k capped at 64, as group_rank_kernel; a lane takes the slots
// sub, sub + G, .. (more than one only when 1 + k > 64: every pass over the group then reads p again instead of
// keeping 64 values per lane).  Rows are only 4-byte aligned, so loads are dwords and consecutive lanes read
// consecutive floats.  In-group maxima and sums are xor-shuffles; a group's lanes all hold the result.
// The forward is bce_fwd_kernel's one launch: every workgroup stores its partial, takes a ticket, and the workgroup
// that draws the last ticket sums the <= 256 partials in index order and re-arms the ticket, so the loss is bitwise
// reproducible from run to run.  gprob_unit receives what the backward writes for gloss == 1 (the two kernels share
// group_dz, compiled without contraction into fused multiply-adds so that both round alike, and x * 1.0f is x).
// 4 B read and 4 B written per sample; the kernel is latency-bound like bce_fwd_kernel and no more tuned than that one.
#include <math.h>

#include "ctr_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxK = CTR_GROUP_MAX_K;
constexpr int kMaxGrid = 256;       // one partial per thread of the last workgroup
constexpr int kTilesPerBlock = 4;   // a workgroup takes at least this many tiles before the grid grows (bce: 4 x 256)

// the logit of a probability, both logs clamped at -100 (header comment); NaN in, NaN out
__device__ __forceinline__ float logit_of(float p) {
#pragma clang fp contract(off)
  float lp = logf(p), l1p = logf(1.0f - p);
  lp = lp < -100.0f ? -100.0f : lp;
  l1p = l1p < -100.0f ? -100.0f : l1p;
  return lp - l1p;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// dL/dz of this lane's slots of one live group, handed to emit(j, p_j, dz_j), and the group's loss term (before the
// 1/(n k) or 1/n), in every lane of the group.  row: the group's slot 0; w = 1 + k; sub: lane within the group.
// A dead group (live == false) reads nothing and shuffles along.
// crow: the group's slot 0 of logq, or null (only kind 1 comes with one): slot j's logit is then z_j - crow[j ldq].
template <int G, typename Emit>
__device__ __forceinline__ float group_dz(const float* __restrict__ row, int64_t ldp, const float* __restrict__ crow,
                                          int64_t ldq, int w, int kind, float scale, int sub, bool live, Emit emit) {
#pragma clang fp contract(off)   // forward and backward must round alike: no multiply-add fused in one and not the other
  const bool mine = live && sub < w;
  const float p_first = mine ? row[sub * ldp] : 0.5f;
  const auto z_of = [&](int j, float p) {                       // the corrected logit of slot j
    const float z = logit_of(p);
    return crow ? z - crow[j * ldq] : z;
  };
  const float z_first = mine ? z_of(sub, p_first) : logit_of(p_first);   // slot `sub`; 0 when there is none
  const float z0 = __shfl(z_first, 0, G);
  if (kind == 0) {
    float term = 0.0f, gsum = 0.0f;                             // softplus terms; sum of the negatives' dz
    for (int j = sub; j < w; j += G) {
      if (!live || j == 0) continue;
      const float pj = j == sub ? p_first : row[j * ldp];
      const float x = (j == sub ? z_first : logit_of(pj)) - z0;
      const float e = expf(-fabsf(x));
      term += (x > 0.0f ? x : 0.0f) + log1pf(e);
      const float dz = (x >= 0.0f ? 1.0f : e) / (1.0f + e) * scale;
      gsum += dz;
      emit(j, pj, dz);
    }
    term = ctr_group_sum<G>(term);
    gsum = ctr_group_sum<G>(gsum);
    if (live && sub == 0) emit(0, p_first, -gsum);
    return term;
  }
  float m = mine ? z_first : -INFINITY;
  for (int j = sub + G; j < w && live; j += G) m = fmaxf(m, z_of(j, row[j * ldp]));
  m = group_max<G>(m);
  float e_first = mine ? expf(z_first - m) : 0.0f, sum = e_first;
  for (int j = sub + G; j < w && live; j += G) sum += expf(z_of(j, row[j * ldp]) - m);
  sum = ctr_group_sum<G>(sum);
  if (mine) emit(sub, p_first, (e_first / sum - (sub == 0 ? 1.0f : 0.0f)) * scale);
  for (int j = sub + G; j < w && live; j += G) {
    const float pj = row[j * ldp];
    emit(j, pj, expf(z_of(j, pj) - m) / sum * scale);
  }
  return m + logf(sum) - z0;
}

__device__ __forceinline__ float dp_of(float p, float dz) {
#pragma clang fp contract(off)
  return dz / fmaxf((1.0f - p) * p, 1e-12f);
}

template <int G>
__global__ void __launch_bounds__(kBlock)
group_loss_fwd_kernel(const float* __restrict__ prob, int64_t ldp, const float* __restrict__ logq /* nullable */,
                      int64_t ldq, int64_t n, int k, int kind, float scale, float* __restrict__ partial, unsigned int* __restrict__ ticket, float* __restrict__ loss,
                      float* __restrict__ gp1 /* nullable: d loss / d p for an upstream gradient of exactly 1 */) {
  __shared__ float s_red[kBlock / 64];
  __shared__ bool s_last;
  constexpr int kPer = kBlock / G;
  const int sub = threadIdx.x & (G - 1), w = 1 + k;
  const int64_t tiles = (n + kPer - 1) / kPer;
  float acc = 0.0f;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t g = tile * kPer + threadIdx.x / G;
    const bool live = g < n;
    const int64_t first = g * w;
    const float term = group_dz<G>(prob + first * ldp, ldp, logq ? logq + first * ldq : nullptr, ldq, w, kind, scale, sub,
                                   live, [&](int j, float p, float dz) {
                                     if (gp1) gp1[first + j] = dp_of(p, dz);
                                   });
    if (live && sub == 0) acc += term;
  }
  acc = ctr_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
    for (int v = 0; v < kBlock / 64; ++v) t += s_red[v];
    __hip_atomic_store(partial + blockIdx.x, t * scale, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // release my partial, acquire everybody else's if I am last
    const unsigned int drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = drawn == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // gridDim.x <= 256 = kBlock partials: one per thread, summed in a fixed tree
  float v = threadIdx.x < gridDim.x
                ? __hip_atomic_load(partial + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : 0.0f;
  v = ctr_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
    for (int x = 0; x < kBlock / 64; ++x) t += s_red[x];
    loss[0] = t;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int G>
__global__ void __launch_bounds__(kBlock)
group_loss_bwd_kernel(const float* __restrict__ prob, int64_t ldp, const float* __restrict__ logq /* nullable */,
                      int64_t ldq, int64_t n, int k, int kind, float scale, const float* __restrict__ gloss, float* __restrict__ gp, int64_t ldg) {
  constexpr int kPer = kBlock / G;
  const int sub = threadIdx.x & (G - 1), w = 1 + k;
  const int64_t tiles = (n + kPer - 1) / kPer;
  const float up = gloss[0];
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t g = tile * kPer + threadIdx.x / G;
    const bool live = g < n;
    const int64_t first = g * w;
    group_dz<G>(prob + first * ldp, ldp, logq ? logq + first * ldq : nullptr, ldq, w, kind, scale, sub, live,
                [&](int j, float p, float dz) { gp[(first + j) * ldg] = dp_of(p, dz) * up; });
  }
}

template <int G>
void launch_fwd(const float* prob, int64_t ldp, const float* logq, int64_t ldq, int64_t n, int k, int kind, float scale,
                float* ws, unsigned int* ticket, float* loss, float* gp1, int64_t grid, hipStream_t st) {
  hipLaunchKernelGGL(group_loss_fwd_kernel<G>, dim3((unsigned)grid), dim3(kBlock), 0, st, prob, ldp, logq, ldq, n, k, kind,
                     scale, ws, ticket, loss, gp1);
}

template <int G>
void launch_bwd(const float* prob, int64_t ldp, const float* logq, int64_t ldq, int64_t n, int k, int kind, float scale,
                const float* gloss, float* gp, int64_t ldg, hipStream_t st) {
  hipLaunchKernelGGL(group_loss_bwd_kernel<G>, dim3(ctr_stream_grid(n, kBlock / G)), dim3(kBlock), 0, st, prob, ldp, logq,
                     ldq, n, k, kind, scale, gloss, gp, ldg);
}

int lanes_per_group(int k) {
  int g = 2;
  while (g < 1 + k && g < 64) g *= 2;
  return g;
}

// 1 / (n k) for BPR, 1 / n for softmax
float loss_scale(int64_t n, int k, int kind) { return kind == 0 ? 1.0f / ((float)n * (float)k) : 1.0f / (float)n; }

bool group_args_ok(const float* prob, int64_t ldp, int64_t n, int k, int kind) {
  return prob && ldp >= 1 && n > 0 && n <= (1ll << 40) && k >= 1 && k <= kMaxK && (kind == 0 || kind == 1);
}

// a logq goes with the softmax only, and with a stride
bool logq_ok(const float* logq, int64_t ldq, int kind) { return !logq || (kind == 1 && ldq >= 1); }

// both forward entry points; logq null: the uncorrected loss
int group_fwd(const float* prob, int64_t ldp, const float* logq, int64_t ldq, int64_t n, int k, int kind, float* loss,
              float* workspace, int64_t workspace_floats, unsigned int* ticket, float* gprob_unit, hipStream_t st) {
  CTR_REQUIRE(group_args_ok(prob, ldp, n, k, kind) && logq_ok(logq, ldq, kind) && loss && workspace && ticket, CTR_EINVAL);
  const int G = lanes_per_group(k);
  int64_t grid = ctr_ceil_div(ctr_ceil_div(n, kBlock / G), kTilesPerBlock);
  if (grid > kMaxGrid) grid = kMaxGrid;
  CTR_REQUIRE(workspace_floats >= grid, CTR_ELIMIT);
  const float scale = loss_scale(n, k, kind);
  switch (G) {
    case 2: launch_fwd<2>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
    case 4: launch_fwd<4>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
    case 8: launch_fwd<8>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
    case 16: launch_fwd<16>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
    case 32: launch_fwd<32>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
    default: launch_fwd<64>(prob, ldp, logq, ldq, n, k, kind, scale, workspace, ticket, loss, gprob_unit, grid, st); break;
  }
  return ctr_launch_status();
}

int group_bwd(const float* prob, int64_t ldp, const float* logq, int64_t ldq, int64_t n, int k, int kind,
              const float* gloss, float* gprob, int64_t ldg, hipStream_t st) {
  CTR_REQUIRE(group_args_ok(prob, ldp, n, k, kind) && logq_ok(logq, ldq, kind) && gloss && gprob && ldg >= 1, CTR_EINVAL);
  const float scale = loss_scale(n, k, kind);
  switch (lanes_per_group(k)) {
    case 2: launch_bwd<2>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
    case 4: launch_bwd<4>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
    case 8: launch_bwd<8>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
    case 16: launch_bwd<16>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
    case 32: launch_bwd<32>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
    default: launch_bwd<64>(prob, ldp, logq, ldq, n, k, kind, scale, gloss, gprob, ldg, st); break;
  }
  return ctr_launch_status();
}

}  // namespace

extern "C" int ctr_group_loss_fwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, float* loss,
                                  float* workspace, int64_t workspace_floats, unsigned int* ticket, float* gprob_unit,
                                  void* stream) {
  return group_fwd(prob, ldp, nullptr, 0, n, k, kind, loss, workspace, workspace_floats, ticket, gprob_unit,
                   (hipStream_t)stream);
}

extern "C" int ctr_group_loss_bwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, const float* gloss,
                                  float* gprob, int64_t ldg, void* stream) {
  return group_bwd(prob, ldp, nullptr, 0, n, k, kind, gloss, gprob, ldg, (hipStream_t)stream);
}

extern "C" int ctr_group_loss_logq_fwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, float* loss,
                                       float* workspace, int64_t workspace_floats, unsigned int* ticket,
                                       float* gprob_unit, const float* logq, int64_t ldq, void* stream) {
  return group_fwd(prob, ldp, logq, ldq, n, k, kind, loss, workspace, workspace_floats, ticket, gprob_unit,
                   (hipStream_t)stream);
}

extern "C" int ctr_group_loss_logq_bwd(const float* prob, int64_t ldp, int64_t n, int k, int kind, const float* gloss,
                                       float* gprob, int64_t ldg, const float* logq, int64_t ldq, void* stream) {
  return group_bwd(prob, ldp, logq, ldq, n, k, kind, gloss, gprob, ldg, (hipStream_t)stream);
}
