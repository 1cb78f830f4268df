// GDCF (GDCF_Final.py of the reference): BCEWithLogitsLoss with mean reduction over ALL m x n entries of the 0/1
// user x item matrix Y, scores S = P Q^T, and its gradients
//     loss = sum_{u,i} softplus(s_ui) - y_ui s_ui / (m n),   G = sigmoid(S) - Y,   dP = G Q / (m n),   dQ = G^T P / (m n)
// on the fp32 matrix cores.  The m x n scores, G and loss terms only ever exist as register tiles.
//
// Both passes are one kernel: a workgroup OWNS 64 rows of X (4 waves x 16), walks every 16-row tile of the STREAMED
// matrix Z in ascending order, and accumulates grad_X = G Z over the walk in registers.
//   row pass   : X = P (owner = user), Z = Q, Y the (m, cols_pad) matrix           -> loss partials and dP
//   column pass: X = Q (owner = item), Z = P, Y = its transpose (n, pad64(m))      -> dQ
// Per tile a wave forms Z_t X_w^T (16 streamed x 16 owners) with v_mfma_f32_16x16x4_f32:
//   A = Z tile (row = streamed l&15, k step from l>>4), B = X^T (k step from l>>4, col = owner l&15);
//   k step s of lane group q is dimension 16 (s>>2) + 4q + (s&3) for A and B alike, so a lane reads its X and Z
//   operands four consecutive floats at a time (k is zero padded to 16 KB in LDS and in the registers of X).
// D has the streamed row in 4 (l>>4) + reg and the owner in l&15: a lane holds four consecutive streamed rows of one
// owner, whose four Y bytes are one 32-bit load.  G in that layout is the B operand of the gradient product
//   grad_X^T (k x owners) += Z_t^T (k x streamed) G^T (streamed x owners)
// as it stands (its row index is the reduction index): MFMA c of k block b takes lane register c of G and A =
// Z^T[16 b + (l&15)][4 (l>>4) + c], read from a transposed LDS copy of the tile, four at a time.  The accumulator has
// dimension 16 b + 4 (l>>4) + reg of owner l&15, stored once after the walk.
//
// Padding streamed rows (>= ns, including the int8 padding columns of Y) and padding owner rows are excluded from the
// loss and from both gradients.  The loss goes per workgroup into a float64 partial, reduced in a fixed order by a
// second launch; no atomics anywhere, so every output is bitwise reproducible.
#include "ctr_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kOwn = 16;                 // owner rows per wave
constexpr int kBO = kWaves * kOwn;       // owner rows per workgroup
constexpr int kTS = 16;                  // streamed rows per tile
constexpr int kTRow = kTS + 4;           // transposed tile row in LDS (floats; 16-byte aligned, staggers banks)

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// KB = k blocks of 16.  LOSS: per-workgroup loss partials.  GRAD: grad_X (else only the scores are formed).
template <int KB, bool LOSS, bool GRAD>
__global__ __launch_bounds__(kThreads) void gdcf_pass_kernel(const float* __restrict__ X, int64_t no,
                                                             const float* __restrict__ Z, int64_t ns, int k,
                                                             const int8_t* __restrict__ Y, int64_t ldy, double inv_mn,
                                                             const float* __restrict__ gout, float* __restrict__ grad,
                                                             double* __restrict__ partials) {
  constexpr int KP = 16 * KB;            // padded k
  constexpr int KRow = KP + 4;           // natural tile row in LDS (floats)
  constexpr int kStage = kTS * KP / kThreads;   // tile elements staged per thread (= KB)
  __shared__ float s_zn[2][kTS * KRow];
  __shared__ float s_zt[GRAD ? 2 : 1][GRAD ? KP * kTRow : 1];
  __shared__ double s_loss[kWaves];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t o = (int64_t)blockIdx.x * kBO + wave * kOwn + r;   // this lane's owner row (B column / D column)
  const bool own_ok = o < no;

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
  double lsum = 0.0;

  const int64_t T = (ns + kTS - 1) / kTS;
  float stage[kStage];
  auto load_tile = [&](int64_t t) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int e = threadIdx.x + i * kThreads, row = e / KP, col = e % KP;
      const int64_t zr = t * kTS + row;
      stage[i] = (zr < ns && col < k) ? Z[zr * k + col] : 0.0f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kStage; ++i) {
      const int e = threadIdx.x + i * kThreads, row = e / KP, col = e % KP;
      s_zn[buf][row * KRow + col] = stage[i];
      if constexpr (GRAD) s_zt[buf][col * kTRow + row] = stage[i];
    }
  };
  const int8_t* yrow = Y + (own_ok ? o : 0) * ldy + 4 * q;
  auto load_y = [&](int64_t t) -> uint32_t {
    return own_ok ? *reinterpret_cast<const uint32_t*>(yrow + t * kTS) : 0u;
  };

  load_tile(0);
  store_tile(0);
  uint32_t ycur = load_y(0);
  __syncthreads();

  for (int64_t t = 0; t < T; ++t) {
    const int buf = (int)(t & 1);
    const bool more = t + 1 < T;
    if (more) load_tile(t + 1);
    const uint32_t ynext = more ? load_y(t + 1) : 0u;

    // scores: two independent accumulator chains over the k steps
    const float* zn = &s_zn[buf][r * KRow + 4 * q];
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(zn + 16 * j);
      s0 = mfma4(a[0], xb[4 * j + 0], s0);
      s1 = mfma4(a[1], xb[4 * j + 1], s1);
      s0 = mfma4(a[2], xb[4 * j + 2], s0);
      s1 = mfma4(a[3], xb[4 * j + 3], s1);
    }

    float g[4];
    float tl = 0.0f;
    const int64_t srow = t * kTS + 4 * q;   // streamed row of register 0
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float s = s0[c] + s1[c];
      const float y = (float)((ycur >> (8 * c)) & 0xffu);
      const bool ok = own_ok && srow + c < ns;
      const float e = expf(-fabsf(s));   // stable: never exp of a positive argument
      // max(s, 0) - y s is exact for y in {0, 1}, so a saturated correct score keeps its log1p(e) term
      if constexpr (LOSS) tl += ok ? (fmaxf(s, 0.0f) - y * s) + log1pf(e) : 0.0f;
      if constexpr (GRAD) {
        // sigmoid(s) - y as sigmoid(s) (y = 0) or -sigmoid(-s) (y = 1): the small side of a saturated score survives
        const float r1 = 1.0f / (1.0f + e), big = r1, small = e * r1;
        const float g_ = y != 0.0f ? -(s >= 0.0f ? small : big) : (s >= 0.0f ? big : small);
        g[c] = ok ? g_ : 0.0f;
      }
    }
    if constexpr (LOSS) lsum += (double)tl;

    if constexpr (GRAD) {
      const float* zt = &s_zt[buf][r * kTRow + 4 * q];
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(zt + 16 * b * kTRow);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[b] = mfma4(a[c], g[c], acc[b]);
      }
    }

    if (more) store_tile(buf ^ 1);
    ycur = ynext;
    __syncthreads();
  }

  if constexpr (GRAD) {
    if (own_ok) {
      const float sc = (float)(inv_mn * (gout ? (double)gout[0] : 1.0));
#pragma unroll
      for (int b = 0; b < KB; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int d = 16 * b + 4 * q + c;
          if (d < k) grad[o * k + d] = acc[b][c] * sc;
        }
    }
  }
  if constexpr (LOSS) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) lsum += __shfl_xor(lsum, m, 64);
    if (lane == 0) s_loss[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double v = 0.0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) v += s_loss[w];
      partials[blockIdx.x] = v;
    }
  }
}

// loss = (sum of the partials in a fixed order) / (m n), one workgroup
__global__ __launch_bounds__(kThreads) void gdcf_loss_kernel(const double* __restrict__ partials, int64_t n,
                                                             double inv_mn, float* __restrict__ loss) {
  __shared__ double s[kThreads];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) v += partials[i];
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(s[0] * inv_mn);
}

template <bool LOSS, bool GRAD>
int launch_pass(int kb, const float* X, int64_t no, const float* Z, int64_t ns, int k, const int8_t* Y, int64_t ldy,
                double inv_mn, const float* gout, float* grad, double* partials, hipStream_t stream) {
  const dim3 grid((unsigned)ctr_ceil_div(no, kBO)), block(kThreads);
#define GDCF_CASE(KB)                                                                                            \
  case KB:                                                                                                     \
    hipLaunchKernelGGL((gdcf_pass_kernel<KB, LOSS, GRAD>), grid, block, 0, stream, X, no, Z, ns, k, Y, ldy, \
                       inv_mn, gout, grad, partials);                                                          \
    break;
  switch (kb) {
    GDCF_CASE(1) GDCF_CASE(2) GDCF_CASE(3) GDCF_CASE(4) GDCF_CASE(5) GDCF_CASE(6) GDCF_CASE(7) GDCF_CASE(8)
    GDCF_CASE(9) GDCF_CASE(10) GDCF_CASE(11) GDCF_CASE(12) GDCF_CASE(13) GDCF_CASE(14) GDCF_CASE(15) GDCF_CASE(16)
    default: return CTR_ELIMIT;
  }
#undef GDCF_CASE
  return ctr_launch_status();
}

static_assert(CTR_GDCF_MAX_DIM == 16 * 16, "one template instance per k block of 16");

int gdcf_check(const float* p, const float* q, int64_t num_users, int64_t num_items, int k, const int8_t* y,
               int64_t ldy, int64_t y_rows_valid) {
  CTR_REQUIRE(num_users >= 1 && num_items >= 1 && k >= 1, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_GDCF_MAX_DIM && num_users < (1ll << 40) && num_items < (1ll << 40), CTR_ELIMIT);
  CTR_REQUIRE(ldy >= y_rows_valid && ldy % 64 == 0, CTR_EINVAL);
  CTR_REQUIRE(p && q && y, CTR_EINVAL);
  CTR_REQUIRE(ctr_aligned16(y), CTR_EALIGN);
  return CTR_OK;
}

}  // namespace

extern "C" int ctr_gdcf_workspace_bytes(int64_t num_users, int64_t num_items, int k, int64_t* bytes) {
  CTR_REQUIRE(bytes && num_users >= 1 && num_items >= 1 && k >= 1, CTR_EINVAL);
  CTR_REQUIRE(k <= CTR_GDCF_MAX_DIM, CTR_ELIMIT);
  *bytes = ctr_ceil_div(num_users, kBO) * (int64_t)sizeof(double);
  return CTR_OK;
}

extern "C" int ctr_gdcf_rows(const float* p, const float* q, int64_t num_users, int64_t num_items, int k,
                             const int8_t* y, int64_t ldy, float* loss, float* grad_p, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  const int rc = gdcf_check(p, q, num_users, num_items, k, y, ldy, num_items);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(loss && workspace, CTR_EINVAL);
  CTR_REQUIRE(workspace_bytes >= ctr_ceil_div(num_users, kBO) * (int64_t)sizeof(double), CTR_EINVAL);
  const double inv_mn = 1.0 / ((double)num_users * (double)num_items);
  const int kb = (k + 15) / 16;
  double* parts = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int r = grad_p ? launch_pass<true, true>(kb, p, num_users, q, num_items, k, y, ldy, inv_mn, nullptr, grad_p,
                                                 parts, s)
                       : launch_pass<true, false>(kb, p, num_users, q, num_items, k, y, ldy, inv_mn, nullptr, nullptr,
                                                  parts, s);
  if (r != CTR_OK) return r;
  hipLaunchKernelGGL(gdcf_loss_kernel, dim3(1), dim3(kThreads), 0, s, parts, ctr_ceil_div(num_users, kBO), inv_mn,
                     loss);
  return ctr_launch_status();
}

extern "C" int ctr_gdcf_cols(const float* p, const float* q, int64_t num_users, int64_t num_items, int k,
                             const int8_t* yt, int64_t ldyt, const float* gout, float* grad_q, void* stream) {
  const int rc = gdcf_check(p, q, num_users, num_items, k, yt, ldyt, num_users);
  if (rc != CTR_OK) return rc;
  CTR_REQUIRE(gout && grad_q, CTR_EINVAL);
  const double inv_mn = 1.0 / ((double)num_users * (double)num_items);
  return launch_pass<false, true>((k + 15) / 16, q, num_items, p, num_users, k, yt, ldyt, inv_mn, gout, grad_q,
                                  nullptr, (hipStream_t)stream);
}
