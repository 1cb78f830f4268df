// NeuralCF over the whole user x item GRID: scores of `rows` users against every item, in one launch, with no id
// tensor anywhere (ctr_ncf_grid_scores; model/neuralcf.py score_rows / score_grid / recommend).
//
// The per-sample forward (ncf_proj.hip, ncfp_fwd_kernel) reads two ids per pair, gathers four 256-byte table rows and
// stores 228 bytes of activations for a backward that an evaluation never runs.  On a grid the pairs are not a bag of
// samples: the sixteen pairs of a matrix-core group can share their USER, and a wave can keep its sixteen ITEMS for as
// long as it likes.  With the first tower layer on the table rows (ncf_proj.hip's header),
//     z0[u, i] = P_U[u] + P_I[i],     P_U = MLP_U W0[:, :64]^T,     P_I = MLP_I W0[:, 64:]^T + b0,
//     out[u, i] = act([GMF_U[u] * GMF_I[i] | tower(relu(z0[u, i]))] . wfold + cfold)
// a wave owns sixteen consecutive items: lane (q, n) loads, ONCE, the operand-layout pieces of P_I[i0 + n] (columns
// 16j + 4q ..) and the head's columns 16q .. 16q + 15 of GMF_I[i0 + n] -- 32 registers; the uncoalesced pattern
// ncf_proj.hip warns about (neighbouring lanes, different rows) is paid once per item tile and amortised over every
// user of the tile, so these are plain loads.  The workgroup stages P_U[u] and wfold[:64] * GMF_U[u] of its kUT users
// in LDS (coalesced, sixteen lanes a row); the waves then walk the users: the user's pieces are LDS broadcasts (the
// sixteen lanes of a quarter read one address), a0 = relu(P_I + P_U), three layer_fwd, the 64 + 8 term dot, two
// shuffles, one store of the wave's sixteen scores.  The four waves take adjacent item tiles: 256 contiguous bytes per
// user and workgroup.  Items past num_items: loads clamped to the last row, stores masked.  No atomics and no order
// dependence between pairs: a pair's score depends on its two table rows and the weights alone (a matrix-core column
// is computed from that column's operands only), so the output is bitwise the same for any user list, row range or
// item order.
//
// Cost: 44 v_mfma_f32_16x16x4_f32 per sixteen pairs (5376 flop a pair with the head), 1408 issue cycles per SIMD; the
// weight prologue is of the order of 10^4 cycles per workgroup against 4 x 32 groups x
// 1408 cycles per user tile, and a workgroup walks several user tiles once the grid's second dimension is exhausted.
#include "grid_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 3;                          // the layers behind the projected one
constexpr int kK[kL] = {64, 32, 16};
constexpr int kN[kL] = {32, 16, 8};
constexpr int kN0 = 64;                        // width of a projected row
constexpr int kP = 64;                         // GMF width = the head's extra columns
constexpr int kNL = 8;                         // head: last activations
constexpr int kUT = 128;                       // users of a user tile: 64 KiB of staged rows, two workgroups a CU
constexpr int kItems = 16 * kWaves;            // items of a workgroup

#include "mfma16_tower.inc"
#include "grid_frame.inc"

constexpr int kHeadFloats = 16;                // wfold[64 .. 71], cfold, pad
constexpr int kLdsFloats = kWFloats + kBFloats + kHeadFloats + 2 * kUT * 64;
static_assert((kUT * 16) % kThreads == 0, "staging: whole passes of the workgroup over the tile's 16-byte pieces");
constexpr int kStagePasses = kUT * 16 / kThreads;

struct Grid {
  const float* pu; const float* pi;            // (nu, 64), (ni, 64) projected rows
  const float* gu; const float* gi;            // (nu, 64), (ni, 64) GMF tables
  const float* wfold; const float* cfold;      // 72 weights, 1 bias
  const int64_t* users; int64_t user0;         // the users of the rows: users[r], or user0 + r
  int64_t rows, nu, ni;
  float* out; int64_t ldo;
  int act;
  int64_t utiles;
};

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
ncf_grid_scores_kernel(const Tower T, const Grid G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_hw = s_b + kBFloats;                       // kHeadFloats
  float* s_pu = s_hw + kHeadFloats;                   // kUT x 64: P_U rows of the user tile
  float* s_gw = s_pu + kUT * 64;                      // kUT x 64: wfold[:64] * GMF_U rows
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: the tower's weights, the head's tail, this lane's pieces of its item's two rows
  f32x4 pI[4], gI[4];
  f32x4 wf4;                                          // wfold[4c .. 4c + 3] of the staging chunk c = thread % 16
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
    const float hw = *(threadIdx.x < kNL ? G.wfold + kP + threadIdx.x : G.cfold);
#pragma unroll
    for (int c = 0; c < 4; ++c) wf4[c] = G.wfold[4 * (threadIdx.x & 15) + c];
#pragma unroll
    for (int j = 0; j < 4; ++j) pI[j] = ldg4(G.pi + ic * kN0 + 16 * j + 4 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) gI[i] = ldg4(G.gi + ic * kP + 16 * q + 4 * i);
    stage_forward_store(s_w, s_b, wv, wdst, bv);
    if (threadIdx.x < kHeadFloats) s_hw[threadIdx.x] = threadIdx.x <= kNL ? hw : 0.0f;
  }
  float* const orow = G.out + item;
  const bool store = q == 0 && item < G.ni;
  for (int64_t ut = blockIdx.y; ut < G.utiles; ut += gridDim.y) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    __syncthreads();                                  // the previous tile's rows are read
    {
      // the tile's rows, sixteen lanes a row: every request before the first LDS store
      f32x4 vp[kStagePasses], vg[kStagePasses];
#pragma unroll
      for (int e = 0; e < kStagePasses; ++e) {
        const int row = (threadIdx.x >> 4) + e * (kThreads / 16);
        const int64_t u = grid_user(G.users, G.user0, G.nu, r0, cnt, row);
        vp[e] = ldg4(G.pu + u * kN0 + 4 * (threadIdx.x & 15));
        vg[e] = ldg4(G.gu + u * kP + 4 * (threadIdx.x & 15));
      }
#pragma unroll
      for (int e = 0; e < kStagePasses; ++e) {
        const int at = ((threadIdx.x >> 4) + e * (kThreads / 16)) * 64 + 4 * (threadIdx.x & 15);
        *reinterpret_cast<f32x4*>(s_pu + at) = vp[e];
        *reinterpret_cast<f32x4*>(s_gw + at) = vg[e] * wf4;
      }
    }
    __syncthreads();                                  // (the first tile: the weights as well)
    const float hc = s_hw[kNL];
    // the user's pieces are read one user ahead of the products that consume them
    f32x4 pU[4], xw[4];
    auto fetch = [&](int r) {
#pragma unroll
      for (int j = 0; j < 4; ++j) pU[j] = *reinterpret_cast<const f32x4*>(s_pu + r * 64 + 16 * j + 4 * q);
#pragma unroll
      for (int i = 0; i < 4; ++i) xw[i] = *reinterpret_cast<const f32x4*>(s_gw + r * 64 + 16 * q + 4 * i);
    };
    fetch(0);
    for (int r = 0; r < cnt; ++r) {
      f32x4 a0[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 z = pI[j] + pU[j];
#pragma unroll
        for (int c = 0; c < 4; ++c) a0[j][c] = fmaxf(z[c], 0.0f);
      }
      // head, GMF part: the four lanes of an item hold sixteen terms each
      float dot = 0.0f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        dot = fmaf(gI[i][0], xw[i][0], dot); dot = fmaf(gI[i][1], xw[i][1], dot);
        dot = fmaf(gI[i][2], xw[i][2], dot); dot = fmaf(gI[i][3], xw[i][3], dot);
      }
      fetch(r + 1 < cnt ? r + 1 : r);
      f32x4 y1[2], y2[1], y3[1];
      layer_fwd<0, 4>(s_w, s_b, lane, q, a0, y1);
      layer_fwd<1, 2>(s_w, s_b, lane, q, y1, y2);
      layer_fwd<2, 1>(s_w, s_b, lane, q, y2, y3);
      {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(s_hw + 4 * (q & 1));
        float d2 = y3[0][0] * wv[0];
        d2 = fmaf(y3[0][1], wv[1], d2); d2 = fmaf(y3[0][2], wv[2], d2); d2 = fmaf(y3[0][3], wv[3], d2);
        dot += q < 2 ? d2 : 0.0f;
      }
      dot = column_sum(dot);
      if (store) orow[(r0 + r) * G.ldo] = ctr_act(dot + hc, G.act);   // (the four lanes of an item agree)
    }
  }
}

}  // namespace

extern "C" int ctr_ncf_grid_scores(const float* p_user, const float* p_item, const float* gmf_user, const float* gmf_item,
                                   int64_t num_users, int64_t num_items, int mf_dim, int width,
                                   const ctr_mlp_layer_t* layers, int nlayers, const float* wfold, const float* cfold,
                                   int fold_k, const int64_t* users, int64_t user0, int64_t rows, int act, float* out,
                                   int64_t ldo, void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && nlayers >= 0, CTR_EINVAL);
  CTR_REQUIRE(p_user && p_item && gmf_user && gmf_item && layers && wfold && cfold, CTR_EINVAL);
  CTR_REQUIRE(act >= CTR_ACT_NONE && act <= CTR_ACT_SIGMOID, CTR_EINVAL);
  if (mf_dim != kP || width != kN0 || nlayers != kL || fold_k != kNL) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  Tower T;
  for (int l = 0; l < kL; ++l) {
    const ctr_mlp_layer_t& s = layers[l];
    if (s.n != kN[l] || s.k != kK[l] || s.act != CTR_ACT_RELU || !s.w || !s.b) return CTR_ELIMIT;
    if (!ctr_aligned16(s.w)) return CTR_EALIGN;
    T.w[l] = s.w; T.b[l] = s.b; T.y[l] = nullptr; T.ldy[l] = 0;
  }
  if (!ctr_aligned16(p_user) || !ctr_aligned16(p_item) || !ctr_aligned16(gmf_user) || !ctr_aligned16(gmf_item))
    return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  const int64_t utiles = ctr_ceil_div(rows, kUT);
  const Grid G{p_user, p_item, gmf_user, gmf_item, wfold, cfold, users, user0, rows, num_users, num_items, out, ldo, act,
               utiles};
  // item tiles along x (neighbouring workgroups share their user tile's rows in L2), user tiles along y
  const dim3 grid((unsigned)ctr_ceil_div(num_items, kItems), grid_clamp_y(utiles, utiles));
  return grid_launch(ncf_grid_scores_kernel, grid, kThreads, sizeof(float) * (size_t)kLdsFloats, stream, T, G);
}
