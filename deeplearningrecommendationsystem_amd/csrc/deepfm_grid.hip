// DeepFM over the whole user x item GRID: scores of `rows` users against every item, in one launch, with no feature
// matrix anywhere (ctr_deepfm_grid_scores; model/deepfm.py catalogue_scorer).
//
// Every column of the (B, 45) feature row depends on the user alone or on the item alone, and the first deep layer
// (`linear`) has no activation, so on a grid the model splits exactly:
//     fm[u, i]  = a[u] + b[i] + <SU[u], SI[i]>                      (SU / SI: the sums of a side's field vectors)
//     h1[u, i]  = relu(ZU[u] + ZI[i])                               (ZU / ZI: W1 W0 on a side's columns of emb, 256 wide)
//     h2 = relu(W2 h1 + b2)    h3 = relu(w3 . h2 + b3)    out[u, i] = sigmoid(o0 fm + o1 h3 + ob)
// The walk is ncf_grid.hip's: a wave owns sixteen consecutive items; lane (q, n) loads, ONCE, the operand-layout pieces
// of ZI[i0 + n] (columns 16j + 4q .., 64 registers), its quarter of SI[i0 + n] (E/4 floats) and b[i0 + n].  The
// workgroup stages ZU[u], SU[u] and a[u] of kUT users in LDS (coalesced); the waves then walk the users: the user's
// pieces are LDS broadcasts, a0 = relu(ZI + ZU), ONE layer_fwd (256 -> 128: 512 v_mfma_f32_16x16x4_f32), the 128-term
// w3 dot and the E-term FM dot, each reduced over the four lanes of a column, the head, one store of sixteen scores.
// Items past num_items: loads clamped to the last row, stores masked.  No atomics and no order dependence between
// pairs: a score is a function of its user's rows, its item's rows and the weights alone (a matrix-core column is
// computed from that column's operands only), so the output is bitwise the same for any user list, row range, item
// order or launch geometry.
//
// Budget: the 256 x 128 weights in operand order are 128 KiB of the 160 KiB of LDS, so ONE workgroup per CU; eight
// waves, two per SIMD, so that one wave's LDS reads and head sit beside its partner's matrix products.  A sixteen-pair
// group costs 16 384 matrix-core issue cycles per SIMD and the weight prologue of the order of 10^4, so -- unlike
// ncf_grid.hip -- a user tile does NOT get a workgroup of its own: gridDim.y is chosen so that the grid is a small
// multiple of the CU count and every workgroup loops over many user tiles (grid_host.h, grid_row_blocks).
#include "grid_host.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 1;                          // the layer on the matrix cores
constexpr int kK[kL] = {256};
constexpr int kN[kL] = {128};
constexpr int kN0 = 256;                       // width of a ZU / ZI row
constexpr int kN2 = 128;                       // width of h2 = the w3 dot
constexpr int kUT = CTR_DEEPFM_GRID_USER_TILE; // users of a user tile
constexpr int kItems = CTR_DEEPFM_GRID_ITEM_TILE;   // items of a workgroup
static_assert(kItems == 16 * kWaves, "a wave owns sixteen items");
static_assert(CTR_WIDEDEEP_GRID_ITEM_TILE == kItems && CTR_WIDEDEEP_GRID_USER_TILE == kUT, "one template, one tiling");

#include "mfma16_tower.inc"
#include "grid_frame.inc"

constexpr int kHeadFloats = 16;                // b3, o0, o1, ob, pad
constexpr int kFixedFloats = kWFloats + kBFloats + kN2 + kHeadFloats;
constexpr int lds_floats(int e) { return kFixedFloats + kUT * (kN0 + e) + kUT; }
static_assert(sizeof(float) * lds_floats(128) <= 160 * 1024, "the widest embedding fits the CU's LDS");
static_assert((kUT * (kN0 / 4)) % kThreads == 0, "ZU staging: whole passes of the workgroup over the tile's 16-byte pieces");
constexpr int kStagePasses = kUT * (kN0 / 4) / kThreads;
static_assert(kUT * (128 / 4) <= kThreads, "SU staging: one pass");

struct Grid {
  const float* zu; const float* zi;            // (nu, 256), (ni, 256)
  const float* su; const float* si;            // (nu, E), (ni, E)
  const float* a; const float* b;              // (nu), (ni)
  const float* w3; const float* b3;            // 128 weights, 1 bias
  const float* ow; const float* ob;            // the output layer: 2 weights (fm, deep), 1 bias
  const int64_t* users; int64_t user0;         // the users of the rows: users[r], or user0 + r
  int64_t rows, nu, ni;
  float* out; int64_t ldo;
  int64_t utiles;
};

// E = 16 E16: a lane holds E16 16-byte pieces of its item's SI row.  E16 == 0 is Wide & Deep (ctr_widedeep_grid_scores):
// the same model without the FM dot -- su / si, their registers and their LDS stage are compiled out
template <int E16>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
deepfm_grid_scores_kernel(const Tower T, const Grid G) {
  constexpr int E = 16 * E16, E4 = E / 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_w3 = s_b + kBFloats;                       // kN2
  float* s_hd = s_w3 + kN2;                           // kHeadFloats
  float* s_zu = s_hd + kHeadFloats;                   // kUT x 256: ZU rows of the user tile
  float* s_su = s_zu + kUT * kN0;                     // kUT x E: SU rows
  float* s_a = s_su + kUT * E;                        // kUT: a[u]
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: the layer's weights, the head, this lane's pieces of its item's rows
  f32x4 zI[16], sI[E16 > 0 ? E16 : 1];
  float bI;
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
    const float w3v = G.w3[threadIdx.x & (kN2 - 1)];
    const float* hp = threadIdx.x == 0 ? G.b3 : threadIdx.x == 1 ? G.ow : threadIdx.x == 2 ? G.ow + 1 : G.ob;
    const float hv = *hp;
#pragma unroll
    for (int j = 0; j < 16; ++j) zI[j] = ldg4(G.zi + ic * kN0 + 16 * j + 4 * q);
    if constexpr (E16 > 0) {
#pragma unroll
      for (int k = 0; k < E16; ++k) sI[k] = ldg4(G.si + ic * E + E4 * q + 4 * k);
    }
    bI = G.b[ic];
    stage_forward_store(s_w, s_b, wv, wdst, bv);
    if (threadIdx.x < kN2) s_w3[threadIdx.x] = w3v;
    if (threadIdx.x < kHeadFloats) s_hd[threadIdx.x] = threadIdx.x < 4 ? hv : 0.0f;
  }
  float* const orow = G.out + item;
  const bool store = q == 0 && item < G.ni;
  for (int64_t ut = blockIdx.y; ut < G.utiles; ut += gridDim.y) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    __syncthreads();                                  // the previous tile's rows are read
    {
      // the tile's rows, coalesced: every request before the first LDS store
      auto user_of = [&](int row) { return grid_user(G.users, G.user0, G.nu, r0, cnt, row); };
      f32x4 vz[kStagePasses], vs;
      float va = 0.0f;
#pragma unroll
      for (int e = 0; e < kStagePasses; ++e) {
        const int row = (threadIdx.x >> 6) + e * (kThreads / 64);
        vz[e] = ldg4(G.zu + user_of(row) * kN0 + 4 * (threadIdx.x & 63));
      }
      constexpr int S4 = E16 > 0 ? E4 : 1;              // (Wide & Deep stages no SU row)
      const int srow = threadIdx.x / S4, spiece = threadIdx.x % S4;
      const bool smine = E16 > 0 && threadIdx.x < kUT * E4;
      if constexpr (E16 > 0) vs = ldg4(G.su + user_of(smine ? srow : 0) * E + 4 * (smine ? spiece : 0));
      if (threadIdx.x < kUT) va = G.a[user_of(threadIdx.x)];
#pragma unroll
      for (int e = 0; e < kStagePasses; ++e) {
        const int row = (threadIdx.x >> 6) + e * (kThreads / 64);
        *reinterpret_cast<f32x4*>(s_zu + row * kN0 + 4 * (threadIdx.x & 63)) = vz[e];
      }
      if constexpr (E16 > 0) {
        if (smine) *reinterpret_cast<f32x4*>(s_su + srow * E + 4 * spiece) = vs;
      }
      if (threadIdx.x < kUT) s_a[threadIdx.x] = va;
    }
    __syncthreads();                                  // (the first tile: the weights and the head as well)
    const float b3 = s_hd[0], o0 = s_hd[1], o1 = s_hd[2], ob = s_hd[3];
    for (int r = 0; r < cnt; ++r) {
      f32x4 a0[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const f32x4 z = zI[j] + *reinterpret_cast<const f32x4*>(s_zu + r * kN0 + 16 * j + 4 * q);
#pragma unroll
        for (int c = 0; c < 4; ++c) a0[j][c] = fmaxf(z[c], 0.0f);
      }
      // FM cross term: the four lanes of an item hold E/4 terms each
      float dfm = 0.0f;
      if constexpr (E16 > 0) {
#pragma unroll
        for (int k = 0; k < E16; ++k) {
          const f32x4 s = *reinterpret_cast<const f32x4*>(s_su + r * E + E4 * q + 4 * k);
          dfm = fmaf(sI[k][0], s[0], dfm); dfm = fmaf(sI[k][1], s[1], dfm);
          dfm = fmaf(sI[k][2], s[2], dfm); dfm = fmaf(sI[k][3], s[3], dfm);
        }
      }
      const float au = s_a[r];
      f32x4 y[8];
      layer_fwd<0, 16>(s_w, s_b, lane, q, a0, y);
      float d3 = 0.0f;
#pragma unroll
      for (int bk = 0; bk < 8; ++bk) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(s_w3 + 16 * bk + 4 * q);
        d3 = fmaf(y[bk][0], wv[0], d3); d3 = fmaf(y[bk][1], wv[1], d3);
        d3 = fmaf(y[bk][2], wv[2], d3); d3 = fmaf(y[bk][3], wv[3], d3);
      }
      const float h3 = fmaxf(column_sum(d3) + b3, 0.0f);
      float fm = au + bI;
      if constexpr (E16 > 0) fm += column_sum(dfm);
      if (store) orow[(r0 + r) * G.ldo] = ctr_sigmoid(fmaf(o0, fm, fmaf(o1, h3, ob)));   // (the four lanes of an item agree)
    }
  }
}

// grid_row_blocks charges the weight prologue as 1/32 of a user tile: 10^4 cycles against kUT x 2 x 16 384
constexpr int kTilesPerPrologue = 32;
constexpr void (*kKernels[8])(const Tower, const Grid) = {   // by E / 16
    deepfm_grid_scores_kernel<1>, deepfm_grid_scores_kernel<2>, deepfm_grid_scores_kernel<3>, deepfm_grid_scores_kernel<4>,
    deepfm_grid_scores_kernel<5>, deepfm_grid_scores_kernel<6>, deepfm_grid_scores_kernel<7>, deepfm_grid_scores_kernel<8>};


// the launch behind both entries: `embed` 0 is Wide & Deep
int launch(const float* zu, const float* zi, const float* su, const float* si, const float* a, const float* b,
           int64_t num_users, int64_t num_items, int embed, const float* w2, const float* b2, const float* w3,
           const float* b3, const float* out_w, const float* out_b, const int64_t* users, int64_t user0, int64_t rows,
           float* out, int64_t ldo, int row_blocks, void* stream) {
  Tower T;
  T.w[0] = w2; T.b[0] = b2; T.y[0] = nullptr; T.ldy[0] = 0;
  const int64_t utiles = ctr_ceil_div(rows, kUT), xtiles = ctr_ceil_div(num_items, kItems);
  const int64_t y = row_blocks > 0 ? row_blocks : grid_row_blocks(xtiles, utiles, kTilesPerPrologue);
  const Grid G{zu, zi, su, si, a, b, w3, b3, out_w, out_b, users, user0, rows, num_users, num_items, out, ldo, utiles};
  // item tiles along x (neighbouring workgroups share their user tile's rows in L2), row blocks along y
  return grid_launch(embed ? kKernels[embed / 16 - 1] : deepfm_grid_scores_kernel<0>,
                     dim3((unsigned)xtiles, grid_clamp_y(y, utiles)), kThreads,
                     sizeof(float) * (size_t)lds_floats(embed), stream, T, G);
}

}  // namespace

extern "C" int ctr_deepfm_grid_scores(const float* zu, const float* zi, const float* su, const float* si, const float* a,
                                      const float* b, int64_t num_users, int64_t num_items, int embed, int n1, int n2,
                                      const float* w2, const float* b2, const float* w3, const float* b3,
                                      const float* out_w, const float* out_b, const int64_t* users, int64_t user0,
                                      int64_t rows, float* out, int64_t ldo, int row_blocks, void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && row_blocks >= 0, CTR_EINVAL);
  CTR_REQUIRE(zu && zi && su && si && a && b && w2 && b2 && w3 && b3 && out_w && out_b, CTR_EINVAL);
  if (n1 != kN0 || n2 != kN2 || embed < 16 || embed > 128 || embed % 16 != 0) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  if (!ctr_aligned16(zu) || !ctr_aligned16(zi) || !ctr_aligned16(su) || !ctr_aligned16(si) || !ctr_aligned16(w2))
    return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  return launch(zu, zi, su, si, a, b, num_users, num_items, embed, w2, b2, w3, b3, out_w, out_b, users, user0, rows, out,
                ldo, row_blocks, stream);
}

// Wide & Deep: the same kernel template without the FM dot (model/widedeep.py)
extern "C" int ctr_widedeep_grid_scores(const float* zu, const float* zi, const float* a, const float* b,
                                        int64_t num_users, int64_t num_items, int n1, int n2, const float* w2,
                                        const float* b2, const float* w3, const float* b3, const float* out_w,
                                        const float* out_b, const int64_t* users, int64_t user0, int64_t rows,
                                        float* out, int64_t ldo, int row_blocks, void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && row_blocks >= 0, CTR_EINVAL);
  CTR_REQUIRE(zu && zi && a && b && w2 && b2 && w3 && b3 && out_w && out_b, CTR_EINVAL);
  if (n1 != kN0 || n2 != kN2) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  if (!ctr_aligned16(zu) || !ctr_aligned16(zi) || !ctr_aligned16(w2)) return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  return launch(zu, zi, nullptr, nullptr, a, b, num_users, num_items, 0, w2, b2, w3, b3, out_w, out_b, users, user0, rows,
                out, ldo, row_blocks, stream);
}
