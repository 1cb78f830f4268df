// PNN (inner mode, six fields) over the whole user x item GRID: scores of `rows` users against every item, in one launch,
// with no feature matrix, no embedding row and no product row anywhere (ctr_pnn_grid_scores; model/pnn.py
// catalogue_scorer).
//
// The product layer's output h0 has no activation in front of the first DNN layer D1, every field vector belongs to the
// user (fields 0, 2, 3, 4) or to the item (1, 5), and of the 15 inner products 6 are the user's alone, 1 the item's alone
// and 8 cross the sides, so on a grid the model splits exactly:
//     z1[u, i] = ZU[u] + ZI[i] + G d(u, i)             (ZU / ZI: D1 of a side's part of h0, 128 wide; G = D1 W2[:, cross],
//                                                       128 x 8; d: the eight cross dots <f_a(u), f_b(i)> of length E)
//     out[u, i] = sigmoid(o . relu(D3 relu(D2 relu(z1) + c2) + c3) + ob)
// The walk is deepfm_grid.hip's: a wave owns sixteen consecutive items; lane (q, n) loads, ONCE, the operand-layout
// pieces of ZI[i0 + n] (columns 16b + 4q .., 32 registers) and its sixteen elements of G.  The workgroup stages ZU[u] of
// kUT = 16 users in LDS (coalesced).  Per user tile a wave then
//   1. forms the dots of its 16 users x 16 items on the matrix cores, eight accumulator tiles (one per cross column),
//      walking E in chunks of sixteen: lane (q, m) loads 16 bytes (elements 16k + 4q ..) of each of the four user-side
//      vectors of the tile's user m (A operands) and of the two item-side vectors of item n (B operands) from L2 -- a
//      chunk ahead of its use, nothing of FU or FI is staged or kept: E floats a lane would be 256 registers at E = 256
//      -- and issues 8 x 4 v_mfma_f32_16x16x4_f32.  A dot is accumulated in ascending chunks by the same instructions
//      whatever the tile: a function of its two rows alone.  The tiles come out user-major (lane (q, n): users 4q ..
//      4q + 3 of item n) and go through the wave's own LDS slab (no barrier: a wave's LDS operations keep their order),
//      from which step 2 reads, per user, the two columns lane (q, n) feeds to the K = 8 product:
//          q = 0: user.item, item.age   q = 1: item.gender, item.occupation   q = 2: user.movie, age.movie
//          q = 3: gender.movie, occupation.movie
//   2. walks the users: z1 = (ZI + ZU) + G d is two v_mfma_f32_16x16x4_f32 per sixteen output rows (K = 8) on top of the
//      sum of the rows, relu, then mfma16_tower.inc's layer_fwd twice (128 -> 64: 128 products, 64 -> 32: 32), the
//      32-term output dot reduced over the four lanes of a column, sigmoid, one store of sixteen scores.
// Items past num_items: loads clamped to the last row, stores masked; users past the tile's count repeat its last user.
// No atomics, no scratch, and no order dependence between pairs: a score is a function of its user's rows, its item's
// rows and the weights alone (a matrix-core column is computed from that column's operands only, a row from that row's),
// so the output is bitwise the same for any user list, row range, item order or launch geometry.
//
// Budget: LDS = D2 32 KiB + D3 8 KiB in operand order, 96 biases, 48 head floats, the user tile's ZU 8 KiB and the dot
// slabs (8 waves x 8 columns x 336 floats = 84 KiB): 132.6 KiB of the CU's 160 KiB at every E, so ONE workgroup per CU;
// eight waves, two per SIMD (amdgpu_waves_per_eu(2, 2): up to 256 registers a lane).  A sixteen-pair group is 176
// matrix products in step 2 and E / 8 in step 1 (2 at E = 16, 32 at E = 256): 5696 .. 6656 matrix-core issue cycles of
// its SIMD.  As in deepfm_grid.hip a user tile does NOT get a workgroup of its own: gridDim.y is chosen so that the
// grid is a small multiple of the CU count (grid_host.h, grid_row_blocks).
#include "grid_host.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 2;                          // the layers on the matrix cores behind z1
constexpr int kK[kL] = {128, 64};
constexpr int kN[kL] = {64, 32};
constexpr int kN1 = 128;                       // width of a ZU / ZI row = rows of G
constexpr int kN3 = 32;                        // width of h3 = the output dot
constexpr int kCross = 8;                      // cross columns = columns of G
constexpr int kUT = CTR_PNN_GRID_USER_TILE;    // users of a user tile
constexpr int kItems = CTR_PNN_GRID_ITEM_TILE; // items of a workgroup
constexpr int kMaxE = 256;
static_assert(kItems == 16 * kWaves, "a wave owns sixteen items");
static_assert(kUT == 16, "a user tile is the sixteen rows of a matrix-core tile");

#include "mfma16_tower.inc"
#include "grid_frame.inc"

constexpr int kHeadFloats = 48;                // the 32 output weights, the output bias, pad
constexpr int kFixedFloats = kWFloats + kBFloats + kHeadFloats;
// a wave's dot slab: [column slot][user][item], user rows kTS = 20 floats apart (a store's quarters q, q + 1 of a
// 32-lane half are 80 floats = 16 banks of the 32 apart), column slots 16 kTS + 16 apart (so are the quarters of a
// load, which read neighbouring slots: kSlabSlot below)
constexpr int kColFloats = 16 * kTS + 16;
constexpr int kSlabFloats = kCross * kColFloats;
constexpr int kLdsFloats = kFixedFloats + kUT * kN1 + kWaves * kSlabFloats;
static_assert(sizeof(float) * kLdsFloats <= 160 * 1024, "fits the CU's LDS");
static_assert(kUT * (kN1 / 4) == kThreads, "ZU staging: one 16-byte piece a thread");

struct Grid {
  const float* zu; const float* zi;            // (nu, 128), (ni, 128)
  const float* fu; const float* fi;            // (nu, 4E): user, age, gender, occupation; (ni, 2E): item, movie
  const float* g;                              // (128, 8): columns in the order of the cross pairs
  const float* ow; const float* ob;            // the output layer: 32 weights, 1 bias
  const int64_t* users; int64_t user0;         // the users of the rows: users[r], or user0 + r
  int64_t rows, nu, ni;
  float* out; int64_t ldo;
  int64_t utiles;
  int embed;
};

// The cross columns in the order of G's columns (= of allpairs): user.item, user.movie, item.age, item.gender,
// item.occupation, age.movie, gender.movie, occupation.movie, as (slot of fu, slot of fi)
constexpr int kColU[kCross] = {0, 0, 1, 2, 3, 1, 2, 3};
constexpr int kColI[kCross] = {0, 1, 0, 0, 0, 1, 1, 1};
// column of quarter q's K = 8 matrix-core call t: user-side slot 2 (q & 1) + t against item-side slot q >> 1
__device__ __forceinline__ int cross_column(int q, int t) {
  const int us = 2 * (q & 1) + t;              // 0 user, 1 age, 2 gender, 3 occupation
  return (q >> 1) == 0 ? (us == 0 ? 0 : us + 1) : (us == 0 ? 1 : us + 4);
}
// where a column's tile sits in the slab: cross_column(q, t) at 4t + q, so that the two quarters of a 32-lane half
// read tiles an odd number of kColFloats (= 16 mod 32 banks) apart
constexpr int kSlabSlot[kCross] = {0, 2, 4, 1, 5, 6, 3, 7};

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
pnn_grid_scores_kernel(const Tower T, const Grid G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = G.embed;
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_hd = s_b + kBFloats;                       // kHeadFloats
  float* s_zu = s_hd + kHeadFloats;                   // kUT x 128: ZU rows of the user tile
  float* s_d = s_zu + kUT * kN1;                      // kWaves x kSlabFloats: the waves' dots
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: the layers' weights, the head, this lane's pieces of its item's ZI row and of G
  f32x4 zI[8];
  float g0[8], g1[8];
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
    const float hv = threadIdx.x < kN3 ? G.ow[threadIdx.x] : *G.ob;
    const int c0 = cross_column(q, 0), c1 = cross_column(q, 1);
#pragma unroll
    for (int b = 0; b < 8; ++b) zI[b] = ldg4(G.zi + ic * kN1 + 16 * b + 4 * q);
#pragma unroll
    for (int b = 0; b < 8; ++b) {                     // A operands of the K = 8 product: lane (q, m) holds G[16b + m][column]
      g0[b] = G.g[(16 * b + n) * kCross + c0];
      g1[b] = G.g[(16 * b + n) * kCross + c1];
    }
    stage_forward_store(s_w, s_b, wv, wdst, bv);
    if (threadIdx.x < kHeadFloats) s_hd[threadIdx.x] = threadIdx.x <= kN3 ? hv : 0.0f;
  }
  const float* fi_row = G.fi + ic * (2 * (int64_t)E) + 4 * q;   // B operands: this lane's quarter of its item's chunks
  float* const slab = s_d + wave * kSlabFloats;
  float* const put = slab + 4 * q * kTS + n;                     // tile element (user 4q + r, item n) of column c: + kSlabSlot[c] kColFloats + r kTS
  const float* const get0 = slab + q * kColFloats + n;           // + r kTS: this lane's B operands of user r
  const float* const get1 = slab + (4 + q) * kColFloats + n;
  float* const orow = G.out + item;
  const bool store = q == 0 && item < G.ni;
  for (int64_t ut = blockIdx.y; ut < G.utiles; ut += gridDim.y) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    // rows past cnt repeat the tile's last user: read, multiplied, never stored
    auto user_of = [&](int row) { return grid_user(G.users, G.user0, G.nu, r0, cnt, row); };
    __syncthreads();                                  // the previous tile's rows are read
    // the tile's ZU rows, coalesced: requested here, stored behind step 1
    const f32x4 vz = ldg4(G.zu + user_of(threadIdx.x >> 5) * kN1 + 4 * (threadIdx.x & 31));
    // ---- 1. the eight dot tiles of the tile's users x this wave's items
    {
      const float* fu_row = G.fu + user_of(n) * (4 * (int64_t)E) + 4 * q;   // A operands: lane (q, m) reads user m's chunks
      f32x4 acc[kCross];
#pragma unroll
      for (int c = 0; c < kCross; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 a[4], b[2];
#pragma unroll
      for (int s = 0; s < 4; ++s) a[s] = ldg4(fu_row + s * E);
#pragma unroll
      for (int s = 0; s < 2; ++s) b[s] = ldg4(fi_row + s * E);
      for (int k = 16; k <= E; k += 16) {
        f32x4 an[4], bn[2];
        const int kn = k < E ? k : 0;                 // (the last round re-reads the first chunk and drops it)
#pragma unroll
        for (int s = 0; s < 4; ++s) an[s] = ldg4(fu_row + s * E + kn);
#pragma unroll
        for (int s = 0; s < 2; ++s) bn[s] = ldg4(fi_row + s * E + kn);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int c = 0; c < kCross; ++c)
            acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kColU[c]][e], b[kColI[c]][e], acc[c], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = an[s];
#pragma unroll
        for (int s = 0; s < 2; ++s) b[s] = bn[s];
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int c = 0; c < kCross; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) put[kSlabSlot[c] * kColFloats + r * kTS] = acc[c][r];
      asm volatile("" ::: "memory");                  // the loads of step 2 stay behind these stores
    }
    *reinterpret_cast<f32x4*>(s_zu + 4 * threadIdx.x) = vz;
    __syncthreads();                                  // the ZU rows (the first tile: the weights and the head as well)
    // ---- 2. the users of the tile
    for (int r = 0; r < cnt; ++r) {
      const float d0 = get0[r * kTS], d1 = get1[r * kTS];
      f32x4 a0[8];
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        f32x4 z = zI[b] + *reinterpret_cast<const f32x4*>(s_zu + r * kN1 + 16 * b + 4 * q);
        z = __builtin_amdgcn_mfma_f32_16x16x4f32(g0[b], d0, z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f32_16x16x4f32(g1[b], d1, z, 0, 0, 0);
#pragma unroll
        for (int c = 0; c < 4; ++c) a0[b][c] = fmaxf(z[c], 0.0f);
      }
      f32x4 y2[4], y3[2];
      layer_fwd<0, 8>(s_w, s_b, lane, q, a0, y2);
      layer_fwd<1, 4>(s_w, s_b, lane, q, y2, y3);
      float dot = 0.0f;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(s_hd + 16 * b + 4 * q);
        dot = fmaf(y3[b][0], wv[0], dot); dot = fmaf(y3[b][1], wv[1], dot);
        dot = fmaf(y3[b][2], wv[2], dot); dot = fmaf(y3[b][3], wv[3], dot);
      }
      dot = column_sum(dot);
      if (store) orow[(r0 + r) * G.ldo] = ctr_sigmoid(dot + s_hd[kN3]);   // (the four lanes of an item agree)
    }
  }
}

// grid_row_blocks charges the weight prologue as 1/16 of a user tile: 10^4 cycles against kUT x 2 x 5696
constexpr int kTilesPerPrologue = 16;

}  // namespace

extern "C" int ctr_pnn_grid_scores(const float* zu, const float* zi, const float* fu, const float* fi, const float* g,
                                   int64_t num_users, int64_t num_items, int embed, int n1, int n2, int n3,
                                   const float* d2_w, const float* d2_b, const float* d3_w, const float* d3_b,
                                   const float* out_w, const float* out_b, const int64_t* users, int64_t user0,
                                   int64_t rows, float* out, int64_t ldo, int row_blocks, void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && row_blocks >= 0, CTR_EINVAL);
  CTR_REQUIRE(zu && zi && fu && fi && g && d2_w && d2_b && d3_w && d3_b && out_w && out_b, CTR_EINVAL);
  if (n1 != kN1 || n2 != kN[0] || n3 != kN3 || embed < 16 || embed > kMaxE || embed % 16 != 0) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  if (!ctr_aligned16(zu) || !ctr_aligned16(zi) || !ctr_aligned16(fu) || !ctr_aligned16(fi) || !ctr_aligned16(d2_w) ||
      !ctr_aligned16(d3_w))
    return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  Tower T;
  T.w[0] = d2_w; T.b[0] = d2_b; T.y[0] = nullptr; T.ldy[0] = 0;
  T.w[1] = d3_w; T.b[1] = d3_b; T.y[1] = nullptr; T.ldy[1] = 0;
  const int64_t utiles = ctr_ceil_div(rows, kUT), xtiles = ctr_ceil_div(num_items, kItems);
  const int64_t y = row_blocks > 0 ? row_blocks : grid_row_blocks(xtiles, utiles, kTilesPerPrologue);
  const Grid G{zu, zi, fu, fi, g, out_w, out_b, users, user0, rows, num_users, num_items, out, ldo, utiles, embed};
  // item tiles along x (neighbouring workgroups share their user tile's rows in L2), row blocks along y
  return grid_launch(pnn_grid_scores_kernel, dim3((unsigned)xtiles, grid_clamp_y(y, utiles)), kThreads,
                     sizeof(float) * (size_t)kLdsFloats, stream, T, G);
}
