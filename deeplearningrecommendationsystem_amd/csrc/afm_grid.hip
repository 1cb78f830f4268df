// AFM (six fields) over the whole user x item GRID: scores of `rows` users against every item, in one launch, with no
// feature matrix, no pair-product row and no hidden row anywhere (ctr_afm_grid_scores; model/afm.py catalogue_scorer).
//
// Per product p = f_a * f_b (elementwise, E wide) the model needs two numbers, the attention logit s(p) = h . relu(W^T p
// + b_att) and t(p) = o . p, because output_layer(sum_k w_k p_k) = sum_k w_k t(p_k) + ob with w = softmax_k s(p_k).  Of
// the 15 products 6 are the user's alone, 1 the item's alone and 8 cross the sides (PNN's columns), so on a grid the
// model splits exactly:
//     user u:  a[u] (wide part), the softmax summary of its six own products (mU = max s, dU = sum exp(s - mU),
//              nU = sum exp(s - mU) t) -- su (U, 4) -- and its field vectors FU[u] (4E: user, age, gender, occupation)
//     item i:  b[i] (wide part, every bias), (sI, tI) of its one own product -- si (I, 3) -- and FI[i] (2E: item, movie)
//     pair:    (s_c, t_c) of the eight cross products FU_a[u] * FI_b[i]; the running softmax (m, d, n) starts at the
//              user's summary, takes the item's term and the eight cross terms one at a time
//                  m' = max(m, s);  d = d exp(m - m') + exp(s - m');  n = n exp(m - m') + exp(s - m') t
//              (no term is ever exponentiated above 0: logits of any size);  out = sigmoid(a + b + n / d)
// The walk is deepfm_grid.hip's / pnn_grid.hip's: a workgroup of eight waves covers 128 items, a wave owns sixteen.
// Lane (q, n) loads, ONCE, the elements 16j + 4q + c of the two FI vectors of item i0 + n (E / 2 registers) -- the B
// operand positions of a 16x16x4 product whose K walks E in mfma16_tower.inc's order -- and the item's three scalars.
// W^T sits in LDS in that file's operand order ([out block][in block][lane][chunk], 64E floats; staged here from the
// (E, 64) parameter as it is stored, so the caller makes no transposed copy), b_att and h in registers (the lane's
// sixteen units 16b + 4q + r), o in LDS.  The workgroup stages the FU rows and the four scalars of kUT = 16 users; the
// next tile's pieces are requested before the current tile is computed and stored behind it.  Per user and per
// user-side slot a (a run-time loop of four; the two item-side vectors unrolled, so both columns share every weight
// read) the lane forms p = FU_a[k] * FI_b[k] in registers one sixteen-block at a time, accumulates its part of t_c from
// the same products and issues 2 x 4 x 4 v_mfma_f32_16x16x4_f32 per block: eight independent accumulator chains.
// Bias is the accumulators' initial value; relu, the dot with h, column_sum over the four lanes of an item, the merge.
// One masked store of sixteen scores per user.  The age columns go through the matrix cores like the others: the
// rank-one shortcut (W^T (age FI_b) = age W^T FI_b) was not built and not measured.
// Items past num_items: loads clamped to the last row, stores masked; only the tile's own users are walked.
// No atomics, no scratch, and no order dependence between pairs: a score is a function of its user's rows, its item's
// rows and the weights alone (a matrix-core column is computed from that column's operands only), so the output is
// bitwise the same for any user list, row range, item order or launch geometry.
//
// Budget (the kernel is a template over E / 16; figures for E = 16 / E = 128): LDS = W^T 4 / 32 KiB + the user tile's
// FU 4 / 32 KiB + o, the tile's scalars: 8.3 / 64.8 KiB of the CU's 160 KiB; eight waves, two per SIMD
// (amdgpu_waves_per_eu(2, 2)), so one workgroup per CU.  `make asm`: 134 / 212 VGPRs (the most: 248 at E = 96), no
// AGPRs, 0 scratch bytes at every E.  A sixteen-pair group is 8E matrix products = 32 x 8E issue cycles of its SIMD:
// 4096 / 32768.  As in deepfm_grid.hip a user tile does NOT get a workgroup of its own: gridDim.y is chosen so that the
// grid is a small multiple of the CU count (grid_host.h, grid_row_blocks).
#include "grid_host.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kAtt = 64;                       // attention units: four sixteen-unit output blocks
constexpr int kAB = kAtt / 16;
constexpr int kMaxE = 128;
// mfma16_tower.inc's shapes: the attention map at its widest.  Only its types and its operand ORDER are used here; its
// staging helpers take a compile-time input width, and E is this kernel's template parameter.
constexpr int kL = 1;
constexpr int kK[kL] = {kMaxE};
constexpr int kN[kL] = {kAtt};
constexpr int kUT = CTR_AFM_GRID_USER_TILE;    // users of a user tile
constexpr int kItems = CTR_AFM_GRID_ITEM_TILE; // items of a workgroup
static_assert(kItems == 16 * kWaves, "a wave owns sixteen items");
static_assert(kUT == 16, "a user tile holds as many 16-byte pieces as W");

#include "mfma16_tower.inc"
#include "grid_frame.inc"

struct Map {
  const float* w;                              // attention_W (E, 64)
  const float* b; const float* h;              // attention_b, attention_h: 64 each
  const float* o;                              // output_layer.weight: E
};

struct Grid {
  const float* su; const float* si;            // (nu, 4): a, mU, dU, nU; (ni, 3): b, sI, tI
  const float* fu; const float* fi;            // (nu, 4E): user, age, gender, occupation; (ni, 2E): item, movie
  const int64_t* users; int64_t user0;         // the users of the rows: users[r], or user0 + r
  int64_t rows, nu, ni;
  float* out; int64_t ldo;
  int64_t utiles;
};

constexpr int lds_floats(int E) { return kAtt * E + E + kUT * 4 * E + kUT * 4; }
static_assert(sizeof(float) * lds_floats(kMaxE) <= 160 * 1024, "fits the CU's LDS");

template <int JE>   // E = 16 JE
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
afm_grid_scores_kernel(const Map M, const Grid G) {
  constexpr int E = 16 * JE;
  constexpr int kPieces = 16 * E;                     // 16-byte pieces of W (E rows of 16) and of a user tile (kUT rows of E)
  constexpr int kPer = (kPieces + kThreads - 1) / kThreads;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_w = lds;                                   // 64 E: W^T in operand order
  float* s_o = s_w + kAtt * E;                        // E
  float* s_fu = s_o + E;                              // kUT x 4E: FU rows of the user tile
  float* s_su = s_fu + kUT * 4 * E;                   // kUT x 4: their scalars
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: W^T and o into LDS, this lane's pieces of its item's two vectors, its units of b_att and h
  f32x4 fi0[JE], fi1[JE], bias[kAB], hh[kAB];
#pragma unroll
  for (int j = 0; j < JE; ++j) {
    fi0[j] = ldg4(G.fi + ic * (2 * E) + 16 * j + 4 * q);
    fi1[j] = ldg4(G.fi + ic * (2 * E) + E + 16 * j + 4 * q);
  }
  const float bI = G.si[ic * 3], sI = G.si[ic * 3 + 1], tI = G.si[ic * 3 + 2];
#pragma unroll
  for (int b = 0; b < kAB; ++b)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bias[b][r] = M.b[16 * b + 4 * q + r];
      hh[b][r] = M.h[16 * b + 4 * q + r];
    }
  {
    // a 16-byte piece of row k of W (units 4 u4 ..) is chunk k & 3 of four neighbouring lanes of block (u4 >> 2, k >> 4)
    f32x4 wv[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = threadIdx.x + i * kThreads;
      wv[i] = ldg4(M.w + 4 * (p < kPieces ? p : 0));
    }
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = threadIdx.x + i * kThreads, k = p >> 4, u4 = p & 15;
      if (p < kPieces) {
        float* dst = s_w + (((u4 >> 2) * JE + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + 4 * (u4 & 3)) * 4 + (k & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[4 * e] = wv[i][e];
      }
    }
    if (threadIdx.x < E) s_o[threadIdx.x] = M.o[threadIdx.x];
  }
  float* const orow = G.out + item;
  const bool store = q == 0 && item < G.ni;
  // the FU rows and scalars of user tile `ut`, coalesced: requested a tile ahead, stored behind the barrier
  f32x4 pv[kPer], psv;
  auto tile_load = [&](int64_t ut) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = threadIdx.x + i * kThreads;       // piece p % E of row p / E (rows past cnt repeat the last user)
      const int row = p < kPieces ? p / E : 0, piece = p < kPieces ? p % E : 0;
      pv[i] = ldg4(G.fu + grid_user(G.users, G.user0, G.nu, r0, cnt, row) * (4 * E) + 4 * piece);
    }
    psv = ldg4(G.su + grid_user(G.users, G.user0, G.nu, r0, cnt, threadIdx.x & (kUT - 1)) * 4);
  };
  int64_t ut = blockIdx.y;
  if (ut < G.utiles) tile_load(ut);
  for (; ut < G.utiles; ut += gridDim.y) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    __syncthreads();                                  // the previous tile's rows are read
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int p = threadIdx.x + i * kThreads;
      if (p < kPieces) *reinterpret_cast<f32x4*>(s_fu + 4 * p) = pv[i];
    }
    if (threadIdx.x < kUT) *reinterpret_cast<f32x4*>(s_su + 4 * threadIdx.x) = psv;
    __syncthreads();                                  // the tile's rows (the first tile: W^T and o as well)
    if (ut + gridDim.y < G.utiles) tile_load(ut + gridDim.y);
    for (int r = 0; r < cnt; ++r) {
      const f32x4 us = *reinterpret_cast<const f32x4*>(s_su + 4 * r);   // a, mU, dU, nU
      float m = us[1], d = us[2], num = us[3];
      auto merge = [&](float s, float t) {
        const float mn = fmaxf(m, s), keep = __expf(m - mn), add = __expf(s - mn);
        d = fmaf(d, keep, add);
        num = fmaf(num, keep, add * t);
        m = mn;
      };
      merge(sI, tI);
#pragma unroll 1
      for (int a = 0; a < 4; ++a) {                   // user, age, gender, occupation against (item, movie)
        const float* fu = s_fu + (r * 4 + a) * E + 4 * q;
        const float* ov = s_o + 4 * q;
        const float* wbase = s_w + lane * 4;
        f32x4 acc0[kAB], acc1[kAB];
#pragma unroll
        for (int b = 0; b < kAB; ++b) acc0[b] = bias[b], acc1[b] = bias[b];
        float t0 = 0.0f, t1 = 0.0f;
        // (input block j, output block b) steps; the weight vector of step s + 2 is requested while step s multiplies,
        // the user's and o's pieces of block j + 1 while block j does (layer_fwd's schedule, for the same reason)
        constexpr int S = JE * kAB;
        auto wread = [&](int s) { return *reinterpret_cast<const f32x4*>(wbase + (((s % kAB) * JE + s / kAB) * 64) * 4); };
        f32x4 w0 = wread(0), w1 = wread(1);
        f32x4 un = *reinterpret_cast<const f32x4*>(fu), on = *reinterpret_cast<const f32x4*>(ov);
#pragma unroll
        for (int j = 0; j < JE; ++j) {
          const f32x4 p0 = un * fi0[j], p1 = un * fi1[j];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            t0 = fmaf(on[c], p0[c], t0);
            t1 = fmaf(on[c], p1[c], t1);
          }
          if (j + 1 < JE) {
            un = *reinterpret_cast<const f32x4*>(fu + 16 * (j + 1));
            on = *reinterpret_cast<const f32x4*>(ov + 16 * (j + 1));
          }
#pragma unroll
          for (int b = 0; b < kAB; ++b) {
            const int s = j * kAB + b;
            const f32x4 wa = w0;
            w0 = w1;
            if (s + 2 < S) w1 = wread(s + 2);
            asm volatile("" ::: "memory");            // later LDS reads stay behind this point
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              acc0[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[c], p0[c], acc0[b], 0, 0, 0);
              acc1[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[c], p1[c], acc1[b], 0, 0, 0);
            }
          }
        }
        float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int b = 0; b < kAB; ++b)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            s0 = fmaf(hh[b][c], fmaxf(acc0[b][c], 0.0f), s0);
            s1 = fmaf(hh[b][c], fmaxf(acc1[b][c], 0.0f), s1);
          }
        s0 = column_sum(s0); t0 = column_sum(t0);
        s1 = column_sum(s1); t1 = column_sum(t1);
        merge(s0, t0);
        merge(s1, t1);
      }
      if (store) orow[(r0 + r) * G.ldo] = ctr_sigmoid(us[0] + bI + num / d);   // (the four lanes of an item agree)
    }
  }
}

// grid_row_blocks charges the weight prologue as 1/16 of a user tile (pnn_grid.hip's figure: a tile here is no shorter
// at any E, 16 users x 2 waves x 32 x 8E cycles, and the prologue stages less)
constexpr int kTilesPerPrologue = 16;

template <int JE>
int launch(const Map& M, const Grid& G, dim3 grid, void* stream) {
  return grid_launch(afm_grid_scores_kernel<JE>, grid, kThreads, sizeof(float) * (size_t)lds_floats(16 * JE), stream, M, G);
}

}  // namespace

extern "C" int ctr_afm_grid_scores(const float* su, const float* si, const float* fu, const float* fi, int64_t num_users,
                                   int64_t num_items, int embed, int attention, const float* att_w, const float* att_b,
                                   const float* att_h, const float* out_w, const int64_t* users, int64_t user0,
                                   int64_t rows, float* out, int64_t ldo, int row_blocks, void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && row_blocks >= 0, CTR_EINVAL);
  CTR_REQUIRE(su && si && fu && fi && att_w && att_b && att_h && out_w, CTR_EINVAL);
  if (attention != kAtt || embed < 16 || embed > kMaxE || embed % 16 != 0) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  if (!ctr_aligned16(su) || !ctr_aligned16(fu) || !ctr_aligned16(fi) || !ctr_aligned16(att_w)) return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  const int64_t utiles = ctr_ceil_div(rows, kUT), xtiles = ctr_ceil_div(num_items, kItems);
  const int64_t y = row_blocks > 0 ? row_blocks : grid_row_blocks(xtiles, utiles, kTilesPerPrologue);
  const Map M{att_w, att_b, att_h, out_w};
  const Grid G{su, si, fu, fi, users, user0, rows, num_users, num_items, out, ldo, utiles};
  // item tiles along x (neighbouring workgroups share their user tile's rows in L2), row blocks along y
  const dim3 grid((unsigned)xtiles, grid_clamp_y(y, utiles));
  switch (embed / 16) {
    case 1: return launch<1>(M, G, grid, stream);
    case 2: return launch<2>(M, G, grid, stream);
    case 3: return launch<3>(M, G, grid, stream);
    case 4: return launch<4>(M, G, grid, stream);
    case 5: return launch<5>(M, G, grid, stream);
    case 6: return launch<6>(M, G, grid, stream);
    case 7: return launch<7>(M, G, grid, stream);
    default: return launch<8>(M, G, grid, stream);
  }
}
