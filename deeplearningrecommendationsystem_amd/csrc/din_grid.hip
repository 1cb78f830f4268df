// DIN over the whole history x item GRID: the attention-pooled history of `rows` history rows against every item, in one
// launch, with no id tensor and no per-position tensor (ctr_din_grid_pool; model/din.py score_histories / recommend).
//
// The per-sample forward (din.hip, DIN.run_forward) gathers a row's L history rows once per (row, item) pair, writes
// the attention operand and both attention activations for every (pair, position), and reads them back for a softmax
// kernel.  On the grid the first attention layer splits into a part of the history position and a part of the item
// (W1 = [Wa | Wb | Wc] over [h, h - t, t]):
//     AH[l] = (Wa + Wb) table[hist[r, l]]          AT[i] = (Wc - Wb) table[i] + b1          (both 128 wide, made by the caller)
//     s[l]  = w3 . relu(W2 relu(AH[l] + AT[i]) + b2)       a = softmax_l(s)       pooled[r, i] = sum_l a[l] table[hist[r, l]]
// (the score layer's bias shifts every s[l] of a pair alike and drops out of the softmax).  The walk is the one of
// ncf_grid.hip: a wave owns sixteen consecutive items; lane (q, n) loads, ONCE, the operand-layout pieces of AT[i0 + n]
// (columns 16j + 4q .., 32 registers).  The workgroup stages blocks of kPB history positions in LDS -- the position's
// AH row and its table row, 768 bytes, coalesced -- and the waves walk them: the position's pieces are LDS broadcasts
// (the sixteen lanes of a quarter read one address), a0 = relu(AT + AH[l]), ONE layer_fwd (128 products), the w3 dot
// over the four lanes of a column, and an online softmax: running maximum, running denominator and the lane's sixteen
// columns of the weighted sum, rescaled when the maximum moves.  The state resets at every multiple of L; the column's
// 64 values are stored once, after the row's last position.  Items past num_items: loads clamped to the last row,
// stores masked.  A history id outside the table raises *err_flag and is read as row 0 (din.hip's safe_row).
// No atomics and no order dependence between pairs: a pair's row is a function of its history row, its item's AT row
// and the weights alone, so the output is bitwise the same for any subset, order or repetition of history rows and for
// any item order.
//
// Cost: 128 v_mfma_f32_16x16x4_f32 per position and sixteen pairs (16384 flop a pair and position), 4096 issue cycles
// per SIMD; the weight prologue (32 KiB) is paid once per workgroup, which walks several row tiles.
#include "grid_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 1;                          // the layer behind the split one
constexpr int kK[kL] = {128};
constexpr int kN[kL] = {64};
constexpr int kN1 = 128;                       // width of an AH / AT row
constexpr int kE = 64;                         // embedding width
constexpr int kPB = 32;                        // history positions of a staged block: 24 KiB
constexpr int kRT = 4;                         // history rows of a row tile (the unit handed out along gridDim.y)
constexpr int kItems = 16 * kWaves;            // items of a workgroup

#include "mfma16_tower.inc"
#include "grid_frame.inc"

constexpr int kLdsFloats = kWFloats + kBFloats + kN[0] + kPB * (kN1 + kE);
static_assert((kPB * (kN1 / 4)) % kThreads == 0 && (kPB * (kE / 4)) % kThreads == 0,
              "staging: whole passes of the workgroup over the block's 16-byte pieces");
constexpr int kAhPasses = kPB * (kN1 / 4) / kThreads;   // 4
constexpr int kHPasses = kPB * (kE / 4) / kThreads;     // 2

struct Pool {
  const float* table;                          // (ni, 64)
  const float* at;                             // (ni, 128)
  const float* ah; int ah_by_position;         // (ni, 128) read by history id, or (rows * len, 128) read by position
  const float* w3;                             // 64
  const int64_t* hist;                         // (rows, len)
  int64_t rows, ni; int len;
  float* out; int64_t ldo;
  int32_t* err;
  int64_t tiles;
};

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
din_grid_pool_kernel(const Tower T, const Pool G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_w3 = s_b + kBFloats;                       // 64
  float* s_ah = s_w3 + kN[0];                         // kPB x 128: AH rows of the position block
  float* s_h = s_ah + kPB * kN1;                      // kPB x 64: table rows of the position block
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: the layer's weights, the score weights, this lane's pieces of its item's AT row
  f32x4 aT[8];
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
    const float w3v = G.w3[threadIdx.x & (kN[0] - 1)];
#pragma unroll
    for (int j = 0; j < 8; ++j) aT[j] = ldg4(G.at + ic * kN1 + 16 * j + 4 * q);
    stage_forward_store(s_w, s_b, wv, wdst, bv);
    if (threadIdx.x < kN[0]) s_w3[threadIdx.x] = w3v;
  }
  const bool store = item < G.ni;
  for (int64_t tile = blockIdx.y; tile < G.tiles; tile += gridDim.y) {
    const int64_t r0 = tile * kRT;
    const int64_t npos = (G.rows - r0 < kRT ? G.rows - r0 : kRT) * G.len;
    const int64_t flat0 = r0 * G.len;                 // hist is row-major: the tile's positions are consecutive
    int64_t r = r0;
    int l = 0;
    float mx = -INFINITY, den = 0.0f;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t p0 = 0; p0 < npos; p0 += kPB) {
      const int cnt = (int)(npos - p0 < kPB ? npos - p0 : kPB);
      __syncthreads();                                // the previous block's rows are read
      {
        // the block's rows, 32 / 16 lanes a row: every request before the first LDS store
        f32x4 va[kAhPasses], vh[kHPasses];
#pragma unroll
        for (int e = 0; e < kAhPasses; ++e) {
          const int pos = (threadIdx.x >> 5) + e * (kThreads / 32);
          const int64_t flat = flat0 + p0 + (pos < cnt ? pos : cnt - 1);
          int64_t id = G.hist[flat];
          if (id < 0 || id >= G.ni) {
            if (G.err) *G.err = 1;
            id = 0;
          }
          va[e] = ldg4(G.ah + (G.ah_by_position ? flat : id) * kN1 + 4 * (threadIdx.x & 31));
        }
#pragma unroll
        for (int e = 0; e < kHPasses; ++e) {
          const int pos = (threadIdx.x >> 4) + e * (kThreads / 16);
          int64_t id = G.hist[flat0 + p0 + (pos < cnt ? pos : cnt - 1)];
          id = id < 0 || id >= G.ni ? 0 : id;
          vh[e] = ldg4(G.table + id * kE + 4 * (threadIdx.x & 15));
        }
#pragma unroll
        for (int e = 0; e < kAhPasses; ++e)
          *reinterpret_cast<f32x4*>(s_ah + ((threadIdx.x >> 5) + e * (kThreads / 32)) * kN1 + 4 * (threadIdx.x & 31)) = va[e];
#pragma unroll
        for (int e = 0; e < kHPasses; ++e)
          *reinterpret_cast<f32x4*>(s_h + ((threadIdx.x >> 4) + e * (kThreads / 16)) * kE + 4 * (threadIdx.x & 15)) = vh[e];
      }
      __syncthreads();                                // (the first block: the weights as well)
      // the position's AH pieces are read one position ahead of the products that consume them
      f32x4 aH[8];
      auto fetch = [&](int p) {
#pragma unroll
        for (int j = 0; j < 8; ++j) aH[j] = *reinterpret_cast<const f32x4*>(s_ah + p * kN1 + 16 * j + 4 * q);
      };
      fetch(0);
      for (int p = 0; p < cnt; ++p) {
        f32x4 a0[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const f32x4 z = aT[j] + aH[j];
#pragma unroll
          for (int c = 0; c < 4; ++c) a0[j][c] = fmaxf(z[c], 0.0f);
        }
        fetch(p + 1 < cnt ? p + 1 : p);
        f32x4 y[4];
        layer_fwd<0, 8>(s_w, s_b, lane, q, a0, y);
        // the score: lane (q, n) holds units 16b + 4q + c of column n
        float s = 0.0f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(s_w3 + 16 * b + 4 * q);
          s = fmaf(y[b][0], wv[0], s); s = fmaf(y[b][1], wv[1], s);
          s = fmaf(y[b][2], wv[2], s); s = fmaf(y[b][3], wv[3], s);
        }
        s = column_sum(s);                            // (the four lanes of a column agree, bitwise)
        // online softmax over the row's positions; this lane's columns 16q .. 16q + 15 of the weighted sum
        const float mnew = fmaxf(mx, s);
        const float scale = expf(mx - mnew), ev = expf(s - mnew);
        mx = mnew;
        den = fmaf(den, scale, ev);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(s_h + p * kE + 16 * q + 4 * i);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[i][c] = fmaf(acc[i][c], scale, ev * h[c]);
        }
        if (++l == G.len) {                           // (uniform over the workgroup)
          if (store) {
            const float inv = 1.0f / den;
            float* dst = G.out + (r * G.ni + item) * G.ldo + 16 * q;
#pragma unroll
            for (int i = 0; i < 4; ++i) stg4(dst + 4 * i, acc[i] * inv);
          }
          ++r;
          l = 0;
          mx = -INFINITY;
          den = 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }
}

}  // namespace

extern "C" int ctr_din_grid_pool(const float* table, int64_t num_items, int embed, const float* at, const float* ah,
                                 int ah_by_position, const float* w2, const float* b2, const float* w3, int n1, int n2,
                                 const int64_t* hist, int64_t rows, int len, float* out, int64_t ldo, int32_t* err_flag,
                                 void* stream) {
  CTR_REQUIRE(rows >= 0 && num_items >= 0 && len >= 1, CTR_EINVAL);
  CTR_REQUIRE(table && at && ah && w2 && b2 && w3, CTR_EINVAL);
  CTR_REQUIRE(embed == kE && n1 == kN1 && n2 == kN[0], CTR_EINVAL);
  CTR_REQUIRE(num_items < ((int64_t)1 << 31), CTR_EINVAL);
  CTR_REQUIRE(ldo >= kE && ldo % 4 == 0, CTR_EINVAL);
  CTR_REQUIRE((hist && out) || rows == 0 || num_items == 0, CTR_EINVAL);
  CTR_REQUIRE(ctr_aligned16(table) && ctr_aligned16(at) && ctr_aligned16(ah) && ctr_aligned16(w2) && ctr_aligned16(out),
              CTR_EINVAL);
  if (rows == 0 || num_items == 0) return CTR_OK;
  Tower T;
  T.w[0] = w2; T.b[0] = b2; T.y[0] = nullptr; T.ldy[0] = 0;
  const int64_t tiles = ctr_ceil_div(rows, kRT);
  const Pool G{table, at, ah, ah_by_position != 0, w3, hist, rows, num_items, len, out, ldo, err_flag, tiles};
  // item tiles along x (neighbouring workgroups share their position block's rows in L2), row tiles along y
  const int64_t gx = ctr_ceil_div(num_items, kItems);
  return grid_launch(din_grid_pool_kernel, dim3((unsigned)gx, grid_history_y(gx, tiles)), kThreads,
                     sizeof(float) * (size_t)kLdsFloats, stream, T, G);
}
