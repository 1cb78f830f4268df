// DIEN over the whole history x item GRID: the last GRU state of `rows` history rows against every item, in one launch,
// with no id tensor and nothing written per history position (ctr_dien_grid_hidden; model/dien.py score_histories /
// recommend).
//
// The per-sample forward (DIEN.run_forward) writes, for every (pair, position), the [h, t] operand, both attention
// activations, the weighted sequence and every GRU state.  On the grid (W1 = [Wa | Wb | Wc] over [h, h - t, t], E = 16):
//     AH[l] = (Wa + Wb) h_l   (64)        AT[i] = (Wc - Wb) t_i + b1   (64)        GX[l] = W_ih h_l   (48, no bias)
//     s[l]  = w3 . relu(W2 relu(AH[l] + AT[i]) + b2)         a = softmax_l(s)      (the score bias drops out)
//     gi_l  = a[l] GX[l] + b_ih       (= W_ih (a[l] h_l) + b_ih: the input projection is linear in the weight)
//     gh = W_hh h + b_hh;  r = sig(gi_r + gh_r);  z = sig(gi_z + gh_z);  n = tanh(gi_n + r gh_n);  h <- (1 - z) n + z h
// The caller hands in AT (num_items, 64) and HP = [AH | GX] (112 wide, read by history id or by position).  The walk
// is din_grid.hip's: a wave owns sixteen consecutive items, lane (q, n) keeps the operand-layout pieces of AT[i0 + n]
// (columns 16j + 4q .., 16 registers), the workgroup stages blocks of kPB positions' HP rows in LDS and the waves walk
// them; a position's pieces are LDS broadcasts.  The softmax has to be complete before the first GRU step -- the
// recurrence is not linear, so there is no online rescaling -- hence TWO passes over a row's positions:
//   pass 1  a0 = relu(AT + AH[l]), one layer_fwd (64 -> 32: 32 v_mfma_f32_16x16x4_f32), the w3 dot over the four lanes
//           of a column; running maximum and denominator; s[l] kept in the wave's LDS strip (64 B a position) for
//           l < kKeep, recomputed in pass 2 by the same device function beyond it (same instructions, same bits).
//   pass 2  a = exp(s - max) / den, gi = a GX[l] + b_ih, and one GRU step on the matrix cores: h stays in the C layout
//           (lane (q, n): units 4q .. 4q+3 of item n), which is the B operand of the next step's three 16 x 16 x 16
//           products against W_hh (gru.hip, gru16_mfma_fwd_kernel): 12 instructions, no cross-lane move.  Gates with
//           expf / tanhf.
// After the last position h_L goes to out[(r * num_items + i) * ldo + 0:16], the left half of the fc operand.
// Items past num_items: loads clamped to the last row, stores masked.  A history id outside the table raises *err_flag
// and is read as row 0.  No atomics, no hand-written waits; a pair's row is a function of its history row, its item's
// AT row and the weights alone, so the output is bitwise the same for any subset, order or repetition of history rows
// and under a permutation of the table.
//
// Cost: 44 matrix instructions per position and sixteen pairs (76 past kKeep), 2 (64 x 32 + 16 x 48) flop a pair.
#include "grid_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 1;                          // the layer behind the split one
constexpr int kK[kL] = {64};
constexpr int kN[kL] = {32};
constexpr int kN1 = 64;                        // width of an AH / AT row
constexpr int kE = 16;                         // embedding width = GRU width
constexpr int kG = 3 * kE;                     // width of a GX row
constexpr int kHP = kN1 + kG;                  // a staged row: [AH | GX], 448 bytes
constexpr int kPB = 32;                        // history positions of a staged block: 14 KiB
constexpr int kRT = 4;                         // history rows of a row tile (the unit handed out along gridDim.y)
constexpr int kKeep = CTR_DIEN_GRID_KEEP;      // positions whose score stays in LDS between the passes: 32 KiB
constexpr int kItems = 16 * kWaves;            // items of a workgroup

#include "mfma16_tower.inc"
#include "grid_frame.inc"

constexpr int kLdsFloats = kWFloats + kBFloats + kPB * kHP + kWaves * kKeep * 16;
constexpr int kStagePieces = kPB * (kHP / 4);                                   // 16-byte pieces of a block
constexpr int kStagePasses = (kStagePieces + kThreads - 1) / kThreads;          // 4 (the last one half full)

struct Grid {
  const float* at;                             // (ni, 64)
  const float* hp; int hp_by_position;         // (ni, 112) read by history id, or (rows * len, 112) read by position
  const float* w3;                             // 32
  const float* b_ih; const float* w_hh; const float* b_hh;   // 48, 48 x 16, 48
  const int64_t* hist;                         // (rows, len)
  int64_t rows, ni; int len;
  float* out; int64_t ldo;
  int32_t* err;
  int64_t tiles;
};

__device__ __forceinline__ float gate_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// the attention score of one staged position for the lane's item: every lane of a column returns the same bits
__device__ __forceinline__ float position_score(const float* s_w, const float* s_b, const float* row, int lane, int q,
                                                const f32x4 (&aT)[4], const f32x4 (&w3)[2]) {
  f32x4 a0[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 z = aT[j] + *reinterpret_cast<const f32x4*>(row + 16 * j + 4 * q);
#pragma unroll
    for (int c = 0; c < 4; ++c) a0[j][c] = fmaxf(z[c], 0.0f);
  }
  f32x4 y[2];
  layer_fwd<0, 4>(s_w, s_b, lane, q, a0, y);
  float s = 0.0f;                              // lane (q, n) holds units 16b + 4q + c of column n
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    s = fmaf(y[b][0], w3[b][0], s); s = fmaf(y[b][1], w3[b][1], s);
    s = fmaf(y[b][2], w3[b][2], s); s = fmaf(y[b][3], w3[b][3], s);
  }
  return column_sum(s);
}

__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
dien_grid_hidden_kernel(const Tower T, const Grid G) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_hp = s_b + kBFloats;                       // kPB x 112: HP rows of the position block
  float* s_sc = s_hp + kPB * kHP;                     // kWaves x kKeep x 16: the kept scores
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* strip = s_sc + wave * (kKeep * 16) + n;
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 16 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: the layer's weights, this lane's pieces of its item's AT row, the score and GRU operands
  f32x4 aT[4], w3[2];
  float ah[3][4];                                     // A operands: W_hh[gate g, unit n][input 4q + c]
  f32x4 ch[3], ci[3];                                 // b_hh, b_ih in accumulator layout: unit 4q + r
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
#pragma unroll
    for (int j = 0; j < 4; ++j) aT[j] = ldg4(G.at + ic * kN1 + 16 * j + 4 * q);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) w3[b][c] = G.w3[16 * b + 4 * q + c];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        ah[g][c] = G.w_hh[(g * kE + n) * kE + 4 * q + c];
        ch[g][c] = G.b_hh[g * kE + 4 * q + c];
        ci[g][c] = G.b_ih[g * kE + 4 * q + c];
      }
    stage_forward_store(s_w, s_b, wv, wdst, bv);
  }
  const bool store = item < G.ni;
  // the HP rows of positions [p0, p0 + cnt) of history row r into s_hp: every request before the first LDS store
  auto stage = [&](int64_t r, int p0, int cnt) {
    __syncthreads();                                  // the previous block's rows are read
    f32x4 v[kStagePasses];
#pragma unroll
    for (int e = 0; e < kStagePasses; ++e) {
      const int u = threadIdx.x + e * kThreads;
      const int pos = u / (kHP / 4), piece = u % (kHP / 4);
      const int64_t flat = r * G.len + p0 + (pos < cnt ? pos : cnt - 1);
      int64_t id = G.hist[flat];
      if (id < 0 || id >= G.ni) {
        if (G.err) *G.err = 1;
        id = 0;
      }
      v[e] = ldg4(G.hp + (G.hp_by_position ? flat : id) * kHP + 4 * piece);
    }
#pragma unroll
    for (int e = 0; e < kStagePasses; ++e) {
      const int u = threadIdx.x + e * kThreads;
      if (u < kStagePieces) *reinterpret_cast<f32x4*>(s_hp + 4 * u) = v[e];
    }
    __syncthreads();                                  // (the first block: the weights as well)
  };
  for (int64_t tile = blockIdx.y; tile < G.tiles; tile += gridDim.y) {
    const int64_t r1 = (tile + 1) * kRT < G.rows ? (tile + 1) * kRT : G.rows;
    for (int64_t r = tile * kRT; r < r1; ++r) {
      // ---- pass 1: the scores, their maximum and the softmax denominator
      float mx = -INFINITY, den = 0.0f;
      for (int p0 = 0; p0 < G.len; p0 += kPB) {
        const int cnt = G.len - p0 < kPB ? G.len - p0 : kPB;
        stage(r, p0, cnt);
        for (int p = 0; p < cnt; ++p) {
          const float s = position_score(s_w, s_b, s_hp + p * kHP, lane, q, aT, w3);
          // the four lanes of a column store the same bits to the same word: pass 2 reads back what the lane itself
          // wrote, so nothing but the thread's own program order stands between the store and the load
          if (p0 + p < kKeep) strip[(p0 + p) * 16] = s;
          const float mnew = fmaxf(mx, s);
          den = fmaf(den, expf(mx - mnew), expf(s - mnew));
          mx = mnew;
        }
      }
      // ---- pass 2: the recurrence (a single block is still staged)
      const float inv = 1.0f / den;
      f32x4 h = {0.f, 0.f, 0.f, 0.f};
      for (int p0 = 0; p0 < G.len; p0 += kPB) {
        const int cnt = G.len - p0 < kPB ? G.len - p0 : kPB;
        if (G.len > kPB) stage(r, p0, cnt);
        for (int p = 0; p < cnt; ++p) {
          const float* row = s_hp + p * kHP;
          float s;
          if (p0 + p < kKeep) {                       // (uniform over the workgroup)
            s = strip[(p0 + p) * 16];                 // this lane's own store of pass 1
          } else {
            s = position_score(s_w, s_b, row, lane, q, aT, w3);
          }
          const float a = expf(s - mx) * inv;
          f32x4 gi[3], gh[3];
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            const f32x4 gx = *reinterpret_cast<const f32x4*>(row + kN1 + g * kE + 4 * q);
            gh[g] = ch[g];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              gi[g][c] = fmaf(a, gx[c], ci[g][c]);
              gh[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[g][c], h[c], gh[g], 0, 0, 0);
            }
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float rg = gate_sigmoid(gi[0][c] + gh[0][c]);
            const float zg = gate_sigmoid(gi[1][c] + gh[1][c]);
            const float ng = tanhf(fmaf(rg, gh[2][c], gi[2][c]));
            h[c] = fmaf(zg, h[c] - ng, ng);           // (1 - z) n + z h
          }
        }
      }
      if (store) stg4(G.out + (r * G.ni + item) * G.ldo + 4 * q, h);
    }
  }
}

}  // namespace

extern "C" int ctr_dien_grid_hidden(const float* at, const float* hp, int hp_by_position, int64_t num_items, int embed,
                                    const float* w2, const float* b2, const float* w3, int n1, int n2, const float* b_ih,
                                    const float* w_hh, const float* b_hh, const int64_t* hist, int64_t rows, int len,
                                    float* out, int64_t ldo, int32_t* err_flag, void* stream) {
  CTR_REQUIRE(rows >= 0 && num_items >= 0 && len >= 1, CTR_EINVAL);
  CTR_REQUIRE(at && hp && w2 && b2 && w3 && b_ih && w_hh && b_hh, CTR_EINVAL);
  CTR_REQUIRE(embed == kE && n1 == kN1 && n2 == kN[0], CTR_ELIMIT);
  CTR_REQUIRE(num_items < ((int64_t)1 << 31), CTR_ELIMIT);
  CTR_REQUIRE(ldo >= kE, CTR_EINVAL);
  CTR_REQUIRE((hist && out) || rows == 0 || num_items == 0, CTR_EINVAL);
  CTR_REQUIRE(ldo % 4 == 0 && ctr_aligned16(at) && ctr_aligned16(hp) && ctr_aligned16(w2) && ctr_aligned16(out),
              CTR_EALIGN);
  if (rows == 0 || num_items == 0) return CTR_OK;
  Tower T;
  T.w[0] = w2; T.b[0] = b2; T.y[0] = nullptr; T.ldy[0] = 0;
  const int64_t tiles = ctr_ceil_div(rows, kRT);
  const Grid G{at, hp, hp_by_position != 0, w3, b_ih, w_hh, b_hh, hist, rows, num_items, len, out, ldo, err_flag, tiles};
  // item tiles along x (neighbouring workgroups share their position block's rows in L2), row tiles along y
  const int64_t gx = ctr_ceil_div(num_items, kItems);
  return grid_launch(dien_grid_hidden_kernel, dim3((unsigned)gx, grid_history_y(gx, tiles)), kThreads,
                     sizeof(float) * (size_t)kLdsFloats, stream, T, G);
}
