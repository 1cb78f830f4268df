// What the direct-to-LDS GEMM kernels (gemm_dlds.hip, gemm_dlds_dx.hip, gemm_dlds_dw.hip, gemm_wide.hip) and the
// tile kernel's launcher (linear.hip) share: the format of an LDS stage, the three-stage ring and the tile policy.
//
// FORMAT.  A direct load (global_load_lds_dwordx4) writes lane L's 16 bytes at M0 + 16 L: the LDS image of a wave's
// instruction is one contiguous 1 KB run and cannot be padded, so a stage is a sequence of 16-byte chunk SLOTS and bank
// conflicts are avoided by choosing WHICH global chunk each slot holds.  A 16-deep operand tile that is read along
// the contraction keeps, in slot q, row q / 4 and k-chunk (q & 3) ^ ((row >> 1) & 3) of that row: the 8 rows a
// quarter-wave reads with one ds_read_b128 then cover all 32 banks.  A tile that is read down its rows is the plain
// row-major [16][W] block.  The loads need 4-byte alignment only.  No load leaves its matrix: rows past the end are
// clamped to the last row, and a chunk that would cross the end of its row is fetched from 4 floats before the end
// (chunk_start); the reader zeroes what is then a duplicate (contraction side) or adds the shift (tail_shift).
//
// RING.  Wave w's i-th load of a tile fills slots wave_slot0(w, i) .. + 63.  Three stages: the loads of pipeline slot
// g + 2 are issued at step g.  They are waited for by hand (wait_vmcnt counts this wave's loads still in flight, so
// every wave must issue the same number per slot), and fragments are read with ds_read_b128 from asm: the compiler
// cannot tell which stage an LDS-DMA load targets and would put vmcnt(0) in front of every ordinary LDS read.
#pragma once
#include "ctr_common.h"

namespace gemm_ring {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kBK = 16;  // contraction depth of one pipeline step
constexpr int kStages = 3;  // of the direct-to-LDS ring (linear.hip's register-staged tile kernel has two buffers of its own)

// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  __builtin_amdgcn_s_waitcnt((N & 0xF) | (0x7 << 4) | (0xF << 8) | ((N >> 4) << 14));
}
__device__ __forceinline__ f32x4 lds_read128(uint32_t byte_addr) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(byte_addr));
  return v;
}

// ---- stage format ----
__device__ __forceinline__ int stage_swizzle(int row) { return (row >> 1) & 3; }
// slot -> (row, k-chunk) and back
__device__ __forceinline__ int slot_row(int q) { return q >> 2; }
__device__ __forceinline__ int slot_chunk(int q) { return (q & 3) ^ stage_swizzle(q >> 2); }
__device__ __forceinline__ int chunk_slot(int row, int c) { return row * 4 + (c ^ stage_swizzle(row)); }

// first slot of wave `wave`'s i-th load (uniform).  A tile of fewer chunks than threads is fetched twice (same bytes
// to the same slots): every wave then has the same number of loads in flight, which wait_vmcnt relies on
template <int kChunks>
__device__ __forceinline__ int wave_slot0(int wave, int i) {
  int q0 = 64 * wave + kThreads * i;
  if (kChunks % kThreads != 0 && q0 >= kChunks) q0 -= kChunks;
  return q0;
}

// where the 4-float chunk that should start at `at` is fetched from in a row of `total` floats
template <class T>
__device__ __forceinline__ T chunk_start(T at, T total) {
  return at < total - 4 ? at : total - 4;
}
// ... and logical column `col` then sits this many floats further right in its (shifted) last chunk
__device__ __forceinline__ int tail_shift(int col, int total) {
  return (total & 3) && col >= (total & ~3) && col < total ? 4 - (total & 3) : 0;
}

// copy 16 rows x columns [col0, col0 + W) of a row-major matrix into a plain [16][W] stage.  Tile row `row` is source
// row row0 + row, clamped to last_start in aligned groups of G rows (G = 4: the rows follow the chunks of a swizzled
// tile's contraction tail)
template <int W, int G, class Row>
__device__ __forceinline__ void fetch_plain(float* stage, const float* __restrict__ src, int64_t ld, Row row0,
                                            Row last_start, int col0, int cols_total, int lane, int wave) {
  constexpr int kPerRow = W / 4, kChunks = 16 * kPerRow;
  constexpr int kIters = (kChunks + kThreads - 1) / kThreads;
#pragma unroll
  for (int i = 0; i < kIters; ++i) {
    const int q0 = wave_slot0<kChunks>(wave, i);
    const int q = q0 + lane;
    const int row = q / kPerRow, cc = q % kPerRow;
    Row gr = row0 + (row & ~(G - 1));
    gr = (gr < last_start ? gr : last_start) + (row & (G - 1));
    const int col = chunk_start(col0 + cc * 4, cols_total);
    ctr_dma16(src + (int64_t)gr * ld + col, __builtin_amdgcn_readfirstlane(ctr_lds_addr(stage + q0 * 4)));
  }
}

// ---- ring ----
__device__ __forceinline__ int ring_next(int stage) { return stage + 1 == kStages ? 0 : stage + 1; }
__device__ __forceinline__ int ring_refill(int stage) {  // the stage two slots ahead
  const int refill = stage + 2;
  return refill >= kStages ? refill - kStages : refill;
}
// the (tile, step) cursor of a workgroup that walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... with nk steps each.
// The kernels keep the two-slots-ahead prologue (t1 = tile, k1 = 0, advance; t2 = t1, k2 = k1, advance) in their own
// text: moved in here, as a struct or as a function, it changed the prologue of every forward and dX instantiation and
// one forward timing with it (profiles/gemm_ring_refactor.txt)
__device__ __forceinline__ void ring_advance(int64_t& t, int& k, int nk) {
  if (++k == nk) {
    k = 0;
    t += gridDim.x;
  }
}

// C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
// `base` goes first and the terms stay in this order: base + (row of e, h) re-associates a 64-bit sum, which cost the
// forward 2 VGPRs and 2.3 % instructions, and even base + (row of e) + 4 * h moved the input gradient's code
template <class T>
__device__ __forceinline__ T mfma_row(T base, int e, int h) {
  return base + (e & 3) + 8 * (e >> 2) + 4 * h;
}
__device__ __forceinline__ int mfma_row(int e) { return mfma_row(0, e, 0); }  // lower half-wave, from the block's top

// ---- tile policy (host) ----
// a workgroup's tile is 128 x 32*nt
inline int pick_nt(int n) { return n <= 32 ? 1 : (n <= 64 ? 2 : 4); }
// few row tiles (a table of ~1000 rows instead of a batch): 128 x 128 tiles would leave most CUs without a workgroup
// (943 x 256: 16 of them) -- narrower column tiles re-read the few rows from L2 and fill the chip
inline int narrow_nt(int nt, int64_t mtiles, int cols, int zs = 1) {
  while (nt > 1 && mtiles * ctr_ceil_div(cols, 32 * nt) * zs < 128) nt >>= 1;
  return nt;
}
// persistent grid: the workgroups that are resident at once, shared among the `others` tiles of the other grid axes
// (rounded down: one workgroup more would start a second round), at most one per row tile
inline int64_t ring_grid(int wgs_per_cu, int64_t others, int64_t mtiles) {
  int64_t gx = kCtrCUs * wgs_per_cu / others;
  if (gx > mtiles) gx = mtiles;
  if (gx < 1) gx = 1;
  return gx;
}
// floats a rows x cols output occupies when `rows` takes the 128-wide side of the tile
inline int64_t padded(int64_t rows, int64_t cols) {
  const int nt = pick_nt((int)cols);
  return ctr_ceil_div(rows, 128) * 128 * ctr_ceil_div(cols, 32 * nt) * 32 * nt;
}

}  // namespace gemm_ring
