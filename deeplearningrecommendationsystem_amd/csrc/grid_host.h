// Host frame of the grid scorers ({ncf,din,dien,deepfm,pnn,afm,lowrank}_grid.hip): what surrounds a grid kernel's launch -- the
// argument checks the user-grid entries share, gridDim.y, and the launch itself.  Host code only: nothing here reaches
// a kernel's instruction stream (device helpers: grid_frame.inc).
#pragma once
#include "ctr_common.h"

// ---- the user x item entries (NeuralCF, DeepFM, Wide & Deep, PNN, AFM, low-rank): rows are users[r], or user0 + r; out is (rows, >= num_items)
// every failure of this check is CTR_EINVAL
static inline bool grid_users_ok(const int64_t* users, int64_t user0, int64_t rows, int64_t num_users, int64_t num_items,
                                 const float* out, int64_t ldo) {
  if (rows < 0 || num_users < 0 || num_items < 0 || ldo < num_items) return false;
  if (!users && !(user0 >= 0 && user0 <= num_users && rows <= num_users - user0)) return false;
  if (rows != 0 && num_users < 1) return false;
  return out || rows == 0 || num_items == 0;
}
// the table sizes the entries take: CTR_ELIMIT beyond
static inline bool grid_ids_fit(int64_t num_users, int64_t num_items) {
  return num_users < ((int64_t)1 << 31) && num_items < ((int64_t)1 << 31);
}

// ---- gridDim.y
// DeepFM, PNN, AFM: user tiles are dealt round-robin over y workgroups per item tile.  One workgroup per CU runs at a time,
// so the launch takes about ceil(x y / CUs) rounds of (prologue + ceil(utiles / y) tiles); the prologue is charged as
// 1 / tiles_per_prologue of a tile.  The smallest y with the least cost among the grids of at most kGridMaxRounds x CUs
// workgroups, so that a workgroup walks many tiles wherever there are many.
constexpr int kGridMaxRounds = 8;
static inline int64_t grid_row_blocks(int64_t xtiles, int64_t utiles, int tiles_per_prologue) {
  const int64_t cap = kGridMaxRounds * kCtrCUs / xtiles > 1 ? kGridMaxRounds * kCtrCUs / xtiles : 1;
  const int64_t ymax = utiles < cap ? utiles : cap;
  int64_t best = 1, best_cost = -1;
  for (int64_t y = 1; y <= ymax; ++y) {
    const int64_t cost = ctr_ceil_div(xtiles * y, kCtrCUs) * (1 + tiles_per_prologue * ctr_ceil_div(utiles, y));
    if (best_cost < 0 || cost < best_cost) best = y, best_cost = cost;
  }
  return best;
}
// a y extent: no more workgroups than tiles to walk, and what a grid dimension holds
static inline unsigned grid_clamp_y(int64_t y, int64_t tiles) {
  y = y < tiles ? y : tiles;
  return (unsigned)(y < 65535 ? y : 65535);
}
// DIN, DIEN: as many workgroups as fill the machine a few times over, each walking its share of the row tiles behind
// one weight prologue
static inline unsigned grid_history_y(int64_t gx, int64_t tiles) {
  return grid_clamp_y(ctr_ceil_div((int64_t)kCtrCUs * 8, gx), tiles);
}

// ---- the launch: `lds_bytes` of dynamic LDS (above the 64 KiB a kernel gets unasked), the two by-value arguments
template <typename A, typename B>
static inline int grid_launch(void (*kernel)(const A, const B), dim3 grid, int threads, size_t lds_bytes, void* stream,
                              const A& a, const B& b) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes) != hipSuccess)
    return CTR_ELAUNCH;
  hipLaunchKernelGGL(kernel, grid, dim3(threads), lds_bytes, (hipStream_t)stream, a, b);
  return ctr_launch_status();
}
