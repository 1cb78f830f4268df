// NeuralCF when the vocabularies are much smaller than the batch (BASELINE configs[1]: 943 users / 1682 items, batch
// 65536): the first tower layer is moved from the SAMPLES to the TABLE ROWS.
//
// The reference computes  z0[b] = W0 . cat(MLP_U[u_b], MLP_I[i_b]) + b0  (model/neuralcf.py:43-49) for every sample:
// 2 * 128 * 64 flops per sample, three quarters of the tower's arithmetic, and its backward another 2x that plus a
// (B, 128) input gradient that the embedding backward has to segment-sum by row.  But a linear layer on a
// concatenation of two gathered rows is the sum of two gathered PROJECTED rows:
//     z0[b] = P_U[u_b] + P_I[i_b],      P_U = MLP_U . W0[:, :64]^T  (U x 64),   P_I = MLP_I . W0[:, 64:]^T + b0  (I x 64)
// -- two small matrix products over U + I = 2625 rows instead of one over 65536 samples -- and the chain rule gives
//     S_U[u] = sum_{b: u_b = u} gz0[b]   (same for S_I),        gz0 = relu'(z0) * (W1^T gz1)
//     dMLP_U = S_U . W0[:, :64],   dW0[:, :64] = S_U^T . MLP_U,   db0 = column sums of S_U
// so layer 0's dX and dW GEMMs over the batch (128 + 128 of the 344 matrix instructions a sample group cost the
// per-sample kernel, mlp_mfma16.hip) become products over the table rows as well.  The GMF half folds the same way:
//     T_U[u] = sum_{b: u_b = u} gz_b * GMF_I[i_b],   dGMF_U = wfold[:64] * T_U,   gwfold[:64] = sum_u GMF_U[u] * T_U[u]
// (gz_b = the head's pre-activation gradient, a scalar per sample).  What is left per sample is the 64-32-16-8 tower,
// the head's dot product and ONE 64-float row gz0[b] -- which is all the segment sums need.
//
// The segment sums are formed without a sort and without a global returning atomic.  The training forward builds a
// bucket PLAN, once: the batch is cut into at most kChunks contiguous chunks, a workgroup per chunk (beside the
// projection workgroups of ncfp_prep) counts the chunk's samples per table row in an LDS histogram -- the returning LDS
// atomic is the sample's rank inside (row, chunk) -- and stores the histogram, zeros included, and its sums over every
// block of 256 rows; a few workgroups behind the per-sample ones of ncfp_fwd, one per block, turn every row's counts
// into exclusive prefixes over the chunks and a row total, scan their own totals and add the blocks in front of them
// from those block sums: rows + 1 bucket offsets, each workgroup its own rows', with no ticket, fence or wait inside the
// launch.  The prefixes are stored with the offset folded in (base[chunk][row] = offset[row] + the row's samples in
// earlier chunks).  The backward kernel stores each sample's gz0 row ONCE, at the sample's own row of a (batch + 1, 64)
// buffer, plus a 16-byte record {gz, partner id, row, sample} into the sample's slot of its user's bucket and of its
// item's, slot = base[chunk][row] + rank: a bucket is a run of records, and a record names the gz0 row and the
// partner GMF row of its sample.  A streaming kernel then sums the buckets, fetching both rows through the record
// (balanced over SLOT ranges, so a hot row of a skewed id distribution is shared by many waves).  Same values as the
// per-sample path up to fp32 summation order; inside a bucket the chunks follow each other in batch order, the order
// inside (row, chunk) follows the LDS atomics, so table gradients are reproducible to rounding, not bitwise.
//
// Launches: forward  ncfp_prep (projected tables, head fold, chunk histograms + block sums) -> ncfp_fwd (+ bases, offsets);
// backward  ncfp_bwd -> ncfp_segsum -> ncfp_finish (the table-row products + tower dW partials, head fold chain rule).
#include "ctr_common.h"

#include <stdlib.h>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kL = 3;                          // the layers that stay per sample
constexpr int kK[kL] = {64, 32, 16};
constexpr int kN[kL] = {32, 16, 8};
constexpr int kH = 64;                         // width of an MLP embedding row = half of layer 0's input
constexpr int kN0 = 64;                        // layer-0 units = width of a projected row
constexpr int kP = 64;                         // GMF width = head's extra columns
constexpr int kNL = 8;                         // head: last activations
constexpr int kHeadW = kP + kNL;

#include "mfma16_tower.inc"

#ifdef CTR_STAMPS
// dev/ncfp_stamps.py: cycle stamps of wave 0 of workgroup 7 (a build of its own: the product has no stamp instruction)
__device__ unsigned long long g_stamps[2][64];
#define STAMP(k, i) do { const int at_ = (i); if (blockIdx.x == 7 && threadIdx.x == 0 && at_ < 64) g_stamps[k][at_] = __builtin_readcyclecounter(); } while (0)
#else
#define STAMP(k, i) do {} while (0)
#endif

struct Ids {
  const int64_t* uidx; int64_t ustride;
  const int64_t* iidx; int64_t istride;
  int64_t nu, ni;
};

// ------------------------------------------------------------------ the bucket plan of a training forward
// The caller's plan buffer (rows * CTR_NCF_PROJ_COUNT_STRIDE int32, rows = nu + ni):
//   [0 .. 3]           head: never touched by the device (word 0 is the word the caller keeps zero; base stays 16-byte aligned)
//   base   [chunk][row]  after ncfp_prep: samples of `row` in `chunk`; after ncfp_fwd: the slot of the row's first sample
//                        of that chunk = offsets[row] + the samples of `row` in EARLIER chunks
//   totals [row]         samples of the row in the batch
//   offsets[rows + 1]    exclusive scan of the totals (user rows first): where a row's bucket begins; [rows] = all slots
//   blk    [chunk][block]  (more than kPlanBlock rows only) after ncfp_prep: samples of `chunk` in the rows of `block`
// A chunk is 2^shift consecutive samples (at least one sample per thread of its workgroup, at most kChunks chunks), so
// the chunk of a sample is a shift of its index.  A block is kPlanBlock consecutive rows: the rows of one plan workgroup.
// Every entry a later launch reads is written by an earlier one, zeros included: nothing has to be clear, and nothing
// is cleared afterwards.
constexpr int kChunks = 64;
constexpr int kPlanHead = 4;                   // int32 in front of base
constexpr int kPlanBlock = 256;                // rows of a block = threads of a plan workgroup
static_assert(kPlanHead + 2 * (kChunks + 2) + 1 <= 2 * CTR_NCF_PROJ_COUNT_STRIDE,
              "CTR_NCF_PROJ_COUNT_STRIDE: the plan of the smallest tables (two rows) does not fit");
// blk exists from kPlanBlock + 1 rows on (two blocks); every kPlanBlock rows more add kChunks entries to it and
// (CTR_NCF_PROJ_COUNT_STRIDE - kChunks - 2) * kPlanBlock to the room behind the offsets
static_assert(kPlanHead + (kChunks + 2) * (kPlanBlock + 1) + 1 + kChunks * 2 <= (kPlanBlock + 1) * CTR_NCF_PROJ_COUNT_STRIDE &&
                  kChunks <= (CTR_NCF_PROJ_COUNT_STRIDE - kChunks - 2) * kPlanBlock,
              "CTR_NCF_PROJ_COUNT_STRIDE: the block totals do not fit behind the offsets");
struct Plan {
  int32_t* base; int32_t* totals; int32_t* offsets; int32_t* blk;
  int64_t rows;
  int shift, chunks, nblk;
};
Plan plan_of(int32_t* buf, int64_t rows, int64_t m) {
  int shift = 8;
  while (((int64_t)kChunks << shift) < m) ++shift;
  Plan p;
  p.base = buf + kPlanHead;
  p.totals = p.base + kChunks * rows;
  p.offsets = p.totals + rows;
  p.blk = p.offsets + rows + 1;
  p.rows = rows;
  p.shift = shift;
  p.chunks = (int)((m + ((int64_t)1 << shift) - 1) >> shift);
  p.nblk = (int)((rows + kPlanBlock - 1) / kPlanBlock);
  return p;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Ranks of one chunk, by workgroup `first` + chunk of a launch that has other work in its first workgroups: an LDS
// histogram over the rows, a returning LDS atomic per sample and id column, an 8-byte record out, then the histogram
// and its sums over the blocks of kPlanBlock rows.
// All ids of a pass are requested before the first atomic (id -> atomic -> store, one sample after the other, is a chain
// of round trips).  Ids sorted by user put a whole wave on one LDS counter: 64 serialised LDS operations, not 64
// memory-side ones.
struct RankJob {
  Ids ids;
  Plan plan; int32_t* ranks;
  int64_t m;
  int first;
};
constexpr int kRankPer = 4;                    // samples of a thread in flight
__device__ __forceinline__ void rank_role(const RankJob& R) {
  extern __shared__ __attribute__((aligned(16))) int s_hist[];   // rows
  const int chunk = (int)blockIdx.x - R.first;
  const int rows = (int)R.plan.rows;
  for (int i = threadIdx.x; i < rows; i += kThreads) s_hist[i] = 0;
  __syncthreads();
  const int64_t lo = (int64_t)chunk << R.plan.shift;
  const int64_t hi = lo + ((int64_t)1 << R.plan.shift) < R.m ? lo + ((int64_t)1 << R.plan.shift) : R.m;   // (lo < m: chunk < chunks)
  for (int64_t s0 = lo + threadIdx.x; s0 < hi; s0 += kRankPer * kThreads) {
    int64_t u[kRankPer], i[kRankPer];
#pragma unroll
    for (int e = 0; e < kRankPer; ++e) {
      const int64_t s = s0 + e * kThreads < hi ? s0 + e * kThreads : hi - 1;
      u[e] = R.ids.uidx[s * R.ids.ustride];
      i[e] = R.ids.iidx[s * R.ids.istride];
    }
#pragma unroll
    for (int e = 0; e < kRankPer; ++e) {
      const int64_t s = s0 + e * kThreads;
      if (s < hi) {
        int ru = -1, ri = -1;                  // an id outside its table has no slot (the per-sample part raises the flag)
        if ((uint64_t)u[e] < (uint64_t)R.ids.nu) ru = atomicAdd(s_hist + u[e], 1);
        if ((uint64_t)i[e] < (uint64_t)R.ids.ni) ri = atomicAdd(s_hist + R.ids.nu + i[e], 1);
        *reinterpret_cast<int2*>(R.ranks + 2 * s) = make_int2(ru, ri);
      }
    }
  }
  __syncthreads();
  int32_t* out = R.plan.base + (int64_t)chunk * rows;
  for (int i = threadIdx.x; i < rows; i += kThreads) out[i] = s_hist[i];
  // block totals (more than one plan workgroup only): a wave per block, four LDS reads a lane and one wave sum -- the
  // histogram is complete and only read from here on, so this needs no barrier and waits for none of the stores above
  const int nblk = R.plan.nblk;
  if (nblk > 1) {
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x >> 6; k < nblk; k += kWaves) {
      int v = 0;
#pragma unroll
      for (int e = 0; e < kPlanBlock / 64; ++e) {
        const int i = k * kPlanBlock + e * 64 + lane;
        v += i < rows ? s_hist[i] : 0;
      }
      v = wave_sum_int(v);
      if (lane == 0) R.plan.blk[chunk * nblk + k] = v;
    }
  }
}

// Prefixes and offsets, by workgroups `first` .. of the launch behind ncfp_prep, workgroup k for the rows of block k: a
// thread per row sums the row's chunk counts into exclusive prefixes and a total; the workgroup scans its totals (a
// wave scan and one combine over the waves) and adds the samples of all blocks in front of it, which ncfp_prep left as
// block totals per chunk -- so every workgroup finishes its own rows' offsets alone: nothing in this launch is ordered
// against anything else in it.  Stored: the totals, the offsets, and base[chunk][row] = offset + prefix, in place.
struct PlanJob {
  Plan plan;
  int first;
};
constexpr int kBlkPer = 16;                    // block totals a thread sums: blocks kWaves e + wave of chunk `lane`
static_assert(kChunks == 64 && kPlanBlock == kThreads && CTR_NCF_PROJ_MAX_ROWS <= kPlanBlock * kWaves * kBlkPer,
              "plan_role: a lane per chunk, a thread per row of the block, kWaves * kBlkPer blocks at most");
__device__ __forceinline__ void plan_role(const PlanJob& J) {
  __shared__ int s_scan[kWaves], s_front[kWaves];
  const Plan& P = J.plan;
  const int64_t rows = P.rows;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = (int)blockIdx.x - J.first;     // this workgroup's block
  const int64_t row = (int64_t)k * kPlanBlock + threadIdx.x;
  const int64_t rr = row < rows ? row : rows - 1;
  // every load of the thread is requested before any is used: the block totals in front of block k (k <= 63 blocks x
  // 64 chunks over 256 threads; the branch is uniform), then the row's chunk counts
  int front = 0, f[kBlkPer];
#pragma unroll
  for (int e = 0; e < kBlkPer; ++e) {
    f[e] = 0;
    if (kWaves * e < k) f[e] = P.blk[(lane < P.chunks ? lane : P.chunks - 1) * P.nblk + (kWaves * e + wave < k ? kWaves * e + wave : 0)];
  }
  int v[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; ++c) v[c] = P.base[(int64_t)(c < P.chunks ? c : P.chunks - 1) * rows + rr];
#pragma unroll
  for (int e = 0; e < kBlkPer; ++e) front += (lane < P.chunks && kWaves * e + wave < k) ? f[e] : 0;
  int total = 0;
#pragma unroll
  for (int c = 0; c < kChunks; ++c) total += c < P.chunks ? v[c] : 0;
  total = row < rows ? total : 0;
  int inc = total;   // inclusive scan of the totals over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  front = wave_sum_int(front);
  if (lane == 63) s_scan[wave] = inc;
  if (lane == 0) s_front[wave] = front;
  __syncthreads();
  int offset = (s_front[0] + s_front[1]) + (s_front[2] + s_front[3]) + inc - total;
  for (int w = 0; w < wave; ++w) offset += s_scan[w];
  if (row < rows) {
    P.totals[row] = total;
    P.offsets[row] = offset;
    if (row == rows - 1) P.offsets[rows] = offset + total;
    int run = offset;
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
      if (c < P.chunks) {
        P.base[(int64_t)c * rows + row] = run;
        run += v[c];
      }
  }
}

// ------------------------------------------------------------------ prep: projected tables + head fold
struct Prep {
  const float* mlp_u; const float* mlp_i;      // (nu, 64), (ni, 64)
  const float* w0; int64_t ldw0; const float* b0;   // layer 0: (64, 128), (64)
  float* ptab;                                 // (nu + ni, 64): P_U rows, then P_I rows
  int64_t nu, ni;
  // head fold (ctr_fold_head_fwd's map for p = 64, n = 64, k = 8): wfold[0:72], wfold[72] = cfold
  const float* fold_u; const float* fold_w; int64_t fold_ldw; const float* fold_b; const float* fold_b2;
  float* wfold;
  RankJob rank;                                // training: the batch's ranks and chunk histograms, by workgroups rank.first ..
};

__global__ void __launch_bounds__(kThreads)
ncfp_prep_kernel(const Prep A) {
  if ((int)blockIdx.x >= A.rank.first) {
    rank_role(A.rank);
    return;
  }
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int64_t wave = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const int64_t ublocks = (A.nu + 15) / 16, iblocks = (A.ni + 15) / 16;
  if ((int)blockIdx.x == A.rank.first - 1) {
    // the folded head (ctr_fold_head_fwd's map): wfold[t < 64] = u[t]; wfold[64 + c] = sum_i W[i][c] u[64 + i] (column c
    // by the 32 threads t % 8 == c, two terms each, summed through LDS); wfold[72] = b . u[64:] + b2
    __shared__ float s_f[kThreads];
    const int t = threadIdx.x;
    const float* u = A.fold_u + kP;
    if (t < kP) A.wfold[t] = A.fold_u[t];
    {
      const int c = t & 7, i = t >> 3;                 // i in 0..31: terms i and i + 32
      s_f[t] = fmaf(A.fold_w[(int64_t)i * A.fold_ldw + c], u[i], A.fold_w[(int64_t)(i + 32) * A.fold_ldw + c] * u[i + 32]);
    }
    __syncthreads();
    if (t < kNL) {
      float acc = 0.0f;
      for (int i = 0; i < 32; ++i) acc += s_f[8 * i + t];
      A.wfold[kP + t] = acc;
    }
    __syncthreads();
    if (t < 64) s_f[t] = A.fold_b ? A.fold_b[t] * u[t] : 0.0f;
    __syncthreads();
    if (t == 0) {
      float acc = A.fold_b2 ? A.fold_b2[0] : 0.0f;
      for (int i = 0; i < 64; ++i) acc += s_f[i];
      A.wfold[kHeadW] = acc;
    }
  }
  // one wave = sixteen table rows x 32 units: out^T (32 units x 16 rows) = W0half (32 x 64) . X^T (64 x 16 rows) -- 32
  // dependent matrix instructions, not 64; the two waves of a row block take the unit blocks {0, 1} and {2, 3}, and an
  // output's sum over the inputs keeps its order
  const int64_t rblk = wave >> 1;
  const int hb = 2 * (int)(wave & 1);
  if (rblk >= ublocks + iblocks) return;
  const bool user = rblk < ublocks;
  const int64_t row = (user ? rblk : rblk - ublocks) * 16 + n, rows = user ? A.nu : A.ni;
  const float* tab = user ? A.mlp_u : A.mlp_i;
  const int coff = user ? 0 : kH;
  const bool live = row < rows;
  f32x4 x[4], acc[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = ldg4(tab + (live ? row : 0) * kH + 16 * j + 4 * q);
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    if (!user && A.b0) acc[b] = ldg4(A.b0 + 16 * (hb + b) + 4 * q);
    else acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f32x4 w[2];   // A operands straight from the weight rows: W0[16 (hb + b) + n][coff + 16j + 4q + c]
#pragma unroll
    for (int b = 0; b < 2; ++b) w[b] = ldg4(A.w0 + (int64_t)(16 * (hb + b) + n) * A.ldw0 + coff + 16 * j + 4 * q);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[b][c], x[j][c], acc[b], 0, 0, 0);
  }
  if (live) {
    float* dst = A.ptab + ((user ? 0 : A.nu) + row) * kN0 + 4 * q;
#pragma unroll
    for (int b = 0; b < 2; ++b) stg4(dst + 16 * (hb + b), acc[b]);
  }
}

// ------------------------------------------------------------------ forward
struct Fwd {
  Ids ids;
  const float* ptab;                           // (nu + ni, 64)
  const float* gmf_u; const float* gmf_i;      // (nu, 64), (ni, 64)
  const float* wfold;                          // 72 weights + the bias
  float* out; int64_t ldout; int act;
  int32_t* err_flag;
  // training: workgroups plan.first .. gridDim - 1 of the SAME launch finish the bucket plan whose chunk histograms the
  // projection launch left (plan_role).  They share the CUs with the per-sample workgroups (two workgroups' worth of LDS
  // fit a CU) and are done long before those are.  (Ranks by returning GLOBAL atomics, one per sample and id column,
  // cost 12 of the forward's 25.8 us inside the per-sample loop and still 2-4 us on workgroups of their own with a
  // 64-byte line per counter: same-line atomics are served one after the other at the memory side, ~30 ns each,
  // profiles/r03_rank_atomics.txt.)
  PlanJob plan;
};

// How the loops of this file are written (what the first version got wrong, found with cycle stamps, an ablation and
// the TA / TCP counters: dev/ncfp_stamps.py, profiles/r03_ncfp_*; the ablation's kernel variants and their script were
// retired and are in git history):
//  * hipcc puts a `s_waitcnt vmcnt(0)` INSIDE every conditional block that consumes a load (`live ? a[i] + b[i] : 0`
//    becomes a branch around two loads, their wait and the add): a fetch written that way is a chain of round trips.
//    Every load here is unconditional (rows past the batch are clamped), every store too (lanes without a sample write
//    to a spare row every per-sample buffer has), so the compiler can count them.
//  * loading a gathered row straight into matrix-core operand layout -- lane (q, n) takes 16 bytes at column 16j + 4q
//    of sample n's row -- makes NEIGHBOURING lanes read DIFFERENT rows: 64 separate 16-byte requests per instruction
//    (TCP_TOTAL_CACHE_ACCESSES = 57 per vector-memory instruction, the texture addresser busy 75 % of the kernel).  The
//    rows are therefore fetched COALESCED -- sixteen lanes per 256-byte row, four rows per instruction -- by LDS-DMA
//    (global_load_lds_dwordx4: per-lane source address, wave-contiguous LDS image) into a wave-private stage, and read
//    back in operand layout with ds_read_b128; the source chunk a lane fetches is XOR-swizzled with its row so that the
//    sixteen rows a quarter-wave reads at one column land on sixteen different bank groups.
//  * the two dependent stages of a gather -- ids, then the rows they name -- are split over iterations: group g waits
//    once, reads its staged rows into registers, requests the rows of the next group (their ids arrived with that wait)
//    and the ids of the one after, and only then computes.
//
// LDS-DMA and its waits are written by hand (the compiler cannot see which bytes an LDS-DMA writes and would wait for
// every load in front of every LDS read).  Vector-memory operations retire in issue order; per group a wave issues
//   [kDma row fetches] [register loads, the forward's GMF rows] [2 id loads] [kStores stores]
// so `vmcnt(kStores)` at the head of the next group means: its rows are staged and its successor's ids are here, while
// this group's stores may still be on their way.  (The compiler counts the register loads itself; it does not see the
// LDS-DMA fetches, which are older than anything it waits for, so its count can only be too careful, never too lax.)
//
// Only rows that become MATRIX OPERANDS go through the stage.  The forward's GMF rows feed the head's scalar
// sum_k wfold[k] GMF_U[u][k] GMF_I[i][k] alone: they are loaded into registers with the DMA's address pattern (sixteen
// lanes per row, four rows per instruction), multiplied where they land and summed over the sixteen lanes of their row
// (row_sum16).  That halves the stage -- per group 8 KB less written into LDS and 8 KB less read back, of the 76 KB a
// group moved through it (44 KB of weight operands, 16 + 16 KB of rows); the workgroup's LDS is
// (2816 + 128 + 80 + 4 x 2048) x 4 B = 44.9 KB.  Round 9 measured the forward 1.0-1.3 us faster for it
// (profiles/r09_ncf_fwd_two_waves.txt, where the geometries that did NOT pay are recorded as well: see kFwdWgs).
constexpr int kFwdStage = 2 * 16 * 64;   // floats per wave: P_U, P_I rows of sixteen samples
constexpr int kFwdStores = 5;            // y1 x 2, y2, y3, prob

// Two waves per SIMD: one of a per-sample workgroup and one of a plan workgroup.  The attribute is an ALLOCATION as
// well as a budget: the compiler pads the kernel (134 registers) to 169 so that a third wave can never join.
//
// kNear: a group's sixteen rows of y1 and of y2 (and the spare row, behind the last group) lie inside one 4 GB store
// window (fwd_rows_near): those rows are written through the L2.  A row stride beyond that keeps the plain stores.  Two
// instantiations, not a branch in the group loop: behind a branch hipcc no longer counts the stores that follow the
// next group's loads in straight-line code, and its own wait behind the hand-placed one came out as vmcnt(2) -- three
// of the group's stores waited for, written through or not.
constexpr int64_t kNearStride = (int64_t)1 << 26;   // floats: fifteen rows of this stride and a row are under 2^32 bytes
bool fwd_rows_near(const Tower& T) { return T.ldy[0] < kNearStride && T.ldy[1] < kNearStride; }

template <bool kNear>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
ncfp_fwd_kernel(const Tower T, int64_t m, const Fwd F) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if ((int)blockIdx.x >= F.plan.first) {
    plan_role(F.plan);
    return;
  }
  float* s_w = lds;                                   // kWFloats
  float* s_b = s_w + kWFloats;                        // kBFloats
  float* s_hw = s_b + kBFloats;                       // kHeadW + 4 (+ 4 pad)
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* stage = s_hw + 80 + wave * kFwdStage;        // this wave's rows: [table][row][chunk ^ row] x 16 bytes
  const uint32_t stage_addr = ctr_lds_addr(stage);
  const int64_t groups = (m + 15) / 16;
  const int64_t wave0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6, nwaves = ((int64_t)F.plan.first * kThreads) >> 6;
  const uint32_t nu = (uint32_t)F.ids.nu, ni = (uint32_t)F.ids.ni;
  const float* tabs[2] = {F.ptab, F.ptab + F.ids.nu * kN0};
  // stage 1: the two ids of this lane's sample (sample n of the group, the same in its four lanes)
  int64_t idu = 0, idi = 0;
  auto issue_ids = [&](int64_t g) {
    int64_t row = g * 16 + n;
    row = row < m ? row : m - 1;
    idu = F.ids.uidx[row * F.ids.ustride];
    idi = F.ids.iidx[row * F.ids.istride];
  };
  // stage 2: the four rows of every sample of the group.  Instruction k of a table moves rows 4k .. 4k+3, sixteen
  // lanes per row.  The projected rows by LDS-DMA: lane l fetches chunk (l % 16) ^ row of row 4k + l / 16 into slot
  // (row, l % 16).  The GMF rows into registers: lane l takes chunk l % 16 (columns 4 (l % 16) ..) of row 4k + l / 16.
  f32x4 gu[4], gi[4];
  auto issue_rows = [&](int64_t g) {
    const bool live = g * 16 + n < m;
    const bool ubad = (uint64_t)idu >= nu, ibad = (uint64_t)idi >= ni;
    const uint32_t u = ubad ? 0u : (uint32_t)idu, i = ibad ? 0u : (uint32_t)idi;
    if (live && (ubad || ibad) && F.err_flag) *F.err_flag = 1;
    uint32_t ur[4], ir[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 4 * k + q;                          // the row this lane helps to fetch
      const int src = (lane & 48) | r;                  // a lane of this quarter that holds sample r's ids
      ur[k] = (uint32_t)__shfl((int)u, src, 64) * 64u;
      ir[k] = (uint32_t)__shfl((int)i, src, 64) * 64u;
      const uint32_t col = 4u * (uint32_t)(n ^ r);      // swizzled 16-byte chunk of the row
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float* g_ = tabs[t] + (t ? ir[k] : ur[k]) + col;
        ctr_dma16(g_, stage_addr + (uint32_t)((t * 16 + 4 * k) * 256));
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      gu[k] = ldg4(F.gmf_u + ur[k] + 4 * n);
      gi[k] = ldg4(F.gmf_i + ir[k] + 4 * n);
    }
  };
  // behind a hand-placed wait: the ids and the GMF rows are "used" here, so that the compiler places ITS wait for them
  // in straight-line code where it can count the stores behind them, instead of a vmcnt(0) at the loop header (which
  // is reached from two paths with different stores in flight)
  auto arrived = [&]() {
    asm volatile("" : "+v"(idu), "+v"(idi), "+v"(gu[0]), "+v"(gu[1]), "+v"(gu[2]), "+v"(gu[3]), "+v"(gi[0]), "+v"(gi[1]),
                      "+v"(gi[2]), "+v"(gi[3]));
  };
  // operand of table t, input block j: row n, chunk (4j + q) ^ n
  auto staged = [&](int t, int j) {
    return *reinterpret_cast<const f32x4*>(stage + (t * 16 + n) * 64 + 4 * ((4 * j + q) ^ n));
  };
  int stamp = 0;
  (void)stamp;
  STAMP(0, stamp++);
  issue_ids(wave0);
  {
    f32x4 wv[kFStagePer];
    int wdst[kFStagePer];
    float bv;
    stage_forward_load(T, wv, wdst, bv);
    float hw = 0.0f;
    if (threadIdx.x <= kHeadW) hw = F.wfold[threadIdx.x];
    issue_rows(wave0);                 // (waits for the ids alone: loads return in order)
    issue_ids(wave0 + nwaves);
    stage_forward_store(s_w, s_b, wv, wdst, bv);
    if (threadIdx.x <= kHeadW) s_hw[threadIdx.x] = hw;
  }
  __syncthreads();
  STAMP(0, stamp++);
  const float hc = s_hw[kHeadW];
  if (wave0 >= groups) return;
  const f32x4 hwn = *reinterpret_cast<const f32x4*>(s_hw + 4 * n);   // head weights of this lane's GMF columns
  // the first group's rows: everything issued so far (no stores yet)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  arrived();
  for (int64_t g = wave0; g < groups; g += nwaves) {
    const int64_t row = g * 16 + n;
    const int64_t srow = row < m ? row : m;             // lanes without a sample store to the spare row m
    // staged rows of g -> operands
    f32x4 a0[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 z = staged(0, j) + staged(1, j);
#pragma unroll
      for (int r = 0; r < 4; ++r) a0[j][r] = fmaxf(z[r], 0.0f);
    }
    // the head's GMF term: this lane's four columns of samples 4k + q, summed over the sixteen lanes of the row; the
    // sum of sample n is load n / 4 of quarter n % 4, and goes to the sample's four lanes by one shuffle
    float gdot = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 p = gu[k] * gi[k];
      float part = p[0] * hwn[0];
      part = fmaf(p[1], hwn[1], part); part = fmaf(p[2], hwn[2], part); part = fmaf(p[3], hwn[3], part);
      part = row_sum16(part);
      gdot = (n >> 2) == k ? part : gdot;
    }
    gdot = __shfl(gdot, ((n & 3) << 4) | n, 64);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stage is read: it may be overwritten
    STAMP(0, stamp++);
    issue_rows(g + nwaves);
    issue_ids(g + 2 * nwaves);
    STAMP(0, stamp++);
    f32x4 y1[2], y2[1], y3[1];
    layer_fwd<0, 4>(s_w, s_b, lane, q, a0, y1);
    layer_fwd<1, 2>(s_w, s_b, lane, q, y1, y2);
    layer_fwd<2, 1>(s_w, s_b, lane, q, y2, y3);
    STAMP(0, stamp++);
    // y1 and y2 (192 of a sample's 224 bytes; 12.6 MB a step at batch 65536) are written THROUGH the L2, as ncfp_bwd
    // writes its gz0 rows: the forward is 0.4-0.6 us shorter for it and the backward, which fetches them a group ahead
    // of their use, no longer (profiles/ncf_store_policy.txt).  y3 keeps its plain store: its upper half-wave parks
    // at the spare row m, which no 32-bit offset from the group's first row reaches.
    if constexpr (kNear) {
      const uint32_t lrow = (uint32_t)(srow - g * 16);    // (the spare row: at most fifteen behind the group's first)
      const auto wy1 = wt_window(T.y[0] + g * 16 * T.ldy[0]), wy2 = wt_window(T.y[1] + g * 16 * T.ldy[1]);
#pragma unroll
      for (int b = 0; b < 2; ++b) stg4_wt(wy1, (lrow * (uint32_t)T.ldy[0] + 16 * b + 4 * q) * 4u, y1[b]);
      stg4_wt(wy2, (lrow * (uint32_t)T.ldy[1] + 4 * q) * 4u, y2[0]);
    } else {
#pragma unroll
      for (int b = 0; b < 2; ++b) stg4(T.y[0] + srow * T.ldy[0] + 16 * b + 4 * q, y1[b]);
      stg4(T.y[1] + srow * T.ldy[1] + 4 * q, y2[0]);
    }
    stg4(T.y[2] + (q < 2 ? srow : m) * T.ldy[2] + 4 * (q & 1), y3[0]);
    // head: prob = act([gmf | h] . wfold + cfold); lanes q < 2 of a sample hold four terms of h each
    float dot;
    {
      const f32x4 wv = *reinterpret_cast<const f32x4*>(s_hw + kP + 4 * (q & 1));
      float d2 = y3[0][0] * wv[0];
      d2 = fmaf(y3[0][1], wv[1], d2); d2 = fmaf(y3[0][2], wv[2], d2); d2 = fmaf(y3[0][3], wv[3], d2);
      dot = q < 2 ? d2 : 0.0f;
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    F.out[srow * F.ldout] = ctr_act(gdot + dot + hc, F.act);   // (the four lanes of a sample agree)
    STAMP(0, stamp++);
    // the next group's rows and its successor's ids are older than this group's kFwdStores stores
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kFwdStores) : "memory");
    arrived();
  }
}

// ------------------------------------------------------------------ backward, per sample
// slab a workgroup leaves in the workspace, in the order its lanes hold the sums (coalesced 16-byte stores; the second
// pass, slab_reduce_role, does the index arithmetic once per output instead of every workgroup once per element):
//   [vector v][lane][register r]: dW accumulator vectors  v < 8: layer 0 block (v / 4, v % 4);  8, 9: layer 1;  10: layer 2
//   (register r of lane (q, lo) = row 16 b + 4 q + r, column 16 j + lo of its layer's weight gradient)
//   then kSmall sums: layer-0 bias (32), layer-1 bias (16), layer-2 bias (8), sum gz * h (8), sum gz (1), and in the
//   loss-fused mode the sum of the samples' BCE terms (1, word 65; zero otherwise)
// (the GMF part of the head's weight gradient comes from the table rows, ncfp_finish)
constexpr int slab_w(int l) {
  int o = 0;
  for (int i = 0; i < l; ++i) o += kN[i] * kK[i] + kN[i];
  return o;
}
constexpr int kSlabHead = slab_w(kL);                     // 2744 tower outputs: [dW_l | db_l] for the three layers
constexpr int kVecs = 8 + 2 + 1;                          // dW accumulator vectors of a lane
constexpr int kSmall = 32 + 16 + 8 + 8 + 1;               // bias sums, sum gz * h, sum gz
constexpr int kCopy = kVecs * 256 + 68;                   // one wave's sums parked in LDS (16-byte multiple)
constexpr int kSlabLoss = kVecs * 256 + 65;               // the first of the three spare words behind the kSmall sums
constexpr int kSlab = kCopy;                              // 2884
constexpr int kStripP = 3 * kTile;                        // per wave: tiles A0 A1 | B0
// the staged operands of a sample group (floats, per wave): sixteen rows each of P_U, P_I, Y1, Y2, Y3 -- fetched
// coalesced by LDS-DMA, 16-byte chunks XOR-swizzled with the row so that both read patterns (sample-major ds_read_b128,
// unit-major ds_read_b32) spread over the banks
constexpr int kSgPU = 0, kSgPI = 1024, kSgY1 = 2048, kSgY2 = 2560, kSgY3 = 2816, kBwdStage = 3072;
// dynamic LDS of ncfp_bwd_kernel (floats): tower weights, per-wave tiles and staging; the wave sums parked at the end
// (kCopy per wave) reuse the same space
constexpr int kBwdLdsFloats = kWFloats + kWaves * (kStripP + kBwdStage) > kWaves * kCopy ? kWFloats + kWaves * (kStripP + kBwdStage)
                                                                                         : kWaves * kCopy;
constexpr int kBwdDma = 12;                               // row fetches per group
constexpr int kBwdStores = 6;                             // 4 pieces of the gz0 row + 2 slot records

struct Bwd {
  Ids ids;
  const float* ptab;
  const float* wfold;
  const float* prob; int64_t ldp;
  const float* gprob; int64_t ldgp;            // kLoss: the TARGET and its stride -- the gradient is formed here
  int act;
  const int32_t* base;                         // the forward's plan: [chunk][row] slot of the row's first sample of the chunk,
  int shift;                                   // chunk of sample s = s >> shift
  const int32_t* ranks;                        // (m + 1, 2): rank of a sample inside (row, chunk)
  float* gz;                                   // (m + 1, 64): gz0 rows in sample order, one spare row
  float* aux;                                  // (2m + 1, 4): {gz, partner id, row, sample} per slot, user rows' slots
                                               // first, one spare slot
  float* slabs;                                // (grid, kSlab)
  float* zero_a; int64_t zero_a_floats;        // cleared first: the segment sums (nu + ni, 128)
  float* zero_b; int64_t zero_b_floats;        // cleared first (nullable): the step's gradient buffer
};

__device__ __forceinline__ int sw1(int r) { return (r >> 1) & 7; }   // chunk swizzles of the 128 / 64 / 32-byte rows
__device__ __forceinline__ int sw2(int r) { return (r >> 2) & 3; }
__device__ __forceinline__ int sw3(int r) { return (r >> 3) & 1; }

// kLoss: the binary cross entropy of (prob, target) and its gradient for an upstream of exactly 1 are formed HERE
// instead of by a launch of their own in front of this one (bce_fwd_kernel, csrc/train_step.hip: the same expressions,
// so the gradient has the same bits): the per-sample scalar load that fetches gprob fetches the target instead -- the
// number and order of vector-memory operations per group, and with them the hand-placed waits, are the same in both
// instantiations -- and one lane per sample sums the loss terms, which leave through word kSlabLoss of the slab; the
// slab second pass (slab_reduce_role) adds them over the workgroups in its fixed order and stores the mean.
template <bool kLoss>
__global__ void __launch_bounds__(kThreads)
ncfp_bwd_kernel(const Tower T, int64_t m, const Bwd B) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ __attribute__((aligned(16))) float s_hw[kHeadW + 4];
  float* s_wt = lds;
  const int lane = threadIdx.x & 63, q = lane >> 4, lo = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* tA = lds + kWFloats + wave * kStripP;
  float* tB = tA + 2 * kTile;
  float* stage = lds + kWFloats + kWaves * kStripP + wave * kBwdStage;
  const uint32_t stage_addr = ctr_lds_addr(stage);
  const int64_t nrows = B.ids.nu + B.ids.ni;
  const int64_t groups = (m + 15) / 16;
  const int64_t wave0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * kThreads) >> 6;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float* pu = B.ptab;
  const float* pi = B.ptab + B.ids.nu * kN0;
  const uint32_t nu = (uint32_t)B.ids.nu, ni = (uint32_t)B.ids.ni;
  int stamp = 0;
  (void)stamp;
  STAMP(1, stamp++);

  // ---- clear what this call accumulates into (both 16-byte aligned multiples of 4 floats)
  // (issued behind the group loop instead, in front of the last wait, they made the launch 0.9 us LONGER:
  // profiles/r07_ncf_plan_blocks.txt section 3)
  {
    const int64_t t0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4, step = (int64_t)gridDim.x * kThreads * 4;
    for (int64_t i = t0; i < B.zero_a_floats; i += step) stg4(B.zero_a + i, zero4);
    if (B.zero_b)
      for (int64_t i = t0; i < B.zero_b_floats; i += step) stg4(B.zero_b + i, zero4);
  }
  // ---- the fetch pipeline (see the note above ncfp_fwd_kernel).  Stage 1: the ids of this lane's sample (sample lo of
  // the group, the same in its four lanes).  Stage 2: the group's rows by LDS-DMA and the per-sample scalars.
  int64_t idu = 0, idi = 0;
  auto issue_ids = [&](int64_t g) {
    int64_t row = g * 16 + lo;
    row = row < m ? row : m - 1;
    idu = B.ids.uidx[row * B.ids.ustride];
    idi = B.ids.iidx[row * B.ids.istride];
  };
  struct Scal {
    float gp, pb;
    int ru, ri;                       // ranks of this lane's sample in its user / item row, inside its chunk,
    int bu, bi;                       // and the slots of those rows' first samples of the chunk
    uint32_t u, i;                    // its ids, clamped (bad ids: row 0, no slot)
    bool ubad, ibad;
  };
  auto issue_rows = [&](int64_t g, Scal& r) {
    int64_t rc = g * 16 + lo;
    rc = rc < m ? rc : m - 1;
    r.ubad = (uint64_t)idu >= nu;
    r.ibad = (uint64_t)idi >= ni;
    r.u = r.ubad ? 0u : (uint32_t)idu;
    r.i = r.ibad ? 0u : (uint32_t)idi;
    // P_U / P_I: instruction k moves rows 4k .. 4k+3, lane l chunk (l % 16) ^ row of row 4k + l / 16
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = 4 * k + q;
      const int src = (lane & 48) | row;                   // a lane of this quarter that holds sample row's ids
      const uint32_t ur = (uint32_t)__shfl((int)r.u, src, 64), ir = (uint32_t)__shfl((int)r.i, src, 64);
      const uint32_t col = 4u * (uint32_t)(lo ^ row);
      ctr_dma16(pu + ur * 64u + col, stage_addr + (uint32_t)((kSgPU + 4 * k * 64) * 4));
      ctr_dma16(pi + ir * 64u + col, stage_addr + (uint32_t)((kSgPI + 4 * k * 64) * 4));
    }
    {
      // Y1 (32 floats a row): instruction k moves rows 8k .. 8k+7, lane l chunk (l % 8) ^ sw1(row) of row 8k + l / 8
      const int64_t g16 = g * 16;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int row = 8 * k + (lane >> 3);
        int64_t gr = g16 + row;
        gr = gr < m ? gr : m - 1;
        ctr_dma16(T.y[0] + gr * T.ldy[0] + 4 * ((lane & 7) ^ sw1(row)), stage_addr + (uint32_t)((kSgY1 + 8 * k * 32) * 4));
      }
      {   // Y2 (16 floats): lane l chunk (l % 4) ^ sw2(row) of row l / 4
        const int row = lane >> 2;
        int64_t gr = g16 + row;
        gr = gr < m ? gr : m - 1;
        ctr_dma16(T.y[1] + gr * T.ldy[1] + 4 * ((lane & 3) ^ sw2(row)), stage_addr + (uint32_t)(kSgY2 * 4));
      }
      {   // Y3 (8 floats): lane l chunk (l % 2) ^ sw3(row) of row (l / 2) % 16 (the upper half-wave repeats the lower)
        const int row = (lane >> 1) & 15;
        int64_t gr = g16 + row;
        gr = gr < m ? gr : m - 1;
        ctr_dma16(T.y[2] + gr * T.ldy[2] + 4 * ((lane & 1) ^ sw3(row)), stage_addr + (uint32_t)(kSgY3 * 4));
      }
    }
    r.gp = B.gprob[rc * B.ldgp];      // (kLoss: the sample's target)
    r.pb = B.prob[rc * B.ldp];
    r.ru = B.ranks[2 * rc];
    r.ri = B.ranks[2 * rc + 1];
    const int32_t* bc = B.base + (rc >> B.shift) * nrows;
    r.bu = bc[r.u];
    r.bi = bc[nu + r.i];
  };
  Scal sc;
  // ---- what a lane sums over every group it walks
  f32x4 dw0[2][4], dw1[2], dw2;                // dW blocks: register r = row 4q + r, column lo
  f32x4 sb0[2], sb1, sb2, hy = zero4;          // bias sums of this lane's sample: units 4q + r
  float hc = 0.0f;
  float lc = 0.0f;                             // kLoss: the loss terms of this lane's samples (q == 0 alone)
  const float inv_n = 1.0f / (float)m;         // (as ctr_bce_fwd forms it on the host: a correctly rounded quotient)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    sb0[b] = zero4;
    dw1[b] = zero4;
#pragma unroll
    for (int j = 0; j < 4; ++j) dw0[b][j] = zero4;
  }
  sb1 = sb2 = dw2 = zero4;
  issue_ids(wave0);
  {
    f32x4 wv[kStagePer];
    int wdst[kStagePer];
    stage_transposed_load(T, wv, wdst);
    const float hw = threadIdx.x <= kHeadW ? B.wfold[threadIdx.x] : 0.0f;
    issue_rows(wave0, sc);
    issue_ids(wave0 + nwaves);
    stage_transposed_store(s_wt, wv, wdst);
    if (threadIdx.x <= kHeadW) s_hw[threadIdx.x] = hw;
  }
  __syncthreads();
  STAMP(1, stamp++);   // weights staged, first group requested
  // the first group's rows and scalars, the second group's ids (nothing else is in flight)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(idu), "+v"(idi), "+v"(sc.gp), "+v"(sc.pb), "+v"(sc.ru), "+v"(sc.ri), "+v"(sc.bu), "+v"(sc.bi));

  for (int64_t g = wave0; g < groups; g += nwaves) {
    const bool live = g * 16 + lo < m;
    // ---- staged rows of g -> operands
    float gp = kLoss ? 0.0f : live ? sc.gp : 0.0f;           // a dead lane's gz is zero: it adds nothing anywhere
    const float yv = sc.gp;                                  // (kLoss: what that load brought is the target)
    const float pb = sc.pb;
    f32x4 y3d, y2d, y2t, y1d[2], y1t[2], a0d[4], a0t[4];
    y3d = *reinterpret_cast<const f32x4*>(stage + kSgY3 + lo * 8 + 4 * ((q & 1) ^ sw3(lo)));
    y3d = q < 2 ? y3d : zero4;
    y2d = *reinterpret_cast<const f32x4*>(stage + kSgY2 + lo * 16 + 4 * (q ^ sw2(lo)));
#pragma unroll
    for (int b = 0; b < 2; ++b) y1d[b] = *reinterpret_cast<const f32x4*>(stage + kSgY1 + lo * 32 + 4 * ((4 * b + q) ^ sw1(lo)));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int at = lo * 64 + 4 * ((4 * j + q) ^ lo);
      const f32x4 z = *reinterpret_cast<const f32x4*>(stage + kSgPU + at) + *reinterpret_cast<const f32x4*>(stage + kSgPI + at);
#pragma unroll
      for (int r = 0; r < 4; ++r) a0d[j][r] = fmaxf(z[r], 0.0f);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int row = 4 * q + c, ch = lo >> 2, w = lo & 3;
      y2t[c] = stage[kSgY2 + row * 16 + 4 * (ch ^ sw2(row)) + w];
#pragma unroll
      for (int b = 0; b < 2; ++b) y1t[b][c] = stage[kSgY1 + row * 32 + 4 * ((4 * b + ch) ^ sw1(row)) + w];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int at = row * 64 + 4 * ((4 * j + ch) ^ row) + w;
        a0t[j][c] = fmaxf(stage[kSgPU + at] + stage[kSgPI + at], 0.0f);
      }
    }
    const int uu = (int)sc.u, ii = (int)sc.i;
    const int su = (live && !sc.ubad && sc.ru >= 0) ? sc.ru + sc.bu : -1;
    const int si = (live && !sc.ibad && sc.ri >= 0) ? sc.ri + sc.bi : -1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the stage is read: it may be overwritten
    STAMP(1, stamp++);   // operands read
    issue_rows(g + nwaves, sc);
    issue_ids(g + 2 * nwaves);
    STAMP(1, stamp++);   // next group requested
    // ---- head: gz, the head's sums, the tower's (masked) gY
    if constexpr (kLoss) {
      // bce_fwd_kernel's expressions on (prob, target), behind the requests so that they run under the fetches; a sample
      // with an id outside its table has a prob, and counts
      const float lp = fmaxf(logf(pb), -100.0f), l1p = fmaxf(logf(1.0f - pb), -100.0f);
      if (q == 0 && live) lc -= yv * lp + (1.0f - yv) * l1p;
      gp = live ? (pb - yv) / fmaxf((1.0f - pb) * pb, 1e-12f) * inv_n : 0.0f;
    }
    const float gzs = gp * ctr_act_grad(pb, B.act);
    if (q == 0) hc += gzs;
    f32x4 gz3[1];
    {
      const f32x4 wv = q < 2 ? *reinterpret_cast<const f32x4*>(s_hw + kP + 4 * q) : zero4;
      hy += gzs * y3d;                                        // (y3d is zero for q >= 2)
      gz3[0] = relu_mask(gzs * wv, y3d);
    }
    sb2 += gz3[0];
    tiles_put<1>(tA, q, lo, gz3);
    f32x4 w0 = zero4, w1 = zero4;
    dx_first<2>(s_wt, lane, w0, w1);
    // ---- layer 2 (16 -> 8)
    f32x4 gz2[1];
    {
      f32x4 tg[1];
      tiles_get<1>(tA, q, lo, tg);
      dx_layer<2, 1>(s_wt, lane, gz3, w0, w1, [&](int, const f32x4& d0, const f32x4&) { gz2[0] = relu_mask(d0, y2d); });
      sb1 += gz2[0];
      tiles_put<1>(tB, q, lo, gz2);
      dx_first<1>(s_wt, lane, w0, w1);
#pragma unroll
      for (int c = 0; c < 4; ++c) dw2 = __builtin_amdgcn_mfma_f32_16x16x4f32(tg[0][c], y2t[c], dw2, 0, 0, 0);
    }
    // ---- layer 1 (32 -> 16)
    f32x4 gz1[2];
    {
      f32x4 tg[1];
      tiles_get<1>(tB, q, lo, tg);
      dx_layer<1, 1>(s_wt, lane, gz2, w0, w1, [&](int, const f32x4& d0, const f32x4& d1) {
        gz1[0] = relu_mask(d0, y1d[0]);
        gz1[1] = relu_mask(d1, y1d[1]);
      });
#pragma unroll
      for (int b = 0; b < 2; ++b) sb0[b] += gz1[b];
      tiles_put<2>(tA, q, lo, gz1);
      dx_first<0>(s_wt, lane, w0, w1);
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j) dw1[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(tg[0][c], y1t[j][c], dw1[j], 0, 0, 0);
    }
    STAMP(1, stamp++);   // head + layers 2, 1 done
    // ---- layer 0 (64 -> 32): its input gradient, masked by relu'(z0), IS gz0 -- stored once, at the sample's own row
    {
      f32x4 tg[2];
      tiles_get<2>(tA, q, lo, tg);
      // row b of the sample-ordered buffer (a group's sixteen rows are 4 KB in a piece); a padding lane writes the spare row m
      // (only the last group has padding lanes, so the spare row is at most fifteen rows behind the group's first).
      // Written THROUGH the L2: 16.8 MB a step at batch 65536 that nothing reads before ncfp_segsum gathers it from
      // all eight XCDs; left dirty they were written back after the last wave had retired, with nothing running beside
      // (profiles/ncf_store_policy.txt: the launch 0.9-1.1 us shorter, a wave's own life unchanged)
      const int brow = (int)(live ? g * 16 + lo : m);
      const auto wz = wt_window(B.gz + g * 16 * kN0);
      const uint32_t dz = (uint32_t)((brow - (int)(g * 16)) * kN0 + 4 * q) * 4u;
      dx_layer<0, 2>(s_wt, lane, gz1, w0, w1, [&](int j, const f32x4& d0, const f32x4& d1) {
        stg4_wt(wz, dz + 64u * j, relu_mask(d0, a0d[j]));
        stg4_wt(wz, dz + 64u * (j + 1), relu_mask(d1, a0d[j + 1]));
      });
      // the sample's two slot records name its row; a sample without a slot (bad id, padding lane) writes the spare slot
      // behind the records (the four lanes of a sample write the same record: an unconditional, countable store)
      stg4(B.aux + (int64_t)(su >= 0 ? su : 2 * m) * 4,
           f32x4{gzs, __int_as_float(ii), __int_as_float(uu), __int_as_float(brow)});
      stg4(B.aux + (int64_t)(si >= 0 ? si : 2 * m) * 4,
           f32x4{gzs, __int_as_float(uu), __int_as_float((int)nu + ii), __int_as_float(brow)});
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            dw0[b][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(tg[b][c], a0t[j][c], dw0[b][j], 0, 0, 0);
    }
    STAMP(1, stamp++);   // layer 0 done
    // the next group's rows, scalars and its successor's ids are older than this group's kBwdStores stores
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kBwdStores) : "memory");
    asm volatile("" : "+v"(idu), "+v"(idi), "+v"(sc.gp), "+v"(sc.pb), "+v"(sc.ru), "+v"(sc.ri), "+v"(sc.bu), "+v"(sc.bi));
  }

  // ---- the workgroup's partial: every wave parks its sums (weights, tiles and stages are dead), the four copies are
  // summed on the way out
  STAMP(1, stamp++);   // loop end
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (row fetches requested for a group past the end have landed)
  __syncthreads();
  {
    auto rsum = [&](const f32x4& v) {
      f32x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = row_sum16(v[r]);
      return o;
    };
    float* copy = lds + wave * kCopy;
    float* small = copy + kVecs * 256;
    auto vec = [&](int v) -> const f32x4& { return v < 8 ? dw0[v >> 2][v & 3] : v < 10 ? dw1[v - 8] : dw2; };
#pragma unroll
    for (int v = 0; v < kVecs; ++v) *reinterpret_cast<f32x4*>(copy + (v * 64 + lane) * 4) = vec(v);
    const f32x4 s00 = rsum(sb0[0]), s01 = rsum(sb0[1]), s1 = rsum(sb1), s2 = rsum(sb2), shy = rsum(hy);
    const float vc = row_sum16(hc);
    const float vl = kLoss ? row_sum16(lc) : 0.0f;
    if (lo == 0) {
      *reinterpret_cast<f32x4*>(small + 4 * q) = s00;              // layer 0 bias sums: units 4q .. (block 0)
      *reinterpret_cast<f32x4*>(small + 16 + 4 * q) = s01;         //                     16 + 4q ..
      *reinterpret_cast<f32x4*>(small + 32 + 4 * q) = s1;          // layer 1: 16 units
      if (q < 2) {
        *reinterpret_cast<f32x4*>(small + 48 + 4 * q) = s2;        // layer 2: 8 units
        *reinterpret_cast<f32x4*>(small + 56 + 4 * q) = shy;       // sum gz * h: 8
      }
    }
    if (lane == 0) {
      small[64] = vc;
      small[65] = vl;
      small[66] = small[67] = 0.0f;
    }
  }
  __syncthreads();
  float* out = B.slabs + (int64_t)blockIdx.x * kSlab;
  for (int i = threadIdx.x; i < kCopy / 4; i += kThreads) {
    const f32x4 t = (*reinterpret_cast<const f32x4*>(lds + 4 * i) + *reinterpret_cast<const f32x4*>(lds + kCopy + 4 * i)) +
                    (*reinterpret_cast<const f32x4*>(lds + 2 * kCopy + 4 * i) + *reinterpret_cast<const f32x4*>(lds + 3 * kCopy + 4 * i));
    stg4(out + 4 * i, t);
  }
  STAMP(1, stamp++);   // slab written
}

// ------------------------------------------------------------------ segment sums over the buckets
// ST[v] = [ S[v] (64) | T[v] (64) ],  S[v] = sum of the gz0 rows in row v's bucket,  T[v] = sum gz_b * partner row.
// A lane group of sixteen owns sixteen consecutive SLOTS, whatever rows they belong to: equal work per wave under any
// id distribution.  Every load of the group is requested before any is consumed -- the slot records, one per lane,
// beside the number of slots in use (one round trip), then the sixteen bucket rows and the sixteen partner rows they
// name (a second one): a load-use loop over the slots was eight dependent round trips, 15 us for a kernel that moves
// 50 MB.  The group keeps running sums for the row it is in; a run that begins and ends inside the group is a whole
// bucket and is stored, a run that continues in a neighbouring group is parked in LDS, where the workgroup sums the
// chains of such runs: a chain inside the workgroup's 256 slots is stored as well, one that reaches its first or last
// slot is added to ST atomically, a thread per column (sixteen consecutive floats from sixteen lanes are one 64-byte
// atomic segment).  ncfp_bwd zeroes ST, so a row without a sample stays zero.
struct Seg {
  const float* gz; const float* aux; const int32_t* offsets;
  const float* gmf_u; const float* gmf_i;
  int64_t nu, ni, m;
  float* st;                                   // (nu + ni, 128), zeroed
};

// ------------------------------------------------------------------ the second pass over ncfp_bwd's slabs
// Two roles on workgroups of their own: the slab reduction (tower dW / db: 32 outputs x 8 part-lanes per workgroup,
// fixed order) and the head fold's chain rule from the slabs' head sums (ctr_fold_head_bwd's map without the GMF
// part).  Both only depend on ncfp_bwd and need no launch of their own.  They ride in front of ncfp_finish's
// workgroups: that launch is one short latency chain on fewer workgroups than the chip has CUs, so the 87 role
// workgroups get CUs of their own.  (They rode with the segment sums before, whose workgroups fill every CU several
// times over.  Measured, profiles/ncf_step_redeal.txt: segment sums 12.0 -> 10.7 us, ncfp_finish 8.1 -> 8.6 us,
// first or last in the grid -- and 8.5 with both roles returning at once: the price is the 87 workgroups themselves.)
struct Roles {
  int red_blocks;                              // by blockIdx.x: [0, red) slabs, red: fold
  const float* slabs; int parts;
  float* gw[kL]; float* gb[kL];                // tower gradients (+=)
  // head fold chain rule: u = linear2.weight (128), w / b = `linear` (64 x 8)
  const float* fold_u; const float* fold_w; int64_t fold_ldw; const float* fold_b;
  float* g_u; float* g_w; int64_t ld_g_w; float* g_b; float* g_b2;   // (+=), nullable
  float* loss; float inv_n;                    // nullable: the mean of the slabs' loss words is STORED here (loss-fused backward)
};

// float offset inside a slab of tower output e (e in the order [dW_l | db_l], l = 0..2)
__device__ __forceinline__ int slab_raw_of(int e) {
  int l = 0, r = e;
#pragma unroll
  for (int i = 0; i < kL; ++i)
    if (e >= slab_w(i)) { l = i; r = e - slab_w(i); }
  const int K = l == 0 ? kK[0] : l == 1 ? kK[1] : kK[2], N = l == 0 ? kN[0] : l == 1 ? kN[1] : kN[2];
  if (r >= N * K) return kVecs * 256 + (l == 0 ? 0 : l == 1 ? 32 : 48) + (r - N * K);   // bias sums
  const int row = r / K, col = r - row * K;
  const int J = K / 16, v0 = l == 0 ? 0 : l == 1 ? 8 : 10;
  const int v = v0 + (row >> 4) * J + (col >> 4);
  return (v * 64 + ((row >> 2) & 3) * 16 + (col & 15)) * 4 + (row & 3);
}

__device__ __forceinline__ void slab_reduce_role(const Roles& A, int blk) {
  // outputs [32 blk, 32 blk + 32) of the kSlabHead tower sums: lane (o, pl) adds every 8th partial, 8 loads in flight.
  // The last block has spare outputs: the first of them, e == kSlabHead, is the loss of a loss-fused backward -- the
  // slabs' word kSlabLoss summed in the same fixed order, times 1 / batch, stored (not added) to the caller's word
  __shared__ float s_part[kWaves][32];
  const int o = threadIdx.x & 31, pl = threadIdx.x >> 5, wave = threadIdx.x >> 6;
  const int e = blk * 32 + o;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool is_loss = A.loss && e == kSlabHead;
  if (e < kSlabHead || is_loss) {
    const float* src = A.slabs + (is_loss ? kSlabLoss : slab_raw_of(e));
    int p = pl;
    for (; p + 7 * 8 < A.parts; p += 8 * 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += src[(int64_t)(p + 8 * u) * kSlab];
    }
    // the at most seven partials left: requested together from clamped indices, the ones past the end masked out (a load
    // inside the loop's condition was a round trip each)
    float tail[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) tail[u] = src[(int64_t)(p + 8 * u < A.parts ? p + 8 * u : A.parts - 1) * kSlab];
#pragma unroll
    for (int u = 0; u < 7; ++u) acc[0] += (p + 8 * u < A.parts ? 1.0f : 0.0f) * tail[u];
  }
  float t = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  t += __shfl_xor(t, 32, 64);
  if ((threadIdx.x & 63) < 32) s_part[wave][o] = t;
  __syncthreads();
  if (threadIdx.x < 32 && e < kSlabHead) {
    const float total = (s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o]);
    int l = 0, r = e;
#pragma unroll
    for (int i = 0; i < kL; ++i)
      if (e >= slab_w(i)) { l = i; r = e - slab_w(i); }
    const int wn = l == 0 ? kN[0] * kK[0] : l == 1 ? kN[1] * kK[1] : kN[2] * kK[2];
    float* dst = r < wn ? A.gw[l] + r : A.gb[l] + (r - wn);
    dst[0] += total;
  }
  if (threadIdx.x < 32 && is_loss) A.loss[0] = ((s_part[0][o] + s_part[1][o]) + (s_part[2][o] + s_part[3][o])) * A.inv_n;
}

__device__ __forceinline__ void head_fold_role(const Roles& A) {
  // nine columns (sum gz * h [8], sum gz) x 28 part-lanes: every load of a thread in flight at once
  __shared__ float s_p[28][12];
  __shared__ float s_g[12];
  const int col = threadIdx.x % 9, pl = threadIdx.x / 9;
  float acc = 0.0f;
  if (pl < 28) {
    const float* src = A.slabs + kVecs * 256 + 56 + col;
    float v[10];
#pragma unroll
    for (int u = 0; u < 10; ++u) v[u] = 0.0f;
    for (int p0 = pl; p0 < A.parts; p0 += 28 * 10) {
      // unconditional loads from clamped indices, masked afterwards: a load inside the condition is a round trip each
      float x[10];
#pragma unroll
      for (int u = 0; u < 10; ++u) x[u] = src[(int64_t)(p0 + 28 * u < A.parts ? p0 + 28 * u : A.parts - 1) * kSlab];
#pragma unroll
      for (int u = 0; u < 10; ++u) v[u] += (p0 + 28 * u < A.parts ? 1.0f : 0.0f) * x[u];
    }
#pragma unroll
    for (int u = 0; u < 10; ++u) acc += v[u];
    s_p[pl][col] = acc;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    float t = 0.0f;
    for (int i = 0; i < 28; ++i) t += s_p[i][threadIdx.x];
    s_g[threadIdx.x] = t;
  }
  __syncthreads();
  const float* u = A.fold_u + kP;
  const float gc = s_g[kNL];
  for (int t = threadIdx.x; t < 64 * kNL; t += kThreads) {            // g `linear`.weight[i][q] += u[64 + i] * hy[q]
    const int i = t / kNL, q = t % kNL;
    if (A.g_w) A.g_w[(int64_t)i * A.ld_g_w + q] += u[i] * s_g[q];
  }
  if (threadIdx.x < 64) {
    const int i = threadIdx.x;
    if (A.g_u) {                                                      // g linear2.weight[64 + i]
      float sacc = A.fold_b ? A.fold_b[i] * gc : 0.0f;
#pragma unroll
      for (int q = 0; q < kNL; ++q) sacc = fmaf(A.fold_w[(int64_t)i * A.fold_ldw + q], s_g[q], sacc);
      A.g_u[kP + i] += sacc;
    }
    if (A.g_b) A.g_b[i] += u[i] * gc;
  }
  if (threadIdx.x == 64 && A.g_b2) A.g_b2[0] += gc;
}

constexpr int kSegSlots = 16;                        // consecutive slots a lane group of sixteen owns: all in flight at once
constexpr int kSegGroups = kThreads / 16;            // lane groups of a workgroup
constexpr int kSegWgSlots = kSegGroups * kSegSlots;  // consecutive slots of a workgroup
constexpr int kSegOpenL = 1, kSegOpenR = 2;          // a parked run continues in the group before / behind

__global__ void __launch_bounds__(kThreads, 3)
ncfp_segsum_kernel(const Seg A) {
  // The chain of a wave is {total || records} -> rows -> sums: lane lo of a group loads the record of slot s0 + lo (the
  // group's records are 256 contiguous bytes) beside the number of slots in use, the fields of slot k reach the other
  // lanes by a shuffle inside the sixteen, and the 32 row loads (gz0 row + partner row of every slot) are requested back
  // to back before any is consumed.  (The version before walked 32 slots 8 at a time behind offsets[rows] -- six
  // dependent round trips at one wave per SIMD, every lane of a group holding a copy of every record.)
  //
  // A run that begins and ends inside the group is the whole bucket of its row: plain stores.  A run that continues in a
  // neighbouring group -- the first when the slot before the range has its row, the last when the slot behind has -- is
  // OPEN: the group parks it in LDS (two entries a group: an open first run that ends inside, and the last run), and
  // after one barrier a thread per column walks the workgroup's entries in slot order, sums the chains of entries that
  // continue each other, stores a chain that lies inside the workgroup and adds one that is open at the workgroup's
  // first or last slot to ST atomically (64-byte segments from sixteen lanes): at most two atomic flushes per 256 slots.
  // (Two per 32-slot range went out at the end of the waves with nothing else in flight: 4.2 MB at the memory side's
  // atomic rate.)
  __shared__ __attribute__((aligned(16))) float s_run[2 * kSegGroups][128];
  __shared__ int s_meta[2 * kSegGroups];             // row << 2 | open flags; -1: no entry
  const int lane = threadIdx.x & 63, lo = lane & 15, grp = threadIdx.x >> 4;
  const int64_t s0 = ((int64_t)blockIdx.x * kSegGroups + grp) * kSegSlots, sme = s0 + lo;
  const int64_t spare = 2 * A.m;                     // the last slot of the record array: every index is clamped to it
  // ---- requests: the slots in use, this lane's record, the rows of the slots just outside the range
  const int64_t total = A.offsets[A.nu + A.ni];
  const f32x4 rec = ldg4(A.aux + (sme < spare ? sme : spare) * 4);
  const int64_t sb = s0 > 0 ? s0 - 1 : 0, sa = s0 + kSegSlots;
  const int row_before = __float_as_int(A.aux[(sb < spare ? sb : spare) * 4 + 2]);
  const int row_after = __float_as_int(A.aux[(sa < spare ? sa : spare) * 4 + 2]);
  // a slot at or behind `total` holds stale bytes of an earlier step: nothing is addressed through it, it joins no sum
  const bool used = sme < total;
  const float gzv = used ? rec[0] : 0.0f;
  const int v = used && (uint32_t)__float_as_int(rec[2]) < (uint32_t)(A.nu + A.ni) ? __float_as_int(rec[2]) : -1;
  const bool urow = v < A.nu;                        // a user row: its partners are items
  // (clamped: records of a call that broke the counters' contract give wrong sums, not a read outside a buffer)
  const uint32_t pid = used ? min((uint32_t)__float_as_int(rec[1]), (uint32_t)((urow ? A.ni : A.nu) - 1)) : 0u;
  const int pk = (int)(2u * pid + (urow ? 1u : 0u));
  const uint32_t b = used ? min((uint32_t)__float_as_int(rec[3]), (uint32_t)A.m) : (uint32_t)A.m;
  const int v_before = (s0 > 0 && s0 - 1 < total) ? row_before : -1;
  const int v_after = sa < total ? row_after : -1;
  // ---- the 32 rows of the range, 16 bytes per lane each
  f32x4 g[kSegSlots], p[kSegSlots];
#pragma unroll
  for (int k = 0; k < kSegSlots; ++k) {
    const int src = (lane & 48) | k;
    const uint32_t bk = (uint32_t)__shfl((int)b, src, 64);
    const int pkk = __shfl(pk, src, 64);
    g[k] = ldg4(A.gz + (int64_t)bk * kN0 + 4 * lo);
    p[k] = ldg4(((pkk & 1) ? A.gmf_i : A.gmf_u) + (int64_t)(pkk >> 1) * kP + 4 * lo);
  }
  // ---- the runs, in slot order (every lane of the group takes the same turns: it holds columns 4 lo .. 4 lo + 3)
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 accs = zero4, acct = zero4;
  int cur = -1;
  bool inside = false;   // the run being summed began inside this range (its row's bucket does not start earlier)
  int meta0 = -1, meta1 = -1;
  auto store_run = [&](int r) {
    float* dst = A.st + (int64_t)r * 128;
    stg4(dst + 4 * lo, accs);
    stg4(dst + 64 + 4 * lo, acct);
  };
  auto park = [&](int e) {
    *reinterpret_cast<f32x4*>(&s_run[2 * grp + e][4 * lo]) = accs;
    *reinterpret_cast<f32x4*>(&s_run[2 * grp + e][64 + 4 * lo]) = acct;
  };
#pragma unroll
  for (int k = 0; k < kSegSlots; ++k) {
    const int src = (lane & 48) | k;
    const int vk = __shfl(v, src, 64);
    const float gk = __shfl(gzv, src, 64);
    if (vk != cur) {
      if (cur >= 0) {                                // it ended here, inside the range
        if (inside) store_run(cur);
        else {
          park(0);
          meta0 = (cur << 2) | kSegOpenL;
        }
      }
      inside = k > 0 || vk != v_before;
      cur = vk;
      accs = acct = zero4;
    }
    accs += g[k];
    acct += gk * p[k];
  }
  if (cur >= 0) {
    const bool open_r = cur == v_after;
    if (inside && !open_r) store_run(cur);
    else {
      park(1);
      meta1 = (cur << 2) | (inside ? 0 : kSegOpenL) | (open_r ? kSegOpenR : 0);
    }
  }
  if (lo == 0) {
    s_meta[2 * grp] = meta0;
    s_meta[2 * grp + 1] = meta1;
  }
  __syncthreads();
  // ---- the open runs of the workgroup, a thread per column.  An entry open to the right is continued by the first
  // entry of the next group (same row, open to the left); a chain that reaches the workgroup's first or last slot open
  // may go on in another workgroup
  if (threadIdx.x >= 128) return;
  const int c = threadIdx.x;
  float sum = 0.0f;
  int row = -1;
  bool shared = false;
  auto emit = [&](bool atomic) {
    float* dst = A.st + (int64_t)row * 128 + c;
    if (atomic) ctr_atomic_add_global(dst, sum);
    else dst[0] = sum;
    row = -1;
  };
  // (every entry is read before the first is looked at, empty ones included: one LDS round trip, not one per entry)
  int meta[2 * kSegGroups];
  float val[2 * kSegGroups];
#pragma unroll
  for (int e = 0; e < 2 * kSegGroups; ++e) {
    meta[e] = s_meta[e];
    val[e] = s_run[e][c];
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int e = 0; e < 2 * kSegGroups; ++e) {
    const int mt = __builtin_amdgcn_readfirstlane(meta[e]);
    const float x = val[e];
    if (mt >= 0) {
      const int r = mt >> 2;
      if (row >= 0 && r != row) emit(true);          // (never, for records that keep the contract)
      if (row < 0) {
        row = r;
        sum = 0.0f;
        shared = (mt & kSegOpenL) != 0;              // open to the left with nothing before it here: the workgroup's edge
      }
      sum += x;
      if (!(mt & kSegOpenR)) emit(shared);
    }
  }
  if (row >= 0) emit(true);                          // still open at the workgroup's last slot
}

// ------------------------------------------------------------------ the products over the table rows
// Per sixteen rows of one table:  dMLP[rows] += S . W0half,  dGMF[rows] += wf * T,  and the rows' share of
// dW0half += S^T . MLP,  db0 += column sums of S (user rows),  g_head_w[:64] += sum_rows GMF * T (user rows).
// These pieces do not depend on each other, and the launch is as long as the longest chain one wave runs (a few
// thousand table rows are a fraction of the chip): the grid is kFinParts copies of the row blocks, and a workgroup
// (four waves = four row blocks of the same table) runs ONE piece for them:
//   parts 0, 1 (h = part):      dW0half for the units [32h, 32h + 32) -- the four waves meet in LDS, one atomic per element
//                               and workgroup goes out (splitting by UNITS leaves the number of atomics a line of g_w0
//                               receives where it was; splitting by rows would multiply it) -- and, h = 0, the small sums
//   parts 2, 3 (h = part - 2):  dMLP for the inputs [32h, 32h + 32) and dGMF for the columns of blocks 2h, 2h + 1: plain
//                               read-modify-write of rows nobody else touches, no LDS, no atomics
// Every operand of a piece is requested before any is consumed: they are independent of each other, and a load-use order
// was eight dependent round trips (unconditional loads from a clamped row, zeroed afterwards: a load inside a
// conditional is a round trip of its own).
struct Fin {
  const float* st;                             // (nu + ni, 128)
  const float* mlp_u; const float* mlp_i; const float* gmf_u; const float* gmf_i;
  const float* w0; int64_t ldw0;
  const float* wfold;
  int64_t nu, ni;
  float* g_mlp_u; float* g_mlp_i; float* g_gmf_u; float* g_gmf_i;   // (+=), nullable
  float* g_w0; int64_t ldgw0; float* g_b0;                           // (+=), nullable
  float* g_head;                                                     // g of linear2.weight[:64] (+=), nullable
  int wgs;                                                           // workgroups of one part
  Roles roles;                                 // dispatched first: gridDim.x = roles.red_blocks + 1 + kFinParts * wgs
};
constexpr int kFinParts = 4;

__global__ void __launch_bounds__(kThreads)
ncfp_finish_kernel(const Fin A) {
  if ((int)blockIdx.x <= A.roles.red_blocks) {
    if ((int)blockIdx.x < A.roles.red_blocks) slab_reduce_role(A.roles, (int)blockIdx.x);
    else head_fold_role(A.roles);
    return;
  }
  __shared__ __attribute__((aligned(16))) float s_dw[2][8 * 256];
  __shared__ float s_sm[kWaves][2][64];
  const int lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15, wave = threadIdx.x >> 6;
  const int fblk = (int)blockIdx.x - (A.roles.red_blocks + 1);
  const int part = fblk / A.wgs, wg = fblk - part * A.wgs, h = part & 1;
  const int64_t ublocks = (A.nu + 15) / 16, iblocks = (A.ni + 15) / 16;
  const int64_t uwgs = (ublocks + kWaves - 1) / kWaves;
  const bool user = wg < uwgs;
  const int64_t blk = (user ? (int64_t)wg : (int64_t)wg - uwgs) * kWaves + wave;
  const int64_t rows = user ? A.nu : A.ni, r0 = blk * 16;
  const bool any = blk < (user ? ublocks : iblocks);
  const float* st = A.st + (user ? 0 : A.nu) * 128;
  const float* tab = user ? A.mlp_u : A.mlp_i;
  const float* gmf = user ? A.gmf_u : A.gmf_i;
  float* gtab = user ? A.g_mlp_u : A.g_mlp_i;
  float* ggmf = user ? A.g_gmf_u : A.g_gmf_i;
  const int coff = user ? 0 : kH;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int64_t row = r0 + n;
  const bool live = any && row < rows;
  const int64_t crow = live ? row : rows - 1;
  const float keep = live ? 1.0f : 0.0f;

  if (part >= 2) {
    // ---- the rows' own gradients: inputs / columns of the blocks 2h, 2h + 1
    if (!any || (!gtab && !ggmf)) return;
    // sample-major operands: this lane's row n, columns 16j + 4q ..
    f32x4 sd[4], td[2], og[2], ot[2], wf[2];
    const float* ogp = ggmf ? ggmf : gmf;      // (a missing gradient buffer: read something valid, the store is skipped)
    const float* otp = gtab ? gtab : tab;
#pragma unroll
    for (int j = 0; j < 4; ++j) sd[j] = ldg4(st + crow * 128 + 16 * j + 4 * q);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 16 * (2 * h + e) + 4 * q;
      td[e] = ldg4(st + crow * 128 + 64 + col);
      og[e] = ldg4(ogp + crow * kP + col);
      ot[e] = ldg4(otp + crow * kH + col);
      wf[e] = ldg4(A.wfold + col);
    }
    // A operands of dMLP, unit-major: W0[16j + 4q + c][coff + 16b + n], b = 2h + e
    f32x4 wt[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) wt[j][e][c] = A.w0[(int64_t)(16 * j + 4 * q + c) * A.ldw0 + coff + 16 * (2 * h + e) + n];
    // dGMF[row] += wfold[:64] * T[row]
    if (ggmf && live) {
#pragma unroll
      for (int e = 0; e < 2; ++e) stg4(ggmf + row * kP + 16 * (2 * h + e) + 4 * q, og[e] + wf[e] * td[e]);
    }
    // dMLP^T (32 inputs x 16 rows) = W0half^T (32 x 64 units) . S^T (64 units x 16 rows)
    if (gtab) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sd[j] *= keep;
      f32x4 acc[2] = {ot[0], ot[1]};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int e = 0; e < 2; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[j][e][c], sd[j][c], acc[e], 0, 0, 0);
      if (live) {
#pragma unroll
        for (int e = 0; e < 2; ++e) stg4(gtab + row * kH + 16 * (2 * h + e) + 4 * q, acc[e]);
      }
    }
    return;
  }

  // ---- the sums over the rows: dW0half for the units of blocks 2h, 2h + 1; h = 0: db0 and the head's GMF weights
  const bool sums = h == 0 && user && (A.g_b0 || A.g_head);
  if (!A.g_w0 && !sums) return;
  f32x4 dw[2][4];
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int j = 0; j < 4; ++j) dw[e][j] = zero4;
  f32x4 colsum[4], gw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) colsum[j] = gw[j] = zero4;
  if (any) {
    f32x4 sd[4], td[4], gd[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sd[j] = ldg4(st + crow * 128 + 16 * j + 4 * q);
      td[j] = ldg4(st + crow * 128 + 64 + 16 * j + 4 * q);
      gd[j] = ldg4(gmf + crow * kP + 16 * j + 4 * q);
    }
    // unit-major operands: unit 16 (2h + e) + n / input 16j + n of rows 4q + c
    f32x4 stt[2], xt[4];
    float okc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t r = r0 + 4 * q + c;
      const int64_t rr = r < rows ? r : rows - 1;
      okc[c] = r < rows ? 1.0f : 0.0f;
#pragma unroll
      for (int e = 0; e < 2; ++e) stt[e][c] = st[rr * 128 + 16 * (2 * h + e) + n];
#pragma unroll
      for (int j = 0; j < 4; ++j) xt[j][c] = tab[rr * kH + 16 * j + n];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gw[j] = gd[j] * (td[j] * keep);
      colsum[j] = sd[j] * keep;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int c = 0; c < 4; ++c) stt[e][c] *= okc[c];
    // dW0half (32 units x 64 inputs) += S^T . X
    if (A.g_w0) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int j = 0; j < 4; ++j) dw[e][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(stt[e][c], xt[j][c], dw[e][j], 0, 0, 0);
    }
  }
  // ---- the workgroup's sums: waves 0 / 1 park their dW blocks, waves 2 / 3 add theirs in place (own lane slots)
  if (wave < 2) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(&s_dw[wave][((e * 4 + j) * 64 + lane) * 4]) = dw[e][j];
  }
  __syncthreads();
  if (wave >= 2) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4* at = reinterpret_cast<f32x4*>(&s_dw[wave - 2][((e * 4 + j) * 64 + lane) * 4]);
        *at = *at + dw[e][j];
      }
  }
  if (sums) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float cs = row_sum16(colsum[j][r]), gs = row_sum16(gw[j][r]);
        if (n == 0) {
          s_sm[wave][0][16 * j + 4 * q + r] = cs;
          s_sm[wave][1][16 * j + 4 * q + r] = gs;
        }
      }
  }
  __syncthreads();
  if (A.g_w0) {
    for (int e = threadIdx.x; e < 32 * 64; e += kThreads) {
      const int ul = e >> 6, k = e & 63, unit = 32 * h + ul;     // dW0[unit][coff + k]
      const int b = ul >> 4, qq = (ul >> 2) & 3, r = ul & 3, j = k >> 4, ll = k & 15;
      const int at = ((b * 4 + j) * 64 + qq * 16 + ll) * 4 + r;
      const float v = s_dw[0][at] + s_dw[1][at];
      ctr_atomic_add_global(A.g_w0 + (int64_t)unit * A.ldgw0 + coff + k, v);
    }
  }
  if (threadIdx.x < 64 && sums) {
    const int t = threadIdx.x;
    if (A.g_b0) ctr_atomic_add_global(A.g_b0 + t, (s_sm[0][0][t] + s_sm[1][0][t]) + (s_sm[2][0][t] + s_sm[3][0][t]));
    if (A.g_head) ctr_atomic_add_global(A.g_head + t, (s_sm[0][1][t] + s_sm[1][1][t]) + (s_sm[2][1][t] + s_sm[3][1][t]));
  }
}

int fill_tower(Tower* T, const ctr_mlp_layer_t* layers, bool need_y) {
  for (int l = 0; l < kL; ++l) {
    const ctr_mlp_layer_t& s = layers[l + 1];
    if (s.n != kN[l] || s.k != kK[l] || s.act != CTR_ACT_RELU || !s.w || !ctr_aligned16(s.w)) return CTR_ELIMIT;
    if (need_y && (!s.y || !ctr_aligned16(s.y) || s.ldy % 4 != 0 || s.ldy < s.n)) return CTR_ELIMIT;
    T->w[l] = s.w; T->b[l] = s.b; T->y[l] = s.y; T->ldy[l] = s.ldy;
  }
  return CTR_OK;
}

bool pattern_ok(const ctr_ncf_proj_t* d) {
  const ctr_mlp_layer_t& l0 = d->layers[0];
  return d->user_idx && d->item_idx && d->mlp_user && d->mlp_item && d->gmf_user && d->gmf_item && l0.w && l0.n == kN0 &&
         l0.k == 2 * kH && l0.act == CTR_ACT_RELU && ctr_aligned16(l0.w) && d->mlp_dim == kH && d->mf_dim == kP &&
         d->proj_n == kP && d->proj_k == kNL && d->proj_w && d->head_w && d->num_users >= 1 && d->num_items >= 1 &&
         d->num_users + d->num_items <= CTR_NCF_PROJ_MAX_ROWS && ctr_aligned16(d->mlp_user) && ctr_aligned16(d->mlp_item) &&
         ctr_aligned16(d->gmf_user) && ctr_aligned16(d->gmf_item) && d->ptab && ctr_aligned16(d->ptab) && d->wfold &&
         ctr_aligned16(d->wfold) && d->batch * 2 < ((int64_t)1 << 31);
}

}  // namespace

#ifdef CTR_STAMPS
extern "C" __attribute__((visibility("default"))) int ctr_ncfp_debug_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 128);
}
#endif

// launch geometry (the round-3 sweeps that chose these values are in git history)
constexpr int kFwdWgs = 256;        // per-sample workgroups of the forward, at most: one per CU (round 9 measured 512)
constexpr int kBwdWgs = 256;        // per-sample workgroups of the backward, at most: one slab each
constexpr int kSlabsMax = 768;      // workspace_floats() reserves slabs for this many backward workgroups
static_assert(kBwdWgs <= kSlabsMax, "the backward's slabs must fit the workspace");
static_assert(kSlabHead < 32 * ((kSlabHead + 31) / 32), "the loss needs a spare output in the last slab-reduce block");

static int64_t workspace_floats(int64_t batch, int64_t num_users, int64_t num_items) {
  const int64_t rows = num_users + num_items;
  const int64_t groups = ctr_ceil_div(batch > 0 ? batch : 1, 16);
  int64_t grid = ctr_ceil_div(groups, kWaves);
  if (grid > kSlabsMax) grid = kSlabsMax;
  // gz0 rows (B + 1, 64) | slot records (2B + 1, 4) | segment sums (rows, 128) | slabs
  // (row B takes the stores of the last group's padding lanes, slot 2B the records of samples without a slot: bad ids,
  // padding lanes; the bucket offsets are the forward's: they live in its plan buffer)
  return (batch + 1) * kN0 + (2 * batch + 1) * 4 + rows * 128 + grid * (int64_t)kSlab;
}

extern "C" int ctr_ncf_proj_workspace_floats(int64_t batch, int64_t num_users, int64_t num_items, int64_t* floats) {
  CTR_REQUIRE(floats && batch >= 0 && num_users >= 0 && num_items >= 0, CTR_EINVAL);
  *floats = workspace_floats(batch, num_users, num_items);
  return CTR_OK;
}

// `phases`: 0 = the whole call; else a mask of its launches (a profiler brackets them one by one): forward 1 = projected
// tables + head fold (+ chunk histograms), 2 = the per-sample kernel (+ the plan's prefixes and offsets); backward 1 =
// the per-sample kernel, 2 = segment sums, 4 = the table-row products + slab reduction + head fold.  With a target the
// backward's launch 1 forms the loss terms and launch 4 stores the loss.
extern "C" int ctr_ncf_proj_fwd(const ctr_ncf_proj_t* d, void* stream) {
  CTR_REQUIRE(d && d->batch >= 0, CTR_EINVAL);
  const int phases = d->phases ? d->phases : 3;
  if (!pattern_ok(d)) return CTR_ELIMIT;
  CTR_REQUIRE(d->prob && d->ldprob >= 1 && d->head_act >= CTR_ACT_NONE && d->head_act <= CTR_ACT_SIGMOID, CTR_EINVAL);
  CTR_REQUIRE(d->ld_proj_w >= d->proj_k, CTR_EINVAL);
  CTR_REQUIRE(!d->training || (d->plan && d->ranks), CTR_EINVAL);
  Tower T;
  int rc = fill_tower(&T, d->layers, true);
  if (rc != CTR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nu = d->num_users, ni = d->num_items;
  const int64_t pwaves = ctr_ceil_div(nu, 16) + ctr_ceil_div(ni, 16);
  const Ids ids{d->user_idx, d->user_stride, d->item_idx, d->item_stride, nu, ni};
  // training: the bucket plan -- a rank workgroup per chunk in this launch, the prefix workgroups in the next
  const bool ranks = d->training && d->batch > 0;
  const Plan plan = plan_of(d->plan, nu + ni, d->batch);
  const int proj_blocks = (int)ctr_ceil_div(2 * pwaves, kWaves) + 1;   // two waves per row block, and the fold workgroup
  const Prep P{d->mlp_user, d->mlp_item, d->layers[0].w, d->layers[0].k, d->layers[0].b, d->ptab, nu, ni,
               d->head_w, d->proj_w, d->ld_proj_w, d->proj_b, d->head_b, d->wfold,
               RankJob{ids, plan, d->ranks, d->batch, proj_blocks}};
  const size_t prep_lds = ranks ? sizeof(int32_t) * (size_t)(nu + ni) : 0;   // a rank workgroup's histogram
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ncfp_prep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(sizeof(int32_t) * CTR_NCF_PROJ_MAX_ROWS)) != hipSuccess)
    return CTR_ELAUNCH;
  if (phases & 1)
    hipLaunchKernelGGL(ncfp_prep_kernel, dim3((unsigned)(proj_blocks + (ranks ? plan.chunks : 0))), dim3(kThreads), prep_lds, st, P);
  rc = ctr_launch_status();
  if (rc != CTR_OK || d->batch == 0 || !(phases & 2)) return rc;
  const int64_t groups = ctr_ceil_div(d->batch, 16);
  int64_t grid = ctr_ceil_div(groups, kWaves);
  // one workgroup per CU, every wave walks several groups (four at batch 65536).  Two per CU -- a second wave per SIMD
  // under whose matrix instructions a wave's row requests and head arithmetic could run -- were measured in round 9 and
  // lost: a workgroup's prologue (ids -> rows -> staged weights, ~4800 of a wave's ~16500 cycles at two groups per
  // wave) is paid twice as often, the launch grew by more than the waves' own lives shrank (supposed: twice the
  // workgroups to launch), and in a training step the forward came to 13.4-13.8 us against 12.7-13.0 us this way
  // (profiles/r09_ncf_fwd_two_waves.txt)
  if (grid > kFwdWgs) grid = kFwdWgs;
  // plan workgroups (training): a thread per table row, behind the per-sample ones
  const int64_t plan_blocks = ranks ? ctr_ceil_div(nu + ni, kThreads) : 0;
  const Fwd F{ids, d->ptab, d->gmf_user, d->gmf_item, d->wfold, d->prob, d->ldprob, d->head_act, d->err_flag,
              PlanJob{plan, (int)grid}};
  constexpr size_t fwd_lds = sizeof(float) * (kWFloats + kBFloats + 80 + kWaves * kFwdStage);
  // the plan workgroups get the launch's dynamic LDS size like everyone else: a CU's 160 KB must hold one of them
  // beside a per-sample workgroup, or the plan would wait for a per-sample workgroup to retire
  static_assert(2 * fwd_lds <= 160 * 1024, "ncfp_fwd: a per-sample workgroup and a plan workgroup share a CU's LDS");
  const auto fwd_kernel = fwd_rows_near(T) ? ncfp_fwd_kernel<true> : ncfp_fwd_kernel<false>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)fwd_lds) != hipSuccess)
    return CTR_ELAUNCH;
  hipLaunchKernelGGL(fwd_kernel, dim3((unsigned)(grid + plan_blocks)), dim3(kThreads), fwd_lds, st, T, d->batch, F);
  return ctr_launch_status();
}

extern "C" int ctr_ncf_proj_bwd(const ctr_ncf_proj_t* d, const ctr_ncf_proj_grad_t* g, void* stream) {
  CTR_REQUIRE(d && g && d->batch >= 0, CTR_EINVAL);
  if (!pattern_ok(d)) return CTR_ELIMIT;
  CTR_REQUIRE(d->plan && d->ranks && d->prob && g->workspace, CTR_EINVAL);
  // the gradient of prob: the caller's, or (target set) the binary cross entropy's, formed by the per-sample kernel
  const bool fused = g->target != nullptr;
  CTR_REQUIRE(fused ? g->ldtarget >= 1 : (g->gprob && g->ldgprob >= 1 && !g->loss), CTR_EINVAL);
  CTR_REQUIRE(!g->loss || d->batch > 0, CTR_EINVAL);   // (no mean over no samples)
  CTR_REQUIRE(!g->zero_buf || (ctr_aligned16(g->zero_buf) && g->zero_floats % 4 == 0 && g->zero_floats >= 0), CTR_EALIGN);
  Tower T;
  int rc = fill_tower(&T, d->layers, true);
  if (rc != CTR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t m = d->batch, nu = d->num_users, ni = d->num_items, rows = nu + ni;
  if (m == 0) return g->zero_buf ? ctr_zero_fill(g->zero_buf, g->zero_floats, st) : CTR_OK;
  for (int l = 1; l <= kL; ++l) CTR_REQUIRE(g->layers[l].gw && g->layers[l].gb, CTR_EINVAL);
  CTR_REQUIRE(g->workspace_floats >= workspace_floats(m, nu, ni) && ctr_aligned16(g->workspace), CTR_ELIMIT);
  // carve the workspace
  float* ws = g->workspace;
  float* gzb = ws;            ws += (m + 1) * kN0;
  float* aux = ws;            ws += (2 * m + 1) * 4;
  float* stt = ws;            ws += rows * 128;
  float* slabs = ws;
  const int64_t groups = ctr_ceil_div(m, 16);
  int64_t grid = ctr_ceil_div(groups, kWaves);
  if (grid > kBwdWgs) grid = kBwdWgs;
  const Ids ids{d->user_idx, d->user_stride, d->item_idx, d->item_stride, nu, ni};
  const Plan plan = plan_of(d->plan, rows, m);
  const int32_t* offs = plan.offsets;
  const Bwd B{ids, d->ptab, d->wfold, d->prob, d->ldprob, fused ? g->target : g->gprob, fused ? g->ldtarget : g->ldgprob,
              d->head_act, plan.base, plan.shift,
              d->ranks, gzb, aux, slabs, stt, rows * 128, g->zero_buf, g->zero_buf ? g->zero_floats : 0};
  constexpr size_t lds_bytes = sizeof(float) * (size_t)kBwdLdsFloats;
  const auto bwd_kernel = fused ? ncfp_bwd_kernel<true> : ncfp_bwd_kernel<false>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes) != hipSuccess)
    return CTR_ELAUNCH;
  const int phases = g->phases ? g->phases : 7;
  if (phases & 1) hipLaunchKernelGGL(bwd_kernel, dim3((unsigned)grid), dim3(kThreads), lds_bytes, st, T, m, B);
  rc = ctr_launch_status();
  if (rc != CTR_OK) return rc;
  // segment sums over the buckets
  const Seg S{gzb, aux, offs, d->gmf_user, d->gmf_item, nu, ni, m, stt};
  if (phases & 2)
    hipLaunchKernelGGL(ncfp_segsum_kernel, dim3((unsigned)ctr_ceil_div(2 * m, kSegWgSlots)), dim3(kThreads), 0, st, S);
  rc = ctr_launch_status();
  if (rc != CTR_OK) return rc;
  // the table-row products, and in front of them (own workgroups) the tower's dW / db partials and the head fold's
  // chain rule (its GMF part comes from the products)
  Roles R{(kSlabHead + 31) / 32,
          slabs, (int)grid, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, d->head_w, d->proj_w, d->ld_proj_w,
          d->proj_b, g->g_head_w, g->g_proj_w, g->ld_g_proj_w, g->g_proj_b, g->g_head_b, g->loss, 1.0f / (float)m};
  for (int l = 0; l < kL; ++l) {
    R.gw[l] = g->layers[l + 1].gw;
    R.gb[l] = g->layers[l + 1].gb;
  }
  const int64_t fwgs = ctr_ceil_div(ctr_ceil_div(nu, 16), kWaves) + ctr_ceil_div(ctr_ceil_div(ni, 16), kWaves);
  const Fin N{stt, d->mlp_user, d->mlp_item, d->gmf_user, d->gmf_item, d->layers[0].w, d->layers[0].k, d->wfold, nu, ni,
              g->g_mlp_user, g->g_mlp_item, g->g_gmf_user, g->g_gmf_item, g->layers[0].gw, d->layers[0].k, g->layers[0].gb,
              g->g_head_w, (int)fwgs, R};
  if (phases & 4)
    hipLaunchKernelGGL(ncfp_finish_kernel, dim3((unsigned)(R.red_blocks + 1 + kFinParts * fwgs)), dim3(kThreads), 0, st, N);
  return ctr_launch_status();
}
