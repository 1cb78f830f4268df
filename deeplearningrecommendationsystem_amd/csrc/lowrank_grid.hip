// A biased low-rank product over the whole user x item GRID (ctr_lowrank_grid_scores):
//     out[r, i] = sigmoid((a[u_r] + b[i]) + sum_k cu[u_r, k] ci[i, k])
// the grid of MatrixFactorization (rank = the embedding size, no biases), of FFM (rank = num_vector: its eight
// cross dots collapse into one) and of LogisticRegression (rank 0): model/mf.py, model/ffm.py, model/lr.py; DESIGN.md
// section 4q.
//
// Unlike its siblings this kernel has little to compute: a pair costs 2 rank flop and 4 bytes of score, and nothing
// else leaves the chip, so the tile is chosen for what a store instruction writes (measured, DESIGN.md section 4q: at
// rank 64 the kernel reaches a quarter of the machine's fill rate -- it is not store-bound as built).
// The tile is users x items on v_mfma_f32_32x32x2_f32: a wave owns 32 consecutive items and holds
// their rows, ONCE, as the B operand (rank / 2 registers: lane (h, n) keeps ci[i0 + n][2 s + h] for step s); the
// workgroup stages the rows of 32 users in LDS in operand order (lane (h, m) of step s reads cu[u_m][2 s + h]: one
// conflict-free 16-byte read per four steps), and rank / 2 matrix products later register j of the accumulator is row
// (j & 3) + 8 (j >> 2) + 4 h of the tile at column n: a store instruction writes 128 contiguous bytes of two score
// rows, the widest shape the accumulator has as it stands.  The siblings' walk (one user x sixteen items a step) would
// store 64 bytes from a quarter of the lanes.  Two LDS stages: the next user tile's rows travel and are put down while a
// tile is computed, one barrier a tile.
//
// One accumulator chain per pair, k ascending (the matrix core's f32 form is an fmaf chain), then (a + b) + dot, then
// ctr_sigmoid; no atomics, no split-K, and a column of the tile is computed from that column's operands only: a score
// is a function of its user's row, its item's row and the two biases alone, bitwise, for any user list, row range,
// item order, ldo or launch geometry.  Items past num_items: loads clamped to the last row, stores masked.
#include "grid_host.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#include "grid_frame.inc"

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUT = CTR_LOWRANK_GRID_USER_TILE;    // users of a user tile = rows of the matrix-core tile
constexpr int kItems = CTR_LOWRANK_GRID_ITEM_TILE; // items of a workgroup
constexpr int kMaxRank = 256;
static_assert(kUT == 32 && kItems == 32 * kWaves, "a wave owns a 32 x 32 tile");
// LDS: eight k of the user tile are a block of 64 lanes x 4 steps, in operand order; 8 floats of padding keep the
// staging stores of neighbouring blocks on different banks
constexpr int kBlock = 64 * 4 + 8;
constexpr int lds_floats(int rank) { return 2 * (rank / 8 * kBlock + kUT); }   // two stages
static_assert(sizeof(float) * lds_floats(kMaxRank) <= 160 * 1024, "the widest rank fits the CU's LDS");

struct Tables {
  const float* cu; const float* ci;            // (nu, rank), (ni, rank)
  const float* a; const float* b;              // (nu), (ni); null: zeros
};
struct Grid {
  const int64_t* users; int64_t user0;         // the users of the rows: users[r], or user0 + r
  int64_t rows, nu, ni;
  float* out; int64_t ldo;
  int64_t utiles;
};

template <int K16>   // rank = 16 K16; 0: the biases alone
__global__ void __launch_bounds__(kThreads) lowrank_grid_scores_kernel(const Tables M, const Grid G) {
  constexpr int K = 16 * K16, K4 = K / 4;
  constexpr int kPieces = kUT * K4;                                   // 16-byte pieces of a user tile
  constexpr int kPasses = K16 == 0 ? 1 : (kPieces + kThreads - 1) / kThreads;
  constexpr int kSteps = K16 == 0 ? 1 : K / 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kUFloats = K / 8 * kBlock;
  float* const s_u = lds;                             // two stages of K / 8 blocks
  float* const s_a = lds + 2 * kUFloats;              // two stages of kUT: a[u]
  const int lane = threadIdx.x & 63, h = lane >> 5, n = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t item = (int64_t)blockIdx.x * kItems + wave * 32 + n;
  const int64_t ic = item < G.ni ? item : G.ni - 1;   // items past the table: the last row, never stored
  // ---- prologue: this lane's half of its item's row, in step order
  float bI[kSteps];
  if constexpr (K16 > 0) {
#pragma unroll
    for (int j = 0; j < K4; ++j) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(M.ci + ic * K + 4 * j);
      bI[2 * j] = h ? v[1] : v[0];
      bI[2 * j + 1] = h ? v[3] : v[2];
    }
  } else {
    bI[0] = 0.0f;
  }
  const float bi = M.b ? M.b[ic] : 0.0f;
  // ---- the user tiles, two LDS stages: while a tile is computed the rows of the next one travel (request) and are
  // put down beside it (stage), so a tile costs ONE barrier, and the wait for the travelling rows comes after the
  // matrix products, when the stores of the tile before have long been acknowledged (the counter is shared)
  f32x4 pv[kPasses];
  float av = 0.0f;
  auto request = [&](int64_t ut) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    if constexpr (K16 > 0) {
#pragma unroll
      for (int e = 0; e < kPasses; ++e) {
        const int p = threadIdx.x + e * kThreads;
        const int row = p < kPieces ? p / K4 : 0, j = p < kPieces ? p % K4 : 0;
        pv[e] = *reinterpret_cast<const f32x4*>(M.cu + grid_user(G.users, G.user0, G.nu, r0, cnt, row) * K + 4 * j);
      }
    }
    if (threadIdx.x < kUT) av = M.a ? M.a[grid_user(G.users, G.user0, G.nu, r0, cnt, threadIdx.x)] : 0.0f;
  };
  auto stage = [&](int buf) {
    if constexpr (K16 > 0) {
#pragma unroll
      for (int e = 0; e < kPasses; ++e) {
        const int p = threadIdx.x + e * kThreads;
        if (p < kPieces) {
          // k = 4 j .. 4 j + 3 of row m: steps 2 j (k even, odd) and 2 j + 1, i.e. block j / 2, step pair j & 1
          const int row = p / K4, j = p % K4;
          float* const dst = s_u + buf * kUFloats + (j >> 1) * kBlock + row * 4 + 2 * (j & 1);
          *reinterpret_cast<f32x2*>(dst) = f32x2{pv[e][0], pv[e][2]};              // h = 0: k = 2 s
          *reinterpret_cast<f32x2*>(dst + 32 * 4) = f32x2{pv[e][1], pv[e][3]};     // h = 1: k = 2 s + 1
        }
      }
    }
    if (threadIdx.x < kUT) s_a[buf * kUT + threadIdx.x] = av;
  };
  if ((int64_t)blockIdx.y < G.utiles) {
    request(blockIdx.y);
    stage(0);
  }
  __syncthreads();
  // register r of the accumulator: row (r & 3) + 8 (r >> 2) + 4 h of the tile, column n
  float* const ocol = G.out + item + 4 * h * G.ldo;
  const bool live = item < G.ni;
  int buf = 0;
  for (int64_t ut = blockIdx.y; ut < G.utiles; ut += gridDim.y, buf ^= 1) {
    const int64_t r0 = ut * kUT;
    const int cnt = (int)(G.rows - r0 < kUT ? G.rows - r0 : kUT);
    const bool more = ut + gridDim.y < G.utiles;
    if (more) request(ut + gridDim.y);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    if constexpr (K16 > 0) {
      const float* const su = s_u + buf * kUFloats + lane * 4;
#pragma unroll
      for (int s4 = 0; s4 < K / 8; ++s4) {
        const f32x4 ua = *reinterpret_cast<const f32x4*>(su + s4 * kBlock);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[c], bI[4 * s4 + c], acc, 0, 0, 0);
      }
    }
    f32x4 au[4];                                      // a[u] of rows 8 g + 4 h .. + 3
#pragma unroll
    for (int g = 0; g < 4; ++g) au[g] = *reinterpret_cast<const f32x4*>(s_a + buf * kUT + 8 * g + 4 * h);
    if (more) stage(buf ^ 1);
    // all sixteen sigmoids first (sixteen independent chains), then the stores: 128 contiguous bytes of two score rows
    // an instruction
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] = ctr_sigmoid((au[r >> 2][r & 3] + bi) + acc[r]);
    float* const otile = ocol + r0 * G.ldo;
    if (cnt == kUT) {
      if (live) {
#pragma unroll
        for (int r = 0; r < 16; ++r) otile[((r & 3) + 8 * (r >> 2)) * G.ldo] = p[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2);
        if (live && row + 4 * h < cnt) otile[row * G.ldo] = p[r];
      }
    }
    __syncthreads();                                  // the next tile's rows are down, this tile's are read
  }
}

constexpr void (*kKernels[kMaxRank / 16 + 1])(const Tables, const Grid) = {   // by rank / 16
    lowrank_grid_scores_kernel<0>,  lowrank_grid_scores_kernel<1>,  lowrank_grid_scores_kernel<2>,
    lowrank_grid_scores_kernel<3>,  lowrank_grid_scores_kernel<4>,  lowrank_grid_scores_kernel<5>,
    lowrank_grid_scores_kernel<6>,  lowrank_grid_scores_kernel<7>,  lowrank_grid_scores_kernel<8>,
    lowrank_grid_scores_kernel<9>,  lowrank_grid_scores_kernel<10>, lowrank_grid_scores_kernel<11>,
    lowrank_grid_scores_kernel<12>, lowrank_grid_scores_kernel<13>, lowrank_grid_scores_kernel<14>,
    lowrank_grid_scores_kernel<15>, lowrank_grid_scores_kernel<16>};

}  // namespace

extern "C" int ctr_lowrank_grid_scores(const float* cu, const float* ci, const float* a, const float* b,
                                       int64_t num_users, int64_t num_items, int rank, const int64_t* users,
                                       int64_t user0, int64_t rows, float* out, int64_t ldo, int row_blocks,
                                       void* stream) {
  CTR_REQUIRE(grid_users_ok(users, user0, rows, num_users, num_items, out, ldo) && row_blocks >= 0, CTR_EINVAL);
  CTR_REQUIRE(rank == 0 ? (a || b) : (cu && ci), CTR_EINVAL);
  if (rank < 0 || rank > kMaxRank || rank % 16 != 0) return CTR_ELIMIT;
  CTR_REQUIRE(grid_ids_fit(num_users, num_items), CTR_ELIMIT);
  if (rank > 0 && (!ctr_aligned16(cu) || !ctr_aligned16(ci))) return CTR_EALIGN;
  if (rows == 0 || num_items == 0) return CTR_OK;
  const int64_t utiles = ctr_ceil_div(rows, kUT), xtiles = ctr_ceil_div(num_items, kItems);
  // a user tile is short (rank / 2 matrix products a wave) and several workgroups share a CU: enough of them to fill
  // the machine a few times over, each walking its share of the user tiles behind one load of its items' rows
  const int64_t y = row_blocks > 0 ? row_blocks : ctr_ceil_div((int64_t)kCtrCUs * 8, xtiles);
  const Tables M{cu, ci, a, b};
  const Grid G{users, user0, rows, num_users, num_items, out, ldo, utiles};
  // item tiles along x (neighbouring workgroups share their user tile's rows in L2), row blocks along y
  return grid_launch(kKernels[rank / 16], dim3((unsigned)xtiles, grid_clamp_y(y, utiles)), kThreads,
                     sizeof(float) * (size_t)lds_floats(rank), stream, M, G);
}
