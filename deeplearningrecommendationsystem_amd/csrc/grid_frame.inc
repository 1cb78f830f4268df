// Device helpers the grid kernels share, included as TEXT behind mfma16_tower.inc.  Scalars in, a scalar out: the
// kernels sit at the register limit of two waves per SIMD, and only helpers of this kind leave every instruction
// stream as it was (DESIGN.md section 4o); nothing that takes the operand arrays belongs here.

// the user of row `row` of the user tile that begins at row r0 and holds cnt rows: rows past cnt repeat the last one,
// an id outside the table reads its nearest row (the caller validates the list: this keeps the reads inside)
__device__ __forceinline__ int64_t grid_user(const int64_t* users, int64_t user0, int64_t nu, int64_t r0, int cnt, int row) {
  const int64_t rr = r0 + (row < cnt ? row : cnt - 1);
  const int64_t u = users ? users[rr] : user0 + rr;
  return u < 0 ? 0 : u >= nu ? nu - 1 : u;
}

// sum over the four lanes (q = 0 .. 3) of a column: every one of them gets the same bits
__device__ __forceinline__ float column_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
