// k_cl_cell.h -- the packed cell of the clustering alignment, shared by the kernels that sweep it (k_cluster.hip: align_pair, the
// identity; k_cigar.hip: the same sweep with direction bits, the path).  One definition, so that the two cannot drift apart:
// (score, matches, counted columns) in one int64, score << 40 | matches << 20 | -columns, and integer max is the lexicographic max.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace itsx {

typedef long long i64;
typedef unsigned long long u64;

static constexpr int SH_S = 40, SH_M = 20;
static constexpr i64 NEGV = -(1LL << 60);
static constexpr i64 ONE_S = 1LL << SH_S, ONE_M = 1LL << SH_M;
static constexpr i64 GOI = -22 * ONE_S - 1, GEI = -2 * ONE_S - 1, GOT = -3 * ONE_S, GET = -1 * ONE_S;
// diagonal increments: match 2*ONE_S + ONE_M - 1, mismatch -4*ONE_S - 1, compatible ambiguity ONE_M - 1, incompatible -1 (built in align_pair)
static constexpr u64 MASK4_LUT = 0xFD7EB96C3A508421ULL;      // IUPAC set of each digital code, 4 bits each

__device__ __forceinline__ uint32_t mask4(uint32_t code) { return (uint32_t)(MASK4_LUT >> (4 * code)) & 15u; }
__device__ __forceinline__ uint32_t revmask4(uint32_t m) { return ((m & 1u) << 3) | ((m & 2u) << 1) | ((m & 4u) >> 1) | ((m & 8u) >> 3); }
__device__ __forceinline__ bool unamb4(uint32_t m) { return __popc(m) == 1; }
__device__ __forceinline__ i64 max64(i64 a, i64 b) { return a > b ? a : b; }
__device__ __forceinline__ i64 shfl_up64(i64 v)
{
  int lo = (int)(v & 0xffffffffLL), hi = (int)(v >> 32);
  lo = __shfl_up(lo, 1); hi = __shfl_up(hi, 1);
  return ((i64)hi << 32) | (i64)(uint32_t)lo;
}
// the cell's three numbers: matches and counted columns of the optimum (identity_of divides them)
__device__ __host__ __forceinline__ void cell_unpack(i64 res, i64 &score, i64 &matches, i64 &cols)
{
  score = (res + (1LL << (SH_S - 1))) >> SH_S;
  const i64 low = res - score * ONE_S;
  matches = (low + (1LL << (SH_M - 1))) >> SH_M;
  cols = matches * ONE_M - low;
}
__device__ __host__ __forceinline__ double identity_of(i64 res)
{
  i64 score, matches, cols;
  cell_unpack(res, score, matches, cols);
  return cols > 0 ? 100.0 * (double)matches / (double)cols : 0.0;
}

}  // namespace itsx
