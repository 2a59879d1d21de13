// k_dn_band.h -- the arithmetic of the denoising rule (itsx_denoise_table; k_denoise.hip) that host and device share: the skew cut-off
// of a pair, the symbols' 4-bit codes and one column of the banded bit-vector edit distance.  Plain C++ so that a host program can
// hold it to a full DP matrix.
//
// The distance is Myers' bit-vector recurrence on a band that slides down one row per column (Hyyro's banded variant).  With the
// query down the rows (i = 1 .. m) and the target along the columns (j = 1 .. n), bit b of column j stands for row i = j - k + b,
// b = 0 .. 63, k = the pair's cut-off <= 31: the band holds the diagonals -k .. 63 - k, which include -k .. k.  Pv / Mv are the
// vertical differences D[i][j] - D[i - 1][j] = +1 / -1.  Going to the next column shifts both right by one (the same row is one bit
// lower there) and then runs Myers' column step.  What the band cannot see is taken at its worst, which is consistent with a DP whose
// cells outside the band are one more than their neighbour inside: the row under the band enters with Pv = 1 (its left neighbour is
// then never the minimum), the row above the band has the horizontal difference +1 (carry-in of Ph; for the rows i <= 0 of the first
// columns that is exact: D[i][j] = |i| + j there, which also makes D[0][j] = j).  Every in-band value is then >= the true one, and a
// path of cost <= k never leaves the diagonals -k .. k, so the result is exact when it is <= k and > k otherwise.
// The score is followed down the diagonal m - n (bit k + m - n <= 2 k <= 62), from |m - n| at column 0 to D[m][n] at column n: a
// diagonal step adds 0 or 1, 0 iff D0 = Xh | Mv has the bit.  So the score never falls, and a pair is lost as soon as it passes k.
#pragma once
#include <stdint.h>
#include "iupac.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_HD __host__ __device__ __forceinline__
#else
#define DN_HD inline
#endif

namespace itsx {

// the largest d <= D with (double)aq <= max_skew[d - 1] * (double)at (one multiply, one compare); 0: the centroid cannot take it
DN_HD int dn_dmax(int32_t aq, int32_t at, const double *max_skew, int D)
{
  int d = 0;
  while (d < D && (double)aq <= max_skew[d] * (double)at) d++;
  return d;
}

// upper-case symbol -> its 4-bit code (iupac.h's order), 'A' .. 'Y' packed as nibbles; anything else reads as '-' (4)
constexpr uint64_t dn_code_lut(int first)
{
  uint64_t v = 0;
  for (int l = 0; l < 16; l++) {
    uint64_t code = 4;
    for (uint32_t c = 0; c < 16; c++) if (iupac_symbol(c) == (uint32_t)('A' + first + l)) code = c;
    v |= code << (4 * l);
  }
  return v;
}
constexpr uint64_t DN_CODES_LO = dn_code_lut(0), DN_CODES_HI = dn_code_lut(16);
DN_HD uint32_t dn_code(uint32_t ch)
{
  const uint32_t l = ch - (uint32_t)'A';
  if (l >= 32u) return 4u;
  return (uint32_t)((l < 16u ? DN_CODES_LO : DN_CODES_HI) >> (4u * (l & 15u))) & 15u;
}
static_assert(((DN_CODES_LO >> 0) & 15) == 0 && ((DN_CODES_LO >> 8) & 15) == 1 && ((DN_CODES_LO >> 24) & 15) == 2 && ((DN_CODES_HI >> 12) & 15) == 3, "A C G T");
static_assert(((DN_CODES_LO >> 52) & 15) == 15 && ((DN_CODES_HI >> 4) & 15) == 5 && ((DN_CODES_HI >> 32) & 15) == 6, "N R Y");

struct DnBand { uint64_t Pv, Mv; int score, bit; };

DN_HD void dn_band_init(DnBand &s, int k, int m, int n)
{
  s.Mv = (2ull << k) - 1ull;                                  // rows -k .. 0: D[i][0] = |i|
  s.Pv = ~s.Mv;                                               // rows 1 ..: D[i][0] = i
  s.bit = k + m - n;
  s.score = m > n ? m - n : n - m;
}
// column j: eq has bit b set iff query symbol j - k + b (1-based; none outside 1 .. m) equals target symbol j
DN_HD void dn_band_step(DnBand &s, uint64_t eq)
{
  const uint64_t Pv = (s.Pv >> 1) | (1ull << 63), Mv = s.Mv >> 1;
  const uint64_t Xv = eq | Mv;
  const uint64_t Xh = (((eq & Pv) + Pv) ^ Pv) | eq;
  const uint64_t Ph = ((Mv | ~(Xh | Pv)) << 1) | 1ull, Mh = (Pv & Xh) << 1;
  s.score += (int)(~((Xh | Mv) >> s.bit) & 1ull);
  s.Pv = Mh | ~(Xv | Ph);
  s.Mv = Ph & Xv;
}
// the 64 match bits from bit P of a symbol's row of the match table (P >= 0; row[(P >> 6) + 1] must exist)
DN_HD uint64_t dn_band_eq(const uint64_t *row, int P)
{
  const int w = P >> 6, sh = P & 63;
  const uint64_t lo = row[w], hi = row[w + 1];
  return (lo >> sh) | ((hi << 1) << (63 - sh));                 // (in two steps: sh == 0 must shift all of hi out)
}

}  // namespace itsx
