// k_msv.hip -- stage B of the path: the MSV filter for every (representative, profile) pair.
//
// Replaces hmmsearch's first filter (HMMER p7_MSVFilter: 8-bit saturating multi-hit
// ungapped local score; reference call site itsxpress/SeqSample.py:191-209, threshold
// --F1 1e-6).  This is U x P x L x M byte-cell updates -- the largest cell count on the path.
//
// CDNA4 mapping (no MFMA: this is a max/add scan, not a contraction):
//   * lane = SEQUENCE, profile = uniform over the block.  A block of 256 lanes takes 256 representatives (neighbours in
//     ascending length, so a wave's lanes finish together) through a.PB profiles (up to 32), one after the other; the
//     profile's emission table (16 residue codes x 23 registers' worth, 1.5 KB) sits in LDS, double-buffered, and every
//     lane fetches the 96 bytes of ITS residue's row with six ds_read_b128 -- lanes with the same residue read the same
//     banks (broadcast), the four nucleotides' rows start 8 banks apart.  There is no branch on the residue: the kernel
//     this one replaced (lane = profile, emission rows in 92 registers, one copy of the row code per nucleotide) spent a
//     sixth of its loop moving the row's registers back after the four-way branch, and could not be talked out of it.
//   * each lane keeps the DP row in 23 VGPRs, two cells per register as packed int16 (v_pk_max_i16 / v_pk_add_u16),
//     STRIPED: register r holds cells r (low half) and r + 23 (high half), so the cell before both halves of register r is
//     register r - 1 as it stands; only register 0 takes its predecessors from a shifted copy of the old register 22.
//     The row is updated in place.
//   * THE FLOORED ROW.  xB is a per-lane floor that almost never moves (xJ never falls, so xB = max(xJ - tjbm, bm0) never falls), and a
//     cell is only ever used through max(cell, xB') with a later xB' >= xB.  So a register keeps  c'' = max(c, xB) - xB - 32768  and
//     "max with xB, then add the emission" is ONE saturating add (v_pk_add_i16 ... clamp): it saturates at -32768, which is
//     max(prev, xB) + e floored at xB.  Two packed instructions per two cells (saturating add, max into xE) instead of three (max with
//     xB, add, max into xE: the plain row, still here as the start-up row and behind ITSX_MSV_FLOOR=0).  The cell before node 1 is the
//     floor; xE's halves start at the floor and the real xE is their maximum + xB + 32768.
//       - start-up: with floored cells a row whose cells all fell below xB reads xE = xB where the plain row reads the true, smaller,
//         maximum.  That moves xJ only when xB - tec > xJ, which (xB = max(xJ - tjbm, bm0), tjbm + tec >= 0) needs xJ < bm0 - tec: the
//         first rows of a chain until some cell had a non-negative emission (reads that begin with N).  xJ >= bm0 - tec is monotone, so
//         a wave runs the plain row while any of its working lanes is below it (normally one row), converts its registers once
//         (max with xB, subtract xB + 32768) and goes on with the floored row.  A restored chain makes the same test on its restored xJ.
//       - when xB rises by delta the lane's cells lose delta by a saturating subtract (cells that reach the new floor stay on it, exact
//         by the argument above), under a wave-uniform branch: xJ passes the base only inside a strong hit.
//       - saved states, restores and the join are in real units: c = c'' + xB + 32768 at the block boundary, in the lanes that save or
//         join.  A saved cell is then max(c, xB), not c: a child only uses it through max(cell, xB') with xB' >= xB.
//   * degenerate residues come from the read's exception list (position, code): one compare per row against the lane's
//     next exception; their emission rows are in the same LDS table.
//   * HMMER's unsigned arithmetic floors cells at 0; cells here are signed and unfloored, which is equivalent because
//     every cell is max'ed with xB >= 0 before it is used and xE starts at 0.  HMMER returns at the first row whose
//     xE + bias reaches 255; here that is tested once at the end, on xJ: by the recurrence xJ = max(0, max_i xE_i - tec), so the
//     largest row maximum is xJ + tec whenever xJ > 0 -- after the overflowing row nothing else of the lane's state is used.
//   * the P-value test is folded into a per-(length, profile) threshold on the final xJ byte, computed on the host with
//     the same double arithmetic hmmsearch uses.
//   * results go to res[profile][sorted position]: consecutive lanes, consecutive halfwords.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>
#include "engine.h"
#include "k_api.h"

namespace itsx {

constexpr int MSV_WMODE_DEFAULT = 2;   // what ITSX_MSV_WHOLE means when it is not set (launch_msv)
constexpr int MSV_WT = 16;      // packed words a lane stages in LDS at a time (256 rows)
typedef short s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s2 as_s2(uint32_t u) { return __builtin_bit_cast(s2, u); }
__device__ __forceinline__ uint32_t as_u(s2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
// what a floored register c'' = c - xB - 32768 gains (wrapping) to be real again; nothing when the registers are real
__device__ __forceinline__ s2 real_off(bool floored, int xB) { return as_s2(floored ? (uint32_t)((xB + 32768) & 0xffff) * 0x10001u : 0u); }

// SHARE (k_share.hip): the block's sequences are chains that start at the same depth -- the rows before come from the state the parent
// chain saved (23 packed registers, xJ, xB: MSV_STATE_Q uint4 per (node, profile)), and a chain saves its own state where a
// later chain branches off.  Integer arithmetic on the same operands: the xJ bytes are those of the unshared kernel.
// FLOOR: the floored row (above); false: the plain three-instruction row on every row (ITSX_MSV_FLOOR=0, A/B and cross-check)
// COUNT: the diagnostic launch (ITSX_TEST_HOOKS=1 ITSX_PASSA_DBG=64) that counts floored wave-rows and those on which xB rose
template <bool SHARE, bool FLOOR, bool COUNT = false>
__global__ void __launch_bounds__(256, 6) k_msv(MsvArgs a)
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[2][16 * MSV_TW];
  // each lane's packed words in LDS (its own column: no barrier), loaded ONCE for all the block's profiles where that can be:
  //   a.wtl > 16: the WHOLE read (the launch's longest fits 37 words, 592 bases: 37 KB a block, four blocks a CU);
  //   a.wwin (shared chains only): the wave's WINDOW -- its chains start at row0 and end by Lw, a third of the read on average --
  //     when that is at most 16 words, indexed from the window's first word: 16 KB a block, six blocks a CU;
  //   else 16 words (256 rows) at a time, again for every profile
  extern __shared__ uint32_t wst[];
  const int s = a.k0 + blockIdx.x * 256 + threadIdx.x;
  const bool valid = s < a.k1;
  int L = 0, nexc = 0, tjb = 0, Lt = 0;
  const uint32_t *wp = a.rd.words;
  const uint32_t *ep = a.rd.exc;
  const int row0 = SHARE ? (a.sl.depth << a.sl.logB) : 0;
  if (valid) {
    const int r = a.seed_read[a.sorted_uniq[s]];
    L = a.rd.len[r];
    wp = a.rd.words + a.rd.woff[r];
    const int64_t eo = a.rd.excoff[r];
    nexc = (int)(a.rd.excoff[r + 1] - eo);
    ep = a.rd.exc + eo;
    Lt = L < a.Lcap ? L : a.Lcap - 1;
    tjb = a.tjb[Lt];
  }
  // two-sided sharing (round 6, k_share.hip: k_join_*): a chain whose suffix another representative of its length ends with too stops
  // after row `myend` = jlev * B and takes the rest of the maximum over paths from that representative's saved BACKWARD state
  // (k_msv_bwd below).  The filter is max-plus arithmetic on integers -- every cell is a maximum over paths of sums -- so
  //     final xJ = max over the state's components (cell_k + g_k, xJ + gJ, xB + gB, g0)
  // is the unshared kernel's xJ exactly, and the overflow test follows from it (xJ = max(0, max_i xE_i - tec) by the recurrence).
  // It stays exact with floored cells max(cell_k, xB): gB = max_k w_k >= g_k for every k (k_msv_bwd), hence
  //     max(cell_k, xB) + g_k <= max(cell_k + g_k, xB + gB)
  // and both terms on the right are components of the maximum already.
  int myend = L, jlev = -1; int64_t jnode = 0;
  if constexpr (SHARE) {
    if (valid && a.sl.endrow) { myend = a.sl.endrow[s]; jlev = a.sl.jlev[s]; jnode = (int64_t)a.sl.jsrc[s] - a.sl.gnode_base; }
  }
  int Lw = valid ? myend : 0;                     // the wave runs to its longest chain (chains of one depth ascend by their last row)
  for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(Lw, d, 64); Lw = o > Lw ? o : Lw; }
  Lw = uni(Lw);
  // wonce: the wave's words are loaded once, from word wbase on (both wave-uniform); words beyond the read are zeros
  const bool whole = a.wtl > MSV_WT;
  const bool wonce = whole || (SHARE && a.wwin && ((Lw - 1) >> 4) - (row0 >> 4) < MSV_WT);      // (the last word read is that of row Lw - 1)
  const int wbase = whole ? 0 : (row0 >> 4);
  if (wonce) {
    const int nw = (L + 15) >> 4;
    for (int j = 0; j < a.wtl; j++) wst[j * 256 + threadIdx.x] = (wbase + j < nw) ? wp[wbase + j] : 0u;
  }
  unsigned long long n_rows = 0, n_rose = 0;        // COUNT: this wave's floored rows, and those that took the xB branch
  if constexpr (COUNT) {                            // ... and the waves with a chain by where their words come from: [2] whole read, [3] window, [4] 16 at a time
    if ((threadIdx.x & 63) == 0 && a.xb_cnt && blockIdx.y == 0 && Lw > 0) atomicAdd(a.xb_cnt + (whole ? 2 : wonce ? 3 : 4), 1ull);
  }
  const int Ppad = a.G * 64;
  const int p0 = a.pfirst + blockIdx.y * a.PB;
  const int np = a.plast;
  int p1 = p0 + a.PB; if (p1 > np) p1 = np;
  const int base = 190;
  for (int pj = p0; pj < p1; pj++) {
    const int p = a.plist ? uni(a.plist[pj]) : pj;
    uint32_t *tb = tab[(pj - p0) & 1];
    // every wave is past the barrier of profile p - 1, so none still reads the table of profile p - 2 in this buffer
    for (int i = threadIdx.x; i < 16 * MSV_TW; i += 256) tb[i] = a.etab[(size_t)p * 16 * MSV_TW + i];
    __syncthreads();
    const int bias = uni(a.pbias[p]), tec = uni(a.ptec[p]), tbm = uni(a.ptbm[p]);
    const int tjbm = tjb + tbm;
    int bm0 = base - tjbm; bm0 = bm0 < 0 ? 0 : bm0;          // xB while xJ is below the base
    int xJ = 0, xB = bm0;
    uint32_t dp[MSV_REGS];
#pragma unroll
    for (int i = 0; i < MSV_REGS; i++) dp[i] = 0;
    if constexpr (SHARE) {
      if (valid && a.sl.depth > 0) {
        // the parent chain's saved state this chain starts from (one 128-byte line; its number: one coalesced load per profile)
        const int64_t src_node = (int64_t)a.sl.src[s] - a.sl.node_base;
        const uint4 *src = (const uint4 *)a.sl.slots + (src_node * a.sl.Pb + (pj - a.pfirst)) * MSV_STATE_Q;
#pragma unroll
        for (int q = 0; q < 6; q++) {
          const uint4 v = src[q];
          dp[4 * q] = v.x; dp[4 * q + 1] = v.y; dp[4 * q + 2] = v.z; if (4 * q + 3 < MSV_REGS) dp[4 * q + 3] = v.w;
        }
        const uint4 v = src[6];
        xJ = (int)v.x; xB = (int)v.y;
      }
    }
    int ei = 0;
    int next_exc = nexc > 0 ? (int)(ep[0] >> 4) : 0x7fffffff;        // (a chain has no exception above its start: k_share.hip)
    uint32_t w = 0;
    const int lend = myend;
    int jxJ = -1;                                    // the joined result, if the chain joins
    int pos = row0;
    // the lane's word of rows q .. q + 15 (q a multiple of 16 below Lw), from its LDS column
    auto word = [&](int q) __attribute__((always_inline)) {
      // 16 at a time (256 rows) where the words were not loaded once: one contiguous 64-byte piece of the read per load instead of a
      // dword every 16 rows -- every one of those dwords cost a whole line once 49 k lanes' lines no longer fit the XCD's L2
      // (75.6 GB fetched per 1 M reads in round 4 against 0.1-0.4 GB of packed reads; profiles/round5_pmc_hbm_traffic_1M.md)
      if (!wonce && ((q & 255) == 0 || q == row0)) {
        const int w0 = (q >> 8) << 4, nw = (L + 15) >> 4;
#pragma unroll
        for (int j = 0; j < MSV_WT; j++) wst[j * 256 + threadIdx.x] = (w0 + j < nw) ? wp[w0 + j] : 0u;
      }
      w = wst[(wonce ? (q >> 4) - wbase : ((q >> 4) & (MSV_WT - 1))) * 256 + threadIdx.x];
    };
    // the emission row of row q (a lane calls it for every row below its `lend`, in ascending order: the exception list is walked here)
    auto erow = [&](int q) __attribute__((always_inline)) -> const uint4 * {
      int code = (int)((w >> ((q & 15) * 2)) & 3u);
      if (q == next_exc) {
        code = (int)(ep[ei] & 15u);
        ei++;
        next_exc = ei < nexc ? (int)(ep[ei] >> 4) : 0x7fffffff;
      }
      return (const uint4 *)(tb + code * MSV_TW);
    };
    // one row.  0: go on, 1: the wave is done, 2 (the plain row of a FLOOR kernel): the start-up rule lets the floored row take this row
    auto step = [&](auto fast_c) __attribute__((always_inline)) -> int {
    constexpr bool FAST = decltype(fast_c)::value;
    {
      if constexpr (FLOOR && !FAST) {
        // the start-up rule: no working lane of the wave is below bm0 - tec any more (monotone: it stays so)
        if (__builtin_amdgcn_ballot_w64(pos < lend && xJ + tec < bm0) == 0ull) return 2;
      }
      const int sh = (pos & 15) * 2;
      if (sh == 0) {
        if constexpr (SHARE) {
          // a block boundary: the state after row `pos` (1-based) is what a chain that branches off here starts from
          if ((pos & ((1 << a.sl.logB) - 1)) == 0 && valid) {
            const int d = pos >> a.sl.logB;
            const unsigned long long m = a.sl.mask[s];
            if (pos > row0 && pos < L && d < 64 && ((m >> d) & 1ull)) {       // (a mask has no bit above the chain's last level)
              const int64_t node = (int64_t)a.sl.node0[s] + __popcll(m & ((1ull << d) - 1ull)) - a.sl.node_base;
              uint4 *dst = (uint4 *)a.sl.slots + (node * a.sl.Pb + (pj - a.pfirst)) * MSV_STATE_Q;
              const s2 ru = real_off(FAST, xB);
#pragma unroll
              for (int q = 0; q < 6; q++)
                dst[q] = make_uint4(as_u(as_s2(dp[4 * q]) + ru), as_u(as_s2(dp[4 * q + 1]) + ru), as_u(as_s2(dp[4 * q + 2]) + ru),
                                    (4 * q + 3 < MSV_REGS) ? as_u(as_s2(dp[(4 * q + 3) % MSV_REGS]) + ru) : 0u);
              dst[6] = make_uint4((uint32_t)xJ, (uint32_t)xB, 0u, 0u);
            }
            if (d == jlev) {
              // the join (saturating adds: a suffix that overflows stays an overflow)
              const uint4 *g = (const uint4 *)a.sl.gslots + (jnode * a.sl.Pb + (pj - a.pfirst)) * MSV_STATE_Q;
              s2 mx = as_s2(0x80008000u);
              const s2 ru = real_off(FAST, xB);
#pragma unroll
              for (int q = 0; q < 6; q++) {
                const uint4 v = g[q];
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_add_sat(as_s2(dp[4 * q]) + ru, as_s2(v.x)));
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_add_sat(as_s2(dp[4 * q + 1]) + ru, as_s2(v.y)));
                mx = __builtin_elementwise_max(mx, __builtin_elementwise_add_sat(as_s2(dp[4 * q + 2]) + ru, as_s2(v.z)));
                if (4 * q + 3 < MSV_REGS) mx = __builtin_elementwise_max(mx, __builtin_elementwise_add_sat(as_s2(dp[4 * q + 3]) + ru, as_s2(v.w)));
              }
              const uint4 t = g[6];
              int xf = (int)mx.x > (int)mx.y ? (int)mx.x : (int)mx.y;
              const int c1 = xJ + (int)t.x, c2 = xB + (int)t.y, c3 = (int)t.z;
              xf = xf > c1 ? xf : c1; xf = xf > c2 ? xf : c2; xf = xf > c3 ? xf : c3;
              jxJ = xf;                               // (xf + tec = the largest row maximum of the whole read when xf > 0); the chain may walk
                                                      // on for the states its prefix children start from
            }
          }
        }
        if (pos >= Lw) return 1;
        word(pos);
      }
      if (pos < lend) {
        const uint4 *e4 = erow(pos);
        uint32_t e[MSV_TW];
#pragma unroll
        for (int q = 0; q < MSV_TW / 4; q++) { const uint4 v = e4[q]; e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w; }
        if constexpr (FAST) {
          const uint32_t wrap = (dp[MSV_REGS - 1] << 16) | 0x8000u;      // the cell before node 1 is the floor
          s2 xEa = as_s2(0x80008000u), xEb = as_s2(0x80008000u);
#pragma unroll
          for (int r = MSV_REGS - 1; r >= 0; r--) {
            const uint32_t prev = (r > 0) ? dp[r > 0 ? r - 1 : 0] : wrap;
            const s2 sv = __builtin_elementwise_add_sat(as_s2(prev), as_s2(e[r]));
            if (r & 1) xEb = __builtin_elementwise_max(xEb, sv); else xEa = __builtin_elementwise_max(xEa, sv);
            dp[r] = as_u(sv);
          }
          const uint32_t xe2 = as_u(__builtin_elementwise_max(xEa, xEb));
          const int xEl = (int)(int16_t)(xe2 & 0xffffu), xEh = (int)xe2 >> 16;
          const int xE = (xEl > xEh ? xEl : xEh) + xB + (32768 - tec);   // the real xE - tec
          xJ = xJ > xE ? xJ : xE;
          int nb = xJ - tjbm; nb = nb > bm0 ? nb : bm0;
          const int delta = nb - xB;
          xB = nb;
          const bool rose = __builtin_amdgcn_ballot_w64(delta > 0) != 0ull;
          // (the lanes at work in a row are nested, so the wave's longest lane counts the wave's rows)
          if constexpr (COUNT) { n_rows++; n_rose += rose; }
          if (rose) {                                                    // xB rose (inside a strong hit): the cells sink by as much
            const s2 dv = as_s2((uint32_t)((-delta) & 0xffff) * 0x10001u);
#pragma unroll
            for (int i = 0; i < MSV_REGS; i++) dp[i] = as_u(__builtin_elementwise_add_sat(as_s2(dp[i]), dv));
          }
        } else {
          const s2 xBv = as_s2((uint32_t)xB * 0x10001u);
          const uint32_t wrap = dp[MSV_REGS - 1] << 16;
          s2 xEa = as_s2(0u), xEb = as_s2(0u);
#pragma unroll
          for (int r = MSV_REGS - 1; r >= 0; r--) {
            const uint32_t prev = (r > 0) ? dp[r > 0 ? r - 1 : 0] : wrap;
            const s2 sv = __builtin_elementwise_max(as_s2(prev), xBv) + as_s2(e[r]);
            if (r & 1) xEb = __builtin_elementwise_max(xEb, sv); else xEa = __builtin_elementwise_max(xEa, sv);
            dp[r] = as_u(sv);
          }
          const uint32_t xe2 = as_u(__builtin_elementwise_max(xEa, xEb));
          int xE = (int)(xe2 & 0xffffu);
          const int xEh = (int)(xe2 >> 16);
          xE = xE > xEh ? xE : xEh;
          xE -= tec;
          xJ = xJ > xE ? xJ : xE;
          xB = xJ - tjbm; xB = xB > bm0 ? xB : bm0;            // = max(max(base, xJ) - tjbm, 0)
        }
      }
    }
    return 0;
    };
    // the rows from `pos` on, FAST: with the floored row (the registers hold c''), else with the plain one.  Two loops, not one loop with
    // a flag: where both rows' registers meet again the compiler copies all 23 of them, every row.  The plain loop of a FLOOR kernel
    // ends with step's 2 at the top of the first row that the start-up rule lets the floored row take.
    auto rows = [&](auto fast_c) -> int {                // (step's 1 or 2)
      for (; pos <= Lw; pos++)
        if (const int r = step(fast_c)) return r;
      return 1;
    };
    if (rows(std::false_type()) == 2) {
      // into the floored form, once: max with xB, subtract xB + 32768
      const s2 xBv = as_s2((uint32_t)xB * 0x10001u);
      const s2 dn = as_s2((uint32_t)((-(xB + 32768)) & 0xffff) * 0x10001u);
#pragma unroll
      for (int i = 0; i < MSV_REGS; i++) dp[i] = as_u(__builtin_elementwise_max(as_s2(dp[i]), xBv) + dn);
      rows(std::true_type());
    }
    if (valid) {
      if (jxJ >= 0) xJ = jxJ;
      const int ovf = (xJ > 0 && xJ + tec + bias >= 255);      // (the largest row maximum is xJ + tec)
      const int thr = a.thr[(size_t)Lt * Ppad + p];
      const int pass = ovf | (xJ >= thr);
      const int xj = ovf ? 255 : xJ;
      a.res[(size_t)p * a.U + s] = (uint16_t)(pass ? (0x100 | xj) : 0);
    }
  }
  if constexpr (COUNT) {
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned long long o = __shfl_xor(n_rows, d, 64), q = __shfl_xor(n_rose, d, 64);
      n_rows = o > n_rows ? o : n_rows; n_rose = q > n_rose ? q : n_rose;
    }
    if ((threadIdx.x & 63) == 0 && a.xb_cnt) { atomicAdd(a.xb_cnt, n_rows); atomicAdd(a.xb_cnt + 1, n_rose); }
  }
}

// Round 6, two-sided sharing: the BACKWARD chains of the filter.  A row of the filter is a max-plus linear map of the state (46 cells, xJ,
// xB and the constant 0: xB = max(xJ - tjbm, bm0)); the final xJ is a max-plus linear functional of the last state.  Pulled back through
// the rows L, L - 1, ..., j B + 1 it becomes a vector g_j with  final xJ = max over components (state after row j B + g_j)  for EVERY
// prefix: it belongs to the suffix, and the uniques of one length that end alike share it.  Lane = Backward chain (k_share.hip: the
// uniques that save a state for somebody), the block's 256 chains start the same number of blocks from the end, a.PB profiles one after
// the other.  With a' the adjoint of a new row's value and x the row's residue:
//     aJ = max(gJ, gB - tjbm),  g0 <- max(g0, gB + bm0),  aE = aJ - tec
//     w_k = max(g_k, aE) + e_k(x)   (k = 46 .. 1),   g_k-1 <- w_k  (g_46 <- none),   gB <- max_k w_k,   gJ <- aJ
// in the forward kernel's register striping (register r = cells r, r + 23: the shift by one cell is a renaming but for the wrap register).
// Adds saturate: a suffix whose score overflows stays above every threshold instead of wrapping.  The rows a Backward chain walks lie
// above its read's last residue outside ACGT (k_share.hip), so it never meets an exception.
__global__ void __launch_bounds__(256, 6) k_msv_bwd(MsvArgs a)
{
  __shared__ __attribute__((aligned(16))) uint32_t tab[2][16 * MSV_TW];
  extern __shared__ uint32_t wst[];
  const bool whole = a.wtl > MSV_WT;
  const int s = a.k0 + blockIdx.x * 256 + threadIdx.x;      // backward position
  const bool valid = s < a.k1;
  int L = 0, tjb = 0, mysteps = 0;
  const uint32_t *wp = a.rd.words;
  if (valid) {
    const int r = a.seed_read[a.sorted_uniq[s]];
    L = a.rd.len[r];
    wp = a.rd.words + a.rd.woff[r];
    const int Lt = L < a.Lcap ? L : a.Lcap - 1;
    tjb = a.tjb[Lt];
    mysteps = a.sl.endrow[s];
  }
  const int nw = (L + 15) >> 4;
  if (whole) for (int j = 0; j < a.wtl; j++) wst[j * 256 + threadIdx.x] = (j < nw) ? wp[j] : 0u;
  int nsteps = mysteps;
  for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(nsteps, d, 64); nsteps = o > nsteps ? o : nsteps; }
  nsteps = (a.sl.dbg & 32) ? 0 : uni(nsteps);                // (diagnostic bit, ITSX_TEST_HOOKS=1 ITSX_PASSA_DBG=32: no rows)
  const int rd = a.sl.depth, logB = a.sl.logB;
  const int A = (L + (1 << logB) - 1) >> logB;
  const int top = (A - rd) << logB;                          // the row the chain's state stands after (virtual past L when rd = 0)
  const int p0 = a.pfirst + blockIdx.y * a.PB;
  int p1 = p0 + a.PB; if (p1 > a.plast) p1 = a.plast;
  const int base = 190;
  constexpr int NEG = -16384;
  const unsigned long long m = valid ? a.sl.mask[s] : 0ull;
  for (int pj = p0; pj < p1; pj++) {
    const int p = pj;
    uint32_t *tb = tab[(pj - p0) & 1];
    for (int i = threadIdx.x; i < 16 * MSV_TW; i += 256) tb[i] = a.etab[(size_t)p * 16 * MSV_TW + i];
    __syncthreads();
    const int tec = uni(a.ptec[p]), tbm = uni(a.ptbm[p]);
    const int tjbm = tjb + tbm;
    int bm0 = base - tjbm; bm0 = bm0 < 0 ? 0 : bm0;
    int gJ = 0, gB = NEG, g0 = NEG;
    uint32_t g[MSV_REGS];
#pragma unroll
    for (int i = 0; i < MSV_REGS; i++) g[i] = 0xC000C000u;   // NEG in both halves
    if (valid && rd > 0) {
      const int64_t src_node = (int64_t)a.sl.src[s] - a.sl.node_base;
      const uint4 *src = (const uint4 *)a.sl.slots + (src_node * a.sl.Pb + (pj - a.pfirst)) * MSV_STATE_Q;
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const uint4 v = src[q];
        g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; if (4 * q + 3 < MSV_REGS) g[4 * q + 3] = v.w;
      }
      const uint4 v = src[6];
      gJ = (int)v.x; gB = (int)v.y; g0 = (int)v.z;
    }
    uint32_t w = 0; int wi = -1;
    for (int step = 0; ; step++) {
      if ((step & ((1 << logB) - 1)) == 0 && step > 0 && valid) {
        // a block boundary: the state after row top - step is what the Forward chains that end there take
        const int rdl = rd + (step >> logB);
        if (step <= mysteps && rdl < 64 && ((m >> rdl) & 1ull)) {
          const int64_t node = (int64_t)a.sl.node0[s] + __popcll(m & ((1ull << rdl) - 1ull)) - a.sl.node_base;
          uint4 *dst = (uint4 *)a.sl.slots + (node * a.sl.Pb + (pj - a.pfirst)) * MSV_STATE_Q;
#pragma unroll
          for (int q = 0; q < 6; q++) dst[q] = make_uint4(g[4 * q], g[4 * q + 1], g[4 * q + 2], (4 * q + 3 < MSV_REGS) ? g[(4 * q + 3) % MSV_REGS] : 0u);
          dst[6] = make_uint4((uint32_t)gJ, (uint32_t)gB, (uint32_t)g0, 0u);
        }
      }
      if (step >= nsteps) break;
      const int row = top - step;                             // this step pulls the state back through row `row` (1-based)
      if (row <= L && step < mysteps) {
        const int pos = row - 1;
        if ((pos >> 4) != wi) {
          wi = pos >> 4;
          if (whole) w = wst[wi * 256 + threadIdx.x];
          else w = wp[wi];                                    // (reads past 592 bases: a dword every 16 rows)
        }
        const int code = (int)((w >> ((pos & 15) * 2)) & 3u);
        const uint4 *e4 = (const uint4 *)(tb + code * MSV_TW);
        uint32_t e[MSV_TW];
#pragma unroll
        for (int q = 0; q < MSV_TW / 4; q++) { const uint4 v = e4[q]; e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w; }
        int aJ = gB - tjbm; aJ = aJ > gJ ? aJ : gJ;
        const int n0 = gB + bm0; g0 = g0 > n0 ? g0 : n0;
        int aE = aJ - tec; aE = aE > 30000 ? 30000 : aE;
        const s2 aEv = as_s2((uint32_t)(aE & 0xffff) * 0x10001u);
        s2 mxa = as_s2(0xC000C000u), mxb = as_s2(0xC000C000u);
        // W[r] = (w of cells r, r + 23); the new g[r] is W[r + 1], the new g[22] = (W[0]'s high half, nothing)
        const s2 W0 = __builtin_elementwise_add_sat(__builtin_elementwise_max(as_s2(g[0]), aEv), as_s2(e[0]));
        mxa = __builtin_elementwise_max(mxa, W0);
#pragma unroll
        for (int r = 1; r < MSV_REGS; r++) {
          const s2 Wr = __builtin_elementwise_add_sat(__builtin_elementwise_max(as_s2(g[r]), aEv), as_s2(e[r]));
          if (r & 1) mxb = __builtin_elementwise_max(mxb, Wr); else mxa = __builtin_elementwise_max(mxa, Wr);
          g[r - 1] = as_u(Wr);
        }
        g[MSV_REGS - 1] = (as_u(W0) >> 16) | 0xC0000000u;
        const uint32_t m2 = as_u(__builtin_elementwise_max(mxa, mxb));
        const int lo = (int)(int16_t)(m2 & 0xffffu), hi = (int)(int16_t)(m2 >> 16);
        gB = lo > hi ? lo : hi;
        gJ = aJ;
      }
    }
  }
}

// ITSX_LAZY_HIST: the blocks a CU really holds of every launch shape (kernel, dynamic LDS) of a search, one stderr line per shape --
// the occupancy the registers allow is not the one a launch gets (37 + 3 KB of LDS a block: four blocks, whatever the registers)
static std::mutex g_occ_mu;
static std::vector<std::pair<const void *, size_t>> g_occ_seen;
void msv_diag_begin() { std::lock_guard<std::mutex> lk(g_occ_mu); g_occ_seen.clear(); }
static void msv_occupancy_line(const void *fn, const char *name, size_t lds)
{
  std::lock_guard<std::mutex> lk(g_occ_mu);
  for (const auto &o : g_occ_seen) if (o.first == fn && o.second == lds) return;
  g_occ_seen.emplace_back(fn, lds);
  int nb = -1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, lds) != hipSuccess) { (void)hipGetLastError(); nb = -1; }
  fprintf(stderr, "[itsx] msv occupancy: %s dynamic LDS %zu B: %d blocks of 256 per CU (%d waves per SIMD)\n", name, lds, nb, nb);
}
template <typename K>
static void msv_go(K kern, const char *name, const dim3 &grid, size_t lds, hipStream_t st, const MsvArgs &a)
{
  if (sw_get("ITSX_LAZY_HIST")) msv_occupancy_line((const void *)kern, name, lds);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
}

// lds_pad: dynamic LDS the launch asks for and never touches -- a cap on the blocks a CU holds (160 KB per CU), for the launch that
// runs beside another stream's kernels and must leave them their registers
void launch_msv(const MsvArgs &a0, hipStream_t st, int lds_pad)
{
  MsvArgs a = a0;
  if (a.k1 <= 0) { a.k0 = 0; a.k1 = a.U; }
  if (a.plast <= 0) { a.pfirst = 0; a.plast = a.plist ? a.nlist : a.P; }
  const int np = a.plast - a.pfirst, nk = a.k1 - a.k0;
  if (nk <= 0 || np <= 0) return;
  const dim3 grid((unsigned)((nk + 255) / 256), (unsigned)((np + a.PB - 1) / a.PB));
  // words a lane keeps in LDS, ITSX_MSV_WHOLE (read at every launch; MSV_WMODE_DEFAULT when unset):
  //   1: every word of the launch's longest read when that is at most 37 (four blocks of 37 + 3 KB fill a CU's 160 KB exactly: four
  //      waves per SIMD whatever the registers allow), else 16 at a time;
  //   2: shared chains keep their wave's window, 16 words (16 + 3 KB a block: six blocks a CU, the six waves per SIMD that 80 registers
  //      are held to); the unshared kernel as under 1;
  //   0: always 16 at a time
  const char *wsw = sw_get("ITSX_MSV_WHOLE");
  int wmode = wsw ? atoi(wsw) : MSV_WMODE_DEFAULT;
  if (wmode < 0 || wmode > 2) wmode = MSV_WMODE_DEFAULT;
  const int need = (a.Lcap - 1 + 15) / 16;
  const bool window = wmode == 2 && a.share == 1;
  a.wtl = (wmode != 0 && !window && need > MSV_WT && need <= 37) ? need : MSV_WT;
  a.wwin = window;
  // (a Backward chain walks a few blocks of its read through one to eight profiles: it takes its words from memory as it goes, a dword
  // every 16 rows -- the whole read in LDS first was 37 gathers per chain for ~6 words used, and 37 KB per block held a CU to 4 blocks)
  static const bool bwd_whole = sw_get("ITSX_MSV_BWD_WHOLE") && atoi(sw_get("ITSX_MSV_BWD_WHOLE")) != 0;
  if (a.share == 2 && !bwd_whole) a.wtl = MSV_WT;
  const size_t lds = std::max<size_t>((size_t)lds_pad, (a.share == 2 && !bwd_whole) ? 0 : (size_t)a.wtl * 256 * sizeof(uint32_t));
  // ITSX_MSV_FLOOR=0: the plain three-instruction row on every row (A/B, and the cross-check of the floored row; read at every launch)
  const bool floored = !(sw_get("ITSX_MSV_FLOOR") && atoi(sw_get("ITSX_MSV_FLOOR")) == 0);
  if (a.share == 2) msv_go(k_msv_bwd, "k_msv_bwd", grid, lds, st, a);
  else if (a.share && floored && a.xb_cnt) msv_go(k_msv<true, true, true>, "k_msv<true, true> counting", grid, lds, st, a);
  else if (a.share && floored) msv_go(k_msv<true, true>, "k_msv<true, true>", grid, lds, st, a);
  else if (a.share) msv_go(k_msv<true, false>, "k_msv<true, false>", grid, lds, st, a);
  else if (floored) msv_go(k_msv<false, true>, "k_msv<false, true>", grid, lds, st, a);
  else msv_go(k_msv<false, false>, "k_msv<false, false>", grid, lds, st, a);
}

// ---------------------------------------------------------------------------------------
// survivor list: (profile, sorted position) cells with the pass bit -> PairRec list grouped by
// profile.  Three small passes: per-chunk counts, per-profile scan of chunk counts, fill.
// a cell is on the list when it passed (bit 8) or when only a chain below it did (bit 9, k_share.hip: the pair runs in pass A for its
// row states and is nobody's result: PairRec::xj = -1); real[p] counts the pairs that passed.  A chunk's two counts (at most CHUNK each)
// travel in one word, cnt = on the list | passed << 16: the scan below sums the second into real[p], so that no chunk adds to its
// profile's counter itself (3 000 chunks of a profile did, one after the other)
static_assert(CHUNK == 2048 && CHUNK < (1 << 15), "k_pair_count packs two chunk counts into one word; k_pair_fill: four waves of eight steps");
__global__ void __launch_bounds__(256) k_pair_count(const uint16_t *__restrict__ res, int32_t U, int32_t nchunks, int32_t *__restrict__ cnt)
{
  __shared__ int32_t ws[4];
  const int p = blockIdx.y, c = blockIdx.x;
  const int64_t base = (int64_t)p * U;
  int32_t v[CHUNK / 256];
#pragma unroll
  for (int i = 0; i < CHUNK / 256; i++) { const int s = c * CHUNK + i * 256 + (int)threadIdx.x; v[i] = s < U ? res[base + s] : 0; }
  int32_t n = 0;
#pragma unroll
  for (int i = 0; i < CHUNK / 256; i++) n += ((v[i] & 0x300) != 0) + (((v[i] >> 8) & 1) << 16);
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) cnt[(int64_t)p * nchunks + c] = ws[0] + ws[1] + ws[2] + ws[3];
}
// one block per profile: exclusive scan of its chunk counts (in place), total and real out
__global__ void __launch_bounds__(256) k_chunk_scan(int32_t *__restrict__ cnt, int32_t nchunks, int32_t *__restrict__ total, int32_t *__restrict__ real)
{
  __shared__ int32_t ws[4], wr[4];
  __shared__ int32_t carry;
  int32_t *row = cnt + (int64_t)blockIdx.x * nchunks;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  int32_t nr = 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int b = 0; b < nchunks; b += 256) {
    const int i = b + threadIdx.x;
    const int32_t both = i < nchunks ? row[i] : 0;
    const int32_t v = both & 0xFFFF;
    nr += both >> 16;
    int32_t inc = v;
    for (int d = 1; d < 64; d <<= 1) { const int32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) ws[wid] = inc;
    __syncthreads();
    int32_t off = carry;
    for (int w = 0; w < wid; w++) off += ws[w];
    if (i < nchunks) row[i] = off + inc - v;
    __syncthreads();
    if (threadIdx.x == 255) carry = off + inc;
    __syncthreads();
  }
  for (int d = 32; d >= 1; d >>= 1) nr += __shfl_down(nr, d, 64);
  if (lane == 0) wr[wid] = nr;
  __syncthreads();
  if (threadIdx.x == 0) { total[blockIdx.x] = carry; real[blockIdx.x] = wr[0] + wr[1] + wr[2] + wr[3]; }
}
// a wave takes CHUNK / 4 consecutive cells of its chunk, 64 at a time: a step's loads are lane-consecutive, its ballot ranks the cells
// that are on the list, and their records leave as consecutive 16-byte stores.  The segment's padding up to the next multiple of 64
// (prof < 0: all 0xFF) is written here too, by the profile's first block: nothing fills the list beforehand
__global__ void __launch_bounds__(256) k_pair_fill(const uint16_t *__restrict__ res, int32_t U, int32_t nchunks, const int32_t *__restrict__ cnt,
                                                   const int64_t *__restrict__ seg_start, const int32_t *__restrict__ total, const int32_t *__restrict__ ulen,
                                                   PairRec *__restrict__ pairs)
{
  __shared__ int32_t ws[4];
  constexpr int STEPS = CHUNK / 256;
  const int p = blockIdx.y, c = blockIdx.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t base = (int64_t)p * U;
  const int64_t seg0 = seg_start[p];
  const int s0 = c * CHUNK + wid * (CHUNK / 4) + lane;
  int32_t v[STEPS], len[STEPS];
#pragma unroll
  for (int i = 0; i < STEPS; i++) { const int s = s0 + 64 * i; v[i] = s < U ? res[base + s] : 0; len[i] = s < U ? ulen[s] : 0; }
  unsigned long long m[STEPS]; int32_t n = 0;
#pragma unroll
  for (int i = 0; i < STEPS; i++) { m[i] = __ballot((v[i] & 0x300) != 0); n += (int32_t)__popcll(m[i]); }
  if (lane == 0) ws[wid] = n;
  __syncthreads();
  int64_t o = seg0 + cnt[(int64_t)p * nchunks + c];
  for (int w = 0; w < wid; w++) o += ws[w];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < STEPS; i++) {
    if (v[i] & 0x300) {
      PairRec pr; pr.useq = s0 + 64 * i; pr.prof = p; pr.xj = (v[i] & 0x100) ? (v[i] & 0xff) : -1; pr.L = len[i];
      pairs[o + __popcll(m[i] & below)] = pr;
    }
    o += __popcll(m[i]);
  }
  if (c == 0 && wid == 0) {
    const int64_t e = seg0 + total[p] + lane;                   // (at most 63 records)
    if (e < seg_start[p + 1]) { PairRec pr; pr.useq = -1; pr.prof = -1; pr.xj = -1; pr.L = -1; pairs[e] = pr; }
  }
}
__global__ void __launch_bounds__(256) k_fill_ulen(int32_t U, const int32_t *__restrict__ sorted_uniq, const int32_t *__restrict__ seed_read,
                                                   const int32_t *__restrict__ len, int32_t *__restrict__ ulen)
{
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < U) ulen[s] = len[seed_read[sorted_uniq[s]]];
}

void launch_pair_count(const uint16_t *res, int32_t P, int32_t U, int32_t nchunks, int32_t *cnt, hipStream_t st)
{
  hipLaunchKernelGGL(k_pair_count, dim3((unsigned)nchunks, (unsigned)P), dim3(256), 0, st, res, U, nchunks, cnt);
}
void launch_chunk_scan(int32_t *cnt, int32_t P, int32_t nchunks, int32_t *total, int32_t *real, hipStream_t st)
{
  hipLaunchKernelGGL(k_chunk_scan, dim3((unsigned)P), dim3(256), 0, st, cnt, nchunks, total, real);
}
void launch_pair_fill(const uint16_t *res, int32_t P, int32_t U, int32_t nchunks, const int32_t *cnt, const int64_t *seg_start, const int32_t *total,
                      const int32_t *ulen, PairRec *pairs, hipStream_t st)
{
  hipLaunchKernelGGL(k_pair_fill, dim3((unsigned)nchunks, (unsigned)P), dim3(256), 0, st, res, U, nchunks, cnt, seg_start, total, ulen, pairs);
}
void launch_fill_ulen(int32_t U, const int32_t *sorted_uniq, const int32_t *seed_read, const int32_t *len, int32_t *ulen, hipStream_t st)
{
  if (U <= 0) return;
  hipLaunchKernelGGL(k_fill_ulen, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, st, U, sorted_uniq, seed_read, len, ulen);
}

}  // namespace itsx
