// k_lazy.hip -- the lazy domain stage: only (representative, profile) pairs that can still win ItsPosition's argmax go
// through Backward, decoding, envelope re-scoring and the ensemble stage.
//
// What the consumer reads.  ItsPosition.parse/_score (itsxpress/SeqSample.py:400-461) keeps, per target sequence and side
// (profile NAME prefix), the FIRST domain row with the strictly greatest %.1f score; rows below the winner are thrown away.
// hmmsearch computes every row all the same (itsxpress/SeqSample.py:191-209); on amplicon data ~130 profiles of a side model
// the same flank, so 98.6 % of the rows lose.
//
// The bound.  For a pair whose multihit Forward score over the whole target is fwdsc (nats), every domain's bit score obeys
//     bits <= (fwdsc - nullsc) / ln 2 + C(n),   C(n) = 1 + (2 ln(2 (n + 3) / (3 (n + 2))) + n ln((n + 3) / (n + 2))) / ln 2  (~1.27)
// (scripts/lazy_bound.py derives it: every path of the envelope's unihit Forward sum is a path of the multihit sum with its
// flanks in N and C, and dombias >= 0; measured slack 1.9-2.6 bits, 0 violations).  LenTables::lazy_c holds C(n) plus a margin
// of 0.02 bits for float rounding (both sides are sums of positive products: relative error <= ~3 (n + M) 2^-24).
//
// The schedule (engine.hip: lazy_rounds), per chunk of representatives:
//   pass A   Forward score of EVERY pair past the MSV filter (k_filters_fwd<., 1>: nothing stored but the score);
//   round 1  per (representative, class) the pair with the best bound goes through the whole domain pipeline;
//   round 2  every pair whose bound, as %.1f tenths, reaches the group's best CERTAIN row so far (k_compact_best: reported for
//            every domZ the data set can have) -- ties included, they go to the EARLIER row -- and every pair of a group that
//            has no certain row.  The winner of the full table is among them, and so is every row that ties with it.
// Exactness of the thresholds: hmmsearch's domZ (reported targets per profile) is not known when pairs are skipped, only
// bounds on it -- the reported targets among the evaluated pairs below, the pairs past the MSV filter above.  k_finalize_lazy
// decides every row that both bounds decide alike; a row that neither decides and that could change a winner or the "sequence
// has a row" flag is counted (k_lazy_pending), and the search is then repeated in full (engine.hip: itsx_search_finalize).
#include "engine.h"
#include "k_api.h"
#include "detmath.h"
#include "k_vec.h"

namespace itsx {

// =========================================================================================
// Pass A's kernel: the Forward score of one (representative, profile) pair per lane, as a BOUND -- the same sum over paths as
// p7_ForwardParser (k_filters_fwd), but not HMMER's arithmetic: nodes in their natural order 1..46 instead of the SSE striping
// (whose four D->D passes per row exist only because of the striping), fused multiply-adds, rescaling at 1e20 instead of 1e4.
// The result differs from HMMER's float by rounding only (relative ~1e-5, far inside LenTables::lazy_c's margin) and is used
// for nothing but the selection; the pairs that matter get HMMER's own arithmetic in the domain pipeline.
//   * lane = pair, wave = 64 pairs of one profile (the work list's grouping), pair j = nodes (2j + 1, 2j + 2): every operation on
//     the cells is a packed one over two adjacent nodes;
//   * the row state is TWO cell arrays, 46 register pairs: row i + 1 reads row i's cells only through S[k] = M[k] t(M_k->M_k+1) +
//     I[k] t(I_k->M_k+1) + D[k] t(D_k->M_k+1), a node's contribution to the NEXT node's match cell, and through I+[k], its own insert
//     cell (I[k] t(I_k->I_k) + M[k] t(M_k->I_k)).  Both are formed in row i itself, when M'[k] and D'[k] are born; M and D live for one
//     step of the row loop.  166 registers instead of 212 with M, I, D carried: three waves per SIMD instead of two (ITSX_BOUND_WAVES);
//   * S is formed on the aligned pairs and shifted by one node with a single register move per pair (the transitions are stored by
//     their source node for that: BoundTab);
//   * the D->D chain is 2 scalar FMAs per pair, sequential, as the recurrence is;
//   * the profile's transitions are wave-uniform: 64 B per pair of nodes through scalar loads, double-buffered by hand (as in
//     k_float.hip: left alone, the scheduler hoists a row's loads and spills SGPRs); emission odds by node in LDS (3 KB).
// ~13 packed instructions per pair of nodes, ~320 per row against the striped kernel's 533.
constexpr int BP = BOUND_PAIRS;                     // 23 pairs of nodes: models of up to 46 nodes (engine.h: MMAX)
typedef const f4 __attribute__((address_space(4))) *cf4q;
// record j of a profile's table (engine.hip: install_profiles), 16 floats, what step j of the row loop reads: the chain of pair j
// (bm md dd dd) and the transitions out of pair j - 1's nodes (mm im dm: into the next node's match cell; mi ii), one record per step
struct BT { f2 mm, im, dm, mi, ii, bm, md; float dd1, dd2; };
DEV BT ldbt(const float *tab, int j)
{
  const f4 a = *(cf4q)(uintptr_t)(tab + j * 16), b = *(cf4q)(uintptr_t)(tab + j * 16 + 4), c = *(cf4q)(uintptr_t)(tab + j * 16 + 8),
           d = *(cf4q)(uintptr_t)(tab + j * 16 + 12);
  BT t;
  // (what the folded recurrences read comes first: 12 floats, one dwordx8 + one dwordx4; mi and md are the plain kernel's alone)
  t.mm = (f2){a.x, a.y}; t.im = (f2){a.z, a.w}; t.dm = (f2){b.x, b.y}; t.ii = (f2){b.z, b.w};
  t.bm = (f2){c.x, c.y}; t.dd1 = c.z; t.dd2 = c.w; t.mi = (f2){d.x, d.y}; t.md = (f2){d.z, d.w};
  return t;
}
DEV f2 pfma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
// largest %.1f tenths (biased) a domain of a pair with pass-A score f can print (k_lazy_bound, and k_fwd_bound where it stores b10 itself)
DEV uint32_t lazy_tenths(float f, const LenTables &lt)
{
  if (f != f || f == __builtin_inff()) return (1u << 24) - 1;               // no usable bound: always evaluated
  if (f == -__builtin_inff()) return 1u;
  const double bits = ((double)f - (double)lt.nullsc) / 0.69314718055994529 + (double)lt.lazy_c;
  double t = __builtin_floor(bits * 10.0 + 0.5) + (double)LAZY_TENTHS_BIAS;      // round half UP: never below rint()
  if (t < 1.0) t = 1.0;
  if (t > (double)((1 << 24) - 1)) t = (double)((1 << 24) - 1);
  return (uint32_t)t;
}
// what k_lazy_bound does for pair pi, with the score that was just stored (ShareLaunch::b10 != nullptr)
DEV void lazy_bound_put(const ShareLaunch &sl, const LenTables *lt, int64_t pi, const PairRec &pr, float f)
{
  if (pr.xj < 0) { sl.b10[pi] = 0u; sl.done[pi] = 1; return; }      // ran for its row states only (k_share.hip): never selected
  const uint32_t b = lazy_tenths(f, lt[pr.L]);
  sl.b10[pi] = b;
  atomicMax(&sl.gtop[(size_t)pr.useq * sl.ncls + sl.cls[pr.prof]], ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)pi));
}
// the largest v of the wave's 64 lanes, wave-uniform (a scalar register)
DEV int wave_max(int v)
{
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return uni(v);
}

// SHARE (k_share.hip): the wave's pairs are chains that start at the same depth of their length's prefix tree -- the rows before
// come from the state the parent chain saved for this profile (FWD_STATE_Q float4: S and I+ of the 46 nodes, xN xJ xC xB, the scale's
// logarithm), and a chain saves its own state after row d * B where a later chain branches off.  The same operations on the same
// operands in the same order as the chain's unshared run: the scores are bitwise equal (tests/test_gpu_share.py).
// A block is FWD_WPB consecutive waves of the work list -- the same profile but at a run's end -- so that the waves a CU holds at one time
// read one or two profiles' transition tables through its scalar cache, not eight (SQC_DCACHE_MISSES: 5e)
#ifndef ITSX_FWD_WPB
#define ITSX_FWD_WPB 1
#endif
constexpr int FWD_WPB = ITSX_FWD_WPB;
// Waves per SIMD both pass-A kernels are compiled for.  The row state is two cell arrays (92 registers), so the kernels fit the 168
// registers that three resident waves leave each of them, without scratch; -DITSX_BOUND_WAVES=2 builds the two-wave arm (256 registers)
// from the same source for an A/B.
#ifndef ITSX_BOUND_WAVES
#define ITSX_BOUND_WAVES 3
#endif
// (the attribute and not __launch_bounds__' second argument, which is a minimum only: the kernels need no more than 168 registers, and
// three waves would be resident whatever the minimum says.  With the maximum given too the compiler reports enough registers to hold
// the occupancy at exactly this many waves)
#define BOUND_OCC __attribute__((amdgpu_waves_per_eu(ITSX_BOUND_WAVES, ITSX_BOUND_WAVES)))
// FOLD (engine.hip: install_profiles builds the table for it; every profile whose interior M->D transitions are all > 0, i.e. every
// profile hmmbuild writes): the delete cells are kept DIVIDED by s_k = t(M_k-1 -> D_k) / g_k-1 and the match cells MULTIPLIED by
// g_k = 1 + the share of M_k that the deletes after it carry into E -- constants of the profile, folded into its transitions and
// emission odds on the host.  The same sum over paths term by term, with two operations per node fewer: a new delete cell is ONE
// multiply-add (D^_k+1 = D^_k a_k + M~_k: no product M_k t(M_k -> D_k+1) first), and the row's E is the sum of the match cells alone
// (no second accumulation of the deletes).  The insert cells are kept divided by r_k = t(M_k -> I_k) / g_k in the same way: I^_k' = I^_k t(I_k -> I_k)
// + M~_k, one multiply-add instead of a product and a multiply-add.  8 packed + 2 plain instructions per pair of nodes instead of 11 + 2.
// A row in the carried state (S, I+), x the row's residue:
//     M~'_k = (xB bm_k + S_k-1) e_k(x),   D^'_k+1 = D^'_k a_k + M~'_k,   E = sum M~'_k
//     S'_k = M~'_k mm_k + I+_k im_k + D^'_k dm_k,   I+'_k = I+_k ii_k + M~'_k
// FOLD = false: S' = M' mm + I+ im + D' dm, I+' = M' mi + I+ ii, D'_k+1 = D'_k dd_k + M'_k md_k, and E adds the deletes.
template <bool SHARE, bool FOLD>
__global__ void __launch_bounds__(64 * FWD_WPB) BOUND_OCC k_fwd_bound(FloatArgs a, int wave0, int nwaves, const float *__restrict__ btab, float *__restrict__ fb, ShareLaunch sl)
{
  const int wv = threadIdx.x >> 6, widx = blockIdx.x * FWD_WPB + wv;
  WaveDesc wd = a.waves[wave0 + min(widx, nwaves - 1)];
  if (widx >= nwaves) { wd.count = 0; wd.rows = 1; }          // (a block's spare waves: no lane, no row)
  const int lane = threadIdx.x & 63;
  const int prof = uni(wd.prof);
  const DevProfile *pp = a.prof + prof;
  // emission odds by node: en[code][k - 1], k = z Q + q + 1 in the striped table (one copy per wave: a run may end inside the block)
  __shared__ __attribute__((aligned(16))) float en_all[FWD_WPB][NCODE * 2 * BP];
  float *en = en_all[wv];
  const float *tab = btab + (size_t)prof * BOUND_TAB;
  const bool active = lane < wd.count;
  const int64_t pi = wd.first + (active ? lane : 0);
  const PairRec pr = a.pairs[pi];
  const int L = pr.L;
  // (two-sided schedule: the chain's record -- one 64-byte load instead of four dependent ones -- and the folded emission table as it
  // stands in memory; each wave fills and reads its OWN copy, so the wave's own order of LDS operations is all the fence it needs)
  const bool recs = SHARE && sl.chain != nullptr;
  ChainRec cr{};
  if (recs) { const f4 *q = (const f4 *)(sl.chain + pr.useq); const f4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3]; f4 *o = (f4 *)&cr; o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; }
  if (FOLD && recs && sl.entab) {
    const f4 *e4 = (const f4 *)(sl.entab + (size_t)prof * (NCODE * 2 * BP));
    for (int i = lane; i < NCODE * 2 * BP / 4; i += 64) ((f4 *)en)[i] = e4[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    const int Q = uni(pp->Q);
    const float *g = tab + (BP + 1) * 16;                      // FOLD: the match cells' scale by node
    for (int i = lane; i < NCODE * 2 * BP; i += 64) {
      const int x = i / (2 * BP), k0 = i % (2 * BP);           // node k0 + 1
      const float e = (k0 < 4 * Q) ? pp->rf[(x * QMAX + (k0 % Q)) * 4 + k0 / Q] : 0.0f;
      en[i] = FOLD ? e * g[k0] : e;
    }
    __syncthreads();
  }
  Seq sq;
  if (recs) { sq.w = a.rd.words + cr.woff; sq.exc = a.rd.exc + cr.excoff; sq.nexc = cr.nexc; sq.L = cr.L; }
  else sq = open_seq(a.rd, a.seed_read[a.sorted_uniq[pr.useq]]);
  int Lw = wd.rows - 1;
  f2 S[BP], Ip[BP];
#pragma unroll
  for (int j = 0; j < BP; j++) { S[j] = (f2){0.f, 0.f}; Ip[j] = (f2){0.f, 0.f}; }
  const float pmove = (2.0f + 1.0f) / ((float)L + 2.0f + 1.0f);
  const float ploop = 1.0f - pmove;
  float xE = 0.f, xN = 1.f, xJ = 0.f, xB = pmove, xC = 0.f;
  double totscale = 0.0;
  const int row0 = SHARE ? (sl.depth << sl.logB) : 0;       // rows done before this launch (wave-uniform)
  unsigned long long smask = 0ull; int64_t snode = 0;
  // two-sided sharing (round 6): the chain's last row, and the level at which it takes the rest of the sum over paths from a saved
  // Backward state (k_bwd_bound) instead of walking on to L
  int endrow = L, jlev = -1; int64_t jnode = 0;
  if constexpr (SHARE) {
    const int k = pr.useq;
    if (active) {
      if (recs) {
        smask = cr.mask; snode = (int64_t)cr.node0 - sl.node_base;
        endrow = cr.endrow; jlev = pr.xj >= 0 ? cr.jlev : -1; jnode = (int64_t)cr.jsrc - sl.gnode_base;
      } else {
        smask = sl.mask[k]; snode = (int64_t)sl.node0[k] - sl.node_base;
        if (sl.endrow) { endrow = sl.endrow[k]; jlev = pr.xj >= 0 ? sl.jlev[k] : -1; jnode = (int64_t)sl.jsrc[k] - sl.gnode_base; }
      }
    }
    // the wave runs to the last row of its longest chain: the maximum over its lanes (the shared schedule's descriptors carry no row
    // count: k_share.hip, k_share_wavelist); a spare wave has no lane and no row
    Lw = wave_max(active ? endrow : 0);
    if (sl.dbg & 1) Lw = row0;
    if (sl.dbg & 4) jlev = -1;
    if (sl.depth > 0 && !(sl.dbg & 2)) {
      const int64_t node = (int64_t)(recs ? cr.src : sl.src[k]) - sl.node_base;
      const f4 *src = (const f4 *)sl.slots + (node * sl.Pb + (prof - sl.p0)) * FWD_STATE_Q;
#pragma unroll
      for (int j = 0; j < BP; j++) { const f4 v = src[j]; S[j] = (f2){v.x, v.y}; Ip[j] = (f2){v.z, v.w}; }
      const f4 u = src[BP], t = src[BP + 1];
      xN = u.x; xJ = u.y; xC = u.z; xB = u.w;
      totscale = __builtin_bit_cast(double, (f2){t.x, t.y});
    }
  }
  SeqStream ss; ss.open(sq, row0, +1);
  int xnext = ss.get(row0);
  for (int i = row0 + 1; ; i++) {
    if constexpr (SHARE) {
      // a block boundary: the state after row i - 1 = d * B is what a chain that branches off there starts from
      if (((i - 1) & ((1 << sl.logB) - 1)) == 0) {
        const int d = (i - 1) >> sl.logB;
        if (d < 64 && ((smask >> d) & 1ull) && i - 1 > row0) {           // (a mask has no bit above the chain's last level)
          const int64_t node = snode + __popcll(smask & ((1ull << d) - 1ull));
          f4 *dst = (f4 *)sl.slots + (node * sl.Pb + (prof - sl.p0)) * FWD_STATE_Q;
#pragma unroll
          for (int j = 0; j < BP; j++) dst[j] = (f4){S[j].x, S[j].y, Ip[j].x, Ip[j].y};
          const f2 ts = __builtin_bit_cast(f2, totscale);
          dst[BP] = (f4){xN, xJ, xC, xB};
          dst[BP + 1] = (f4){ts.x, ts.y, 0.f, 0.f};
        }
        if (d == jlev) {
          // the join: every path crosses the cut after row d * B in exactly one of S_k (a cell of row d B on its way to the next row's
          // match cell M_k+1), I+_k (the next row's insert cell), N, J, C, B -- the score is the inner product of the Forward state with
          // the suffix's Backward state (same layout, dual units: k_bwd_bound), plus both scales
          const f4 *g = (const f4 *)sl.gslots + (jnode * sl.Pb + (prof - sl.p0)) * FWD_STATE_Q;
          f2 sa = (f2){0.f, 0.f}, sb = (f2){0.f, 0.f};
#pragma unroll
          for (int j = 0; j < BP; j++) { const f4 v = g[j]; sa = pfma(S[j], (f2){v.x, v.y}, sa); sb = pfma(Ip[j], (f2){v.z, v.w}, sb); }
          const f4 u = g[BP], t = g[BP + 1];
          sb = pfma((f2){xN, xJ}, (f2){u.x, u.y}, sb);
          sa = pfma((f2){xC, xB}, (f2){u.z, u.w}, sa);
          const float dot = (sa.x + sa.y) + (sb.x + sb.y);
          const double gscale = __builtin_bit_cast(double, (f2){t.x, t.y});
          const bool jbad = (dot != dot) || (dot <= 0.0f) || (dot == __builtin_inff());
          const float sc = jbad ? __builtin_nanf("") : (float)(totscale + gscale + det_log((double)dot));
          fb[pi] = sc;
          if (sl.b10) lazy_bound_put(sl, a.lt, pi, pr, sc);
        }
      }
    }
    if (i > Lw) break;
    if (i <= endrow) {
      const int x = xnext;
      if (i < L) xnext = ss.get(i);
      const float *ex = en + x * (2 * BP);
      const float *tb = tab + opaque_zero();
      const f2 xBv = (f2){xB, xB};
      f2 acc = (f2){0.f, 0.f};
      BT cur = ldbt(tb, 0);
      f2 ecur = *(const f2 *)(ex);
      float dprev = 0.0f, mdprev = 0.0f;         // D'[2j] and M'[2j] t(M->D) (FOLD: M'[2j] itself) of the node before the pair (none before node 1)
      float sprev = 0.0f;                        // the OLD row's S of the node before the pair (S[0] = 0)
      f2 mnp = (f2){0.f, 0.f}, dnp = mnp;        // the new match and delete cells of the pair before: they live for one step
      // One step = the chain of pair j (sh -> w -> mn -> dn.y: the new row's match and delete cells) and, between its links, what pair
      // j - 1's new cells leave for the next row (S' and I+': 5 instructions, independent of the chain).  An instruction that reads the
      // result of the one before it costs a wait state that the other waves only partly fill (profiles/round5_valu_issue.md), so the
      // order is fixed by hand -- every statement fenced -- and no instruction follows its producer directly.  The old S of pair j - 1
      // goes into sh before the new one is written.
#define SB __builtin_amdgcn_sched_barrier(0)
#pragma unroll
      for (int j = 0; j <= BP; j++) {
        __builtin_amdgcn_s_waitcnt(0xC07F);     // lgkmcnt(0): record j and pair j's emissions, requested one step ago
        const bool chain = j < BP, fin = j > 0;
        const BT c = cur; const f2 e = ecur;
        if (chain) { cur = ldbt(tb, j + 1); if (j + 1 < BP) ecur = *(const f2 *)(ex + 2 * (j + 1)); }
        SB;
        f2 sh = (f2){0.f, 0.f}, t = sh, u = sh, w = sh, mn = sh, md = sh, dn = sh;
        if (chain) { sh = (f2){sprev, S[j].x}; sprev = S[j].y; SB; }
        if (fin) { t = Ip[j - 1] * c.im; SB; if constexpr (!FOLD) { u = Ip[j - 1] * c.ii; SB; } }
        // both new delete cells of the pair are born in this step: dd1 = D_2j -> D_2j+1 (0 for j = 0), dd2 = D_2j+1 -> D_2j+2
        // (as inline assembly: left to itself the compiler accumulates into the dying product's register -- v_fmac -- and then
        // moves the result into the pair, twice per pair of nodes and row)
        if (chain) { asm("v_fma_f32 %0, %1, %2, %3" : "=v"(dn.x) : "v"(dprev), "s"(c.dd1), "v"(mdprev)); SB; }
        if (chain) { w = pfma(xBv, c.bm, sh); SB; }
        if (fin) { t = pfma(dnp, c.dm, t); SB; }
        if (chain) { mn = w * e; SB; }
        if (fin) { S[j - 1] = pfma(mnp, c.mm, t); SB; }
        if constexpr (FOLD) {
          if (chain) { acc = acc + mn; SB; }
          if (fin) { Ip[j - 1] = pfma(Ip[j - 1], c.ii, mnp); SB; }             // (the insert cells divided by t(M_k -> I_k) / g_k)
          if (chain) { asm("v_fma_f32 %0, %1, %2, %3" : "=v"(dn.y) : "v"(dn.x), "s"(c.dd2), "v"(mn.x)); SB; mdprev = mn.y; }
        } else {
          if (chain) { md = mn * c.md; SB; acc = acc + mn; SB; }
          if (fin) { Ip[j - 1] = pfma(mnp, c.mi, u); SB; acc = acc + dnp; SB; }
          if (chain) { asm("v_fma_f32 %0, %1, %2, %3" : "=v"(dn.y) : "v"(dn.x), "s"(c.dd2), "v"(md.x)); SB; mdprev = md.y; }
        }
        mnp = mn; dnp = dn; dprev = dn.y;
      }
#undef SB
      xE = acc.x + acc.y;
      xN = xN * ploop;
      xC = __builtin_fmaf(xC, ploop, xE * 0.5f);
      xJ = __builtin_fmaf(xJ, ploop, xE * 0.5f);
      xB = (xJ + xN) * pmove;
      // (1e20; at 1e28 -- most targets never get here, a 45-node domain multiplies E by up to ~1e25 -- pass A takes the same 1.600 s per
      // 10 M reads: ITSX_BOUND_RESCALE_EXP)
      if (xE > sl.rescale) {
        const float r = 1.0f / xE;
        xN *= r; xC *= r; xJ *= r; xB *= r;
        const f2 rv = (f2){r, r};
#pragma unroll
        for (int j = 0; j < BP; j++) { S[j] = S[j] * rv; Ip[j] = Ip[j] * rv; }
        totscale += det_log((double)xE);
        xE = 1.0f;
      }
    }
  }
  const bool bad = (xC != xC) || (xC == 0.0f) || (xC == __builtin_inff());
  if (active && jlev < 0) {
    const float sc = bad ? __builtin_nanf("") : (float)(totscale + det_log((double)(xC * pmove)));
    fb[pi] = sc;
    if (sl.b10) lazy_bound_put(sl, a.lt, pi, pr, sc);
  }
}

// =========================================================================================
// Round 6, two-sided sharing: the BACKWARD half of pass A's sum over paths.  One Forward row is a linear map of the row state
// (S, I+ of 46 nodes, N, J, C, B: k_fwd_bound's folded units); the score is a linear functional of the last row's state (C times
// the move out).  Pulled back through the rows L, L - 1, ..., j B + 1 -- the TRANSPOSED maps, applied in that order -- it becomes a
// vector gamma_j with   score = < Forward state after row j B, gamma_j >   for EVERY prefix, and gamma_j depends on the profile, the
// target's length and the residues after row j B only: the uniques of one length that end alike share it.  This kernel walks a
// Backward chain (lane = chain x profile, wave = 64 chains of one (batch, blocks-from-the-end) segment) and saves gamma at the block
// boundaries where somebody joins (k_share.hip: k_join_*), in k_fwd_bound's state layout, so that the join is 48 packed multiply-adds.
// What it carries is the dual of Forward's (S, I+): W_k = w_k+1 of the last row pulled back, the adjoint of S_k, and G_k, the adjoint of
// I+_k -- the gI that row was entered with; the adjoints of the row's own cells are formed from them on the fly:
//     gM_k = mm_k W_k + G_k,   gD_k = dm_k W_k,   G_k <- im_k W_k + ii_k G_k,   W_k <- w_k+1
//     score = sum_k S_k W_k + sum_k I+_k G_k + N gN + J gJ + C gC + B gB        (plus both scale logarithms)
// The transposed row, with a' = adjoint of the new row's cell and x the row's residue:
//     nJ = gJ + move gB,  nN = gN + move gB,  aE = (nJ + gC) / 2
//     aD_k = gD_k + dd_k aD_k+1,   aM_k = gM_k + aE + aD_k+1,   w_k = e_k(x) aM_k                  (k = 46 .. 1, aD_47 = w_47 = 0)
//     gM_k <- mm_k w_k+1 + gI_k,   gI_k <- im_k w_k+1 + ii_k gI_k,   gD_k <- dm_k w_k+1,   gB <- sum_k bm_k w_k
//     gN <- loop nN,  gJ <- loop nJ,  gC <- loop gC
// (the same table entries as the Forward kernel's, by pair of nodes: engine.hip builds rtab).  The cells are kept below ~1e6 by a sum test
// every 16 rows (block boundaries are multiples of 16), the scale's logarithm travels with the state like Forward's.
// record j of the table (engine.hip: install_profiles): bm of pair j; mm im dm, ii and dd (aa) of pair j - 1 -- what ONE step of the
// row loop below reads: the late half of pair j and the early half of pair j - 1 (record BP: the last pair's early half alone)
struct RT { f2 mm, im, dm, bm, ii, aa; };
DEV RT ldrt(const float *tab, int j)
{
  const f4 a = *(cf4q)(uintptr_t)(tab + j * 12), b = *(cf4q)(uintptr_t)(tab + j * 12 + 4), c = *(cf4q)(uintptr_t)(tab + j * 12 + 8);
  RT t;
  t.mm = (f2){a.x, a.y}; t.im = (f2){a.z, a.w}; t.dm = (f2){b.x, b.y}; t.bm = (f2){b.z, b.w}; t.ii = (f2){c.x, c.y}; t.aa = (f2){c.z, c.w};
  return t;
}
__global__ void __launch_bounds__(64 * FWD_WPB) BOUND_OCC k_bwd_bound(FloatArgs a, int wave0, int nwaves, const float *__restrict__ btab, const float *__restrict__ rtab, ShareLaunch sl)
{
  const int wv = threadIdx.x >> 6, widx = blockIdx.x * FWD_WPB + wv;
  WaveDesc wd = a.waves[wave0 + min(widx, nwaves - 1)];
  if (widx >= nwaves) { wd.count = 0; wd.rows = 1; }
  const int lane = threadIdx.x & 63;
  const int prof = uni(wd.prof);
  const DevProfile *pp = a.prof + prof;
  __shared__ __attribute__((aligned(16))) float en_all[FWD_WPB][NCODE * 2 * BP];
  float *en = en_all[wv];
  const float *tab = rtab + (size_t)prof * BOUND_RTAB;
  (void)pp; (void)btab;
  const bool active = lane < wd.count;
  const int64_t pi = wd.first + (active ? lane : 0);
  const PairRec pr = a.pairs[pi];
  const int L = pr.L;
  ChainRec cr;
  { const f4 *q = (const f4 *)(sl.chain + pr.useq); const f4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3]; f4 *o = (f4 *)&cr; o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; }
  {
    const f4 *e4 = (const f4 *)(sl.entab + (size_t)prof * (NCODE * 2 * BP));
    for (int i = lane; i < NCODE * 2 * BP / 4; i += 64) ((f4 *)en)[i] = e4[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  Seq sq; sq.w = a.rd.words + cr.woff; sq.exc = a.rd.exc + cr.excoff; sq.nexc = cr.nexc; sq.L = cr.L;
  const int nsteps = (sl.dbg & 32) ? 0 : wave_max(active ? cr.endrow : 0);         // the wave's longest chain (no lane: no step)
  f2 W[BP], G[BP];
#pragma unroll
  for (int j = 0; j < BP; j++) { W[j] = (f2){0.f, 0.f}; G[j] = (f2){0.f, 0.f}; }
  const float pmove = (2.0f + 1.0f) / ((float)L + 2.0f + 1.0f);
  const float ploop = 1.0f - pmove;
  float xN = 0.f, xJ = 0.f, xB = 0.f, xC = pmove;            // gamma after the last row: the score is C times the move out
  double totscale = 0.0;
  const int kb = pr.useq;
  const int rd = sl.depth;                                    // blocks from the end the launch's chains start at (wave-uniform)
  unsigned long long smask = 0ull; int64_t snode = 0; int mysteps = 0;
  (void)kb;
  if (active) { smask = cr.mask; snode = (int64_t)cr.node0 - sl.node_base; mysteps = cr.endrow; }
  if (rd > 0 && !(sl.dbg & 16)) {
    const int64_t node = (int64_t)cr.src - sl.node_base;
    const f4 *src = (const f4 *)sl.slots + (node * sl.Pb + (prof - sl.p0)) * FWD_STATE_Q;
#pragma unroll
    for (int j = 0; j < BP; j++) { const f4 v = src[j]; W[j] = (f2){v.x, v.y}; G[j] = (f2){v.z, v.w}; }
    const f4 u = src[BP], t = src[BP + 1];
    xN = u.x; xJ = u.y; xC = u.z; xB = u.w;
    totscale = __builtin_bit_cast(double, (f2){t.x, t.y});
  }
  const int A =(L + (1 << sl.logB) - 1) >> sl.logB;
  const int top = (A - rd) << sl.logB;                        // the row the chain's state stands after (virtual when rd = 0 and L is no multiple of B)
  const int first = top < L ? top : L;
  SeqStream ss; ss.open(sq, first > 0 ? first - 1 : 0, -1);
  int xnext = first > 0 ? ss.get(first - 1) : 0;
  for (int step = 0; ; step++) {
    if ((step & ((1 << sl.logB) - 1)) == 0 && step > 0) {
      // a block boundary: gamma after row top - step = (A - rdl) B is what the Forward chains that end there take
      const int rdl = rd + (step >> sl.logB);
      if (active && rdl < 64 && ((smask >> rdl) & 1ull) && !(sl.dbg & 8)) {
        const int64_t node = snode + __popcll(smask & ((1ull << rdl) - 1ull));
        f4 *dst = (f4 *)sl.slots + (node * sl.Pb + (prof - sl.p0)) * FWD_STATE_Q;
#pragma unroll
        for (int j = 0; j < BP; j++) dst[j] = (f4){W[j].x, W[j].y, G[j].x, G[j].y};
        const f2 ts = __builtin_bit_cast(f2, totscale);
        dst[BP] = (f4){xN, xJ, xC, xB};
        dst[BP + 1] = (f4){ts.x, ts.y, 0.f, 0.f};
      }
    }
    if (step >= nsteps) break;
    const int row = top - step;                               // this step pulls gamma back through row `row`
    if (row <= L && step < mysteps) {
      const int x = xnext;
      if (row > 1) xnext = ss.get(row - 2);
      const float *ex = en + x * (2 * BP);
      const float *tb = tab + opaque_zero();
      const float gb0 = xB * pmove;
      const float nJ = xJ + gb0, nN = xN + gb0;
      const float aE = 0.5f * (nJ + xC);
      const f2 aEv = (f2){aE, aE};
      float aDn = 0.0f, wn = 0.0f;                            // aD and w of the node after the pair
      f2 accB = (f2){0.f, 0.f};
      // One step = the LATE half of pair j (w = e aM, its share of B, the pair's new W) and the EARLY half of pair j - 1 (gD, gM and the new
      // G from its W and G, its aD chain -- two dependent multiply-adds --, aM), statement by statement in a fixed order so that no
      // instruction reads the result of the one before it (at two waves per SIMD that costs a wait state the other wave only half fills:
      // the compiler's own order ran at 0.87 ns per wave-row against the Forward step's 0.56); the step's table record (engine.hip: what
      // both halves read, 12 floats) and emission odds are requested one step ahead, as in the Forward step.
#define SB __builtin_amdgcn_sched_barrier(0)
      RT cur = ldrt(tb, BP);                                  // mm im dm ii dd of the last pair
      f2 ecur = (f2){0.f, 0.f};
      f2 aM = (f2){0.f, 0.f};
#pragma unroll
      for (int j = BP; j >= 0; j--) {
        __builtin_amdgcn_s_waitcnt(0xC07F);                   // lgkmcnt(0): step j's record and pair j's emissions, requested one step ago
        const RT t = cur;
        const f2 e = ecur;
        const bool late = j < BP, more = j > 0;
        if (more) { cur = ldrt(tb, j - 1); ecur = *(const f2 *)(ex + 2 * (j - 1)); }
        SB;
        f2 w = (f2){0.f, 0.f}, gD = w, pren = w, gMp = w, iig = w, aMn = w;
        float aD2n = 0.f, aD1n = 0.f;
        if (late) { w = aM * e; SB; }
        if (more) { gD = t.dm * W[j - 1]; SB; }               // the adjoints of the row's cells, from (W, G): gD = dm W, gM = mm W + G
        if (late) { accB = pfma(t.bm, w, accB); SB; }
        if (more) { pren = G[j - 1] + aEv; SB; }
        if (more) { aD2n = __builtin_fmaf(t.aa.y, aDn, gD.y); SB; }
        if (late) { W[j] = (f2){w.y, wn}; SB; }               // w of the node after each of the pair's two (the old W[j] was read one step ago)
        if (more) { gMp = pfma(t.mm, W[j - 1], pren); SB; }   // gM + aE
        if (more) { aD1n = __builtin_fmaf(t.aa.x, aD2n, gD.x); SB; }
        if (more) { iig = t.ii * G[j - 1]; SB; }
        if (more) { aMn = gMp + (f2){aD2n, aDn}; SB; }
        if (more) { G[j - 1] = pfma(t.im, W[j - 1], iig); SB; }
        wn = w.x; aDn = aD1n; aM = aMn;
      }
#undef SB
      xB = accB.x + accB.y;
      xN = ploop * nN; xJ = ploop * nJ; xC = ploop * xC;
    }
    if ((step & 15) == 15) {
      f2 sm = (f2){0.f, 0.f};
#pragma unroll
      for (int j = 0; j < BP; j++) sm = sm + (W[j] + G[j]);
      const float tot = (sm.x + sm.y) + ((xN + xJ) + (xC + xB));
      if (tot > 1e6f || (tot < 1e-6f && tot > 0.0f)) {
        const float r = 1.0f / tot;
        const f2 rv = (f2){r, r};
#pragma unroll
        for (int j = 0; j < BP; j++) { W[j] = W[j] * rv; G[j] = G[j] * rv; }
        xN *= r; xJ *= r; xC *= r; xB *= r;
        totscale += det_log((double)tot);
      }
    }
  }
}
void launch_bwd_bound_share(const FloatArgs &a, const float *btab, const float *rtab, int nwaves, int wave0, const ShareLaunch &sl, hipStream_t st)
{
  if (nwaves <= 0) return;
  const dim3 g((nwaves + FWD_WPB - 1) / FWD_WPB), b(64 * FWD_WPB);
  hipLaunchKernelGGL(k_bwd_bound, g, b, 0, st, a, wave0, nwaves, btab, rtab, sl);
}

// 1e20 by default (ITSX_BOUND_RESCALE_EXP: another power of ten, for A/B; at most 28 -- the folded cells must stay inside float)
static float bound_rescale()
{
  // (read at every launch: a process can run an A/B of it)
  const char *e = sw_get("ITSX_BOUND_RESCALE_EXP");
  const double x = e ? atof(e) : 20.0;
  return (float)pow(10.0, x < 4.0 ? 4.0 : x > 28.0 ? 28.0 : x);
}
void launch_fwd_bound_seq(const FloatArgs &a, const float *btab, bool fold, float *fb, int nwaves, int wave0, hipStream_t st)
{
  if (nwaves <= 0) return;
  ShareLaunch none{}; none.rescale = bound_rescale();
  const dim3 g((nwaves + FWD_WPB - 1) / FWD_WPB), b(64 * FWD_WPB);
  if (fold) hipLaunchKernelGGL((k_fwd_bound<false, true>), g, b, 0, st, a, wave0, nwaves, btab, fb, none);
  else hipLaunchKernelGGL((k_fwd_bound<false, false>), g, b, 0, st, a, wave0, nwaves, btab, fb, none);
}
void launch_fwd_bound_share(const FloatArgs &a, const float *btab, bool fold, float *fb, int nwaves, int wave0, const ShareLaunch &sl0, hipStream_t st)
{
  if (nwaves <= 0) return;
  ShareLaunch sl = sl0; sl.rescale = bound_rescale();
  const dim3 g((nwaves + FWD_WPB - 1) / FWD_WPB), b(64 * FWD_WPB);
  if (fold) hipLaunchKernelGGL((k_fwd_bound<true, true>), g, b, 0, st, a, wave0, nwaves, btab, fb, sl);
  else hipLaunchKernelGGL((k_fwd_bound<true, false>), g, b, 0, st, a, wave0, nwaves, btab, fb, sl);
}

// largest %.1f tenths (biased) a domain of each pair can print, and the best-bound pair of every (representative, class)
__global__ void __launch_bounds__(256) k_lazy_bound(LazyArgs a)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.NP) return;
  const PairRec pr = a.pairs[i];
  if (pr.prof < 0) { a.b10[i] = 0u; return; }
  if (pr.xj < 0) { a.b10[i] = 0u; a.done[i] = 1; return; }      // ran for its row states only (k_share.hip): never selected
  const uint32_t b = lazy_tenths(a.fb[i], a.lt[pr.L]);
  a.b10[i] = b;
  const size_t g = (size_t)pr.useq * a.ncls + a.cls[pr.prof];
  atomicMax(&a.gtop[g], ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i));
}

// ---- selection: a round's pairs are marked in ONE bit each (smask[c] = the ballot of chunk c = pairs [64 c, 64 c + 64), scnt[c] its
// popcount; scnt[nch] = 0 so that the scan's last element is the total), the chunk counts are scanned (NP / 64 elements), and the set
// bits are scattered.  Profile segments start at multiples of 64: a chunk lies inside one segment, and the rank of a pair inside its
// profile is spos[its chunk] + the set bits below it - spos[the segment's first chunk].
__device__ __forceinline__ void select_store(int64_t i, int64_t nch, int f, unsigned long long *__restrict__ smask, int32_t *__restrict__ scnt)
{
  const unsigned long long m = __ballot(f);
  if ((threadIdx.x & 63) == 0) {
    const int64_t c = i >> 6;
    if (c < nch) smask[c] = m;
    scnt[c] = (int32_t)__popcll(m);      // (chunk nch: no pair, 0)
  }
}

// round 0: the best-bound pair of each group, taken from the GROUPS (a few per cent as many as there are pairs): gtop names the pair,
// the pair's record confirms that it is one of the group's (so the selection is what asking every pair "am I my group's best?" gives,
// whatever the table holds), and its bit goes into the zeroed masks; k_select_count then counts each chunk's bits.
__global__ void __launch_bounds__(256) k_lazy_first(LazyArgs a)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.ngroups) return;
  const unsigned long long top = a.gtop[g];
  const int64_t i = (int64_t)(0xFFFFFFFFu - (uint32_t)(top & 0xFFFFFFFFull));
  if (i >= a.NP) return;                                        // (an empty group: top == 0)
  const PairRec pr = a.pairs[i];
  if (pr.prof < 0 || a.done[i] || (int64_t)pr.useq * a.ncls + a.cls[pr.prof] != g) return;
  a.done[i] = 1;
  atomicOr(&a.smask[i >> 6], 1ull << (i & 63));
}
__global__ void __launch_bounds__(256) k_select_count(const unsigned long long *__restrict__ smask, int64_t nch, int32_t *__restrict__ scnt)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= nch) scnt[c] = c < nch ? (int32_t)__popcll(smask[c]) : 0;
}
// round 1: everything not yet evaluated that could still beat (or tie with) the group's best certain row; all of a group that has none.
// The group's row is asked for by 691 M pairs but there are only chunk uniques x ncls groups, and bestc lies by GLOBAL unique index: a
// gather at random for every pair.  k_lazy_thr first lays the one number a pair compares with -- the row's tenths, 0 for a group that has
// no certain row (every bound is >= 0: all of it selected) -- by sorted position, thr[useq * ncls + class]; useq ascends inside a profile
// segment, so a wave of the marking kernel then reads consecutive words.
__global__ void __launch_bounds__(256) k_lazy_thr(LazyArgs a)
{
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.nthr) return;
  const int64_t su = a.sorted_uniq[g / a.ncls], idx = su * a.ncls + g % a.ncls;
  const unsigned long long bc = (su >= 0 && idx < a.nbest) ? a.bestc[idx] : 0ull;      // (a position no pair names may point anywhere)
  a.thr[g] = (uint32_t)(bc >> 40);
}
// A wave of a marking kernel takes MARK_K consecutive chunks, a lane one pair of each: the MARK_K records, flags and bounds are
// requested before the first of them is used, then the MARK_K loads that hang on them, level by level (one pair per thread went through
// pair -> sorted_uniq -> bestc as one chain of latencies).  Chunk c is still the ballot of pairs [64 c, 64 c + 64), and chunk nch (no
// pair: count 0) is still covered.
constexpr int MARK_K = 4;
static inline unsigned select_grid(int64_t NP) { const int64_t nw = (((NP + 63) >> 6) + 1 + MARK_K - 1) / MARK_K; return (unsigned)((nw + 3) / 4); }
__global__ void __launch_bounds__(256) k_lazy_mark(LazyArgs a)
{
  const int lane = threadIdx.x & 63;
  const int64_t nch = (a.NP + 63) >> 6;
  const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * MARK_K;
  if (c0 > nch) return;                                         // (whole waves)
  PairRec pr[MARK_K]; uint8_t dn[MARK_K]; uint32_t b[MARK_K], t[MARK_K]; int cl[MARK_K]; bool live[MARK_K];
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    const int64_t i = (c0 + k) * 64 + lane;
    pr[k].useq = 0; pr[k].prof = -1; pr[k].xj = -1; pr[k].L = 0; dn[k] = 1; b[k] = 0;
    if (i < a.NP) { pr[k] = a.pairs[i]; dn[k] = a.done[i]; b[k] = a.b10[i]; }
  }
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    live[k] = pr[k].prof >= 0 && !dn[k];
    cl[k] = 0;
    if (live[k]) cl[k] = a.cls[pr[k].prof];
  }
#pragma unroll
  for (int k = 0; k < MARK_K; k++) { t[k] = 0u; if (live[k]) t[k] = a.thr[(size_t)pr[k].useq * a.ncls + cl[k]]; }
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    const int64_t c = c0 + k;
    if (c > nch) break;                                         // (wave-uniform)
    const int f = live[k] && b[k] >= t[k];
    if (f) a.done[c * 64 + lane] = 1;
    select_store(c * 64 + lane, nch, f, a.smask, a.scnt);
  }
}

// selected pairs keep their profile segment and their order inside it (ascending length): out[seg_new[p] + rank inside p].
// One wave takes SCATTER_CHUNKS chunks, one after the other; a chunk without a set bit costs it one 8-byte load.
constexpr int SCATTER_CHUNKS = 16;
__global__ void __launch_bounds__(256) k_lazy_scatter(const PairRec *__restrict__ pairs, int64_t NP, const unsigned long long *__restrict__ smask,
                                                      const int32_t *__restrict__ spos, const int64_t *__restrict__ seg_old,
                                                      const int64_t *__restrict__ seg_new, PairRec *__restrict__ out, int32_t *__restrict__ src)
{
  const int lane = threadIdx.x & 63;
  const int64_t nch = (NP + 63) >> 6;
  const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * SCATTER_CHUNKS;
  for (int k = 0; k < SCATTER_CHUNKS; k++) {
    const int64_t c = c0 + k;
    if (c >= nch) return;
    const unsigned long long m = smask[c];
    if (!((m >> lane) & 1ull)) continue;
    const int64_t i = c * 64 + lane;                            // (< NP: a bit is set only for a pair)
    const PairRec pr = pairs[i];
    const int32_t rank = spos[c] + (int32_t)__popcll(m & ((1ull << lane) - 1ull)) - spos[seg_old[pr.prof] >> 6];
    out[seg_new[pr.prof] + (int64_t)rank] = pr;
    if (src) src[seg_new[pr.prof] + (int64_t)rank] = (int32_t)i;     // (the count-only top-up round finds a pair's done flag again by it)
  }
}

__global__ void __launch_bounds__(256) k_finalize_lazy(itsx_domain *__restrict__ dom, int64_t n, const int64_t *__restrict__ zlb,
                                                       const int64_t *__restrict__ zub, double domE, const int32_t *__restrict__ usample, int P)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const itsx_domain d = dom[i];
  if (d.dom_idx < 0) return;
  int rep = 0;
  if (d.seq_reported) {
    const size_t z = (size_t)(usample ? usample[d.rep] * P : 0) + d.prof;
    const double p = det_exp(d.lnP);
    // this target is reported itself, so the true count is at least 1 and at least the lower bound
    const double lo = (double)(zlb[z] > 1 ? zlb[z] : 1), hi = (double)(zub[z] > 1 ? zub[z] : 1);
    rep = (p * hi <= domE) ? 1 : (p * lo <= domE) ? 2 : 0;
  }
  dom[i].dom_reported = rep;
}

__global__ void __launch_bounds__(256) k_lazy_sure(const itsx_domain *__restrict__ dom, int64_t n, const int8_t *__restrict__ cls, int ncls,
                                                   unsigned long long *__restrict__ sure, int32_t *__restrict__ has)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const itsx_domain d = dom[i];
  if (d.dom_idx < 0 || d.dom_reported != 1) return;
  has[d.rep] = 1;
  atomicMax(&sure[(size_t)d.rep * ncls + cls[d.prof]], rank_key(d));
}
__global__ void __launch_bounds__(256) k_lazy_pending(const itsx_domain *__restrict__ dom, int64_t n, const int8_t *__restrict__ cls, int ncls,
                                                      const unsigned long long *__restrict__ sure, const int32_t *__restrict__ has,
                                                      unsigned long long *__restrict__ count, int32_t *__restrict__ prof_flag,
                                                      uint8_t *__restrict__ uniq_flag, unsigned long long *__restrict__ zneed, const unsigned long long *__restrict__ zsplit,
                                                      double domE)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int c = 0;
  if (i < n) {
    const itsx_domain d = dom[i];
    // an undecided row matters when it would beat its group's best sure row, or when the sequence has no sure row at all
    if (d.dom_idx >= 0 && d.dom_reported == 2) c = !has[d.rep] || rank_key(d) > sure[(size_t)d.rep * ncls + cls[d.prof]];
    if (c) {
      prof_flag[d.prof] = 1; uniq_flag[d.rep] = 1;
      // the row is NOT reported as soon as the profile's reported targets exceed domE / P-value: the count that settles it (the top-up
      // round of itsx_search_finalize evaluates that many more of the profile's best pairs before anything is counted in full)
      // ... and it IS reported as soon as the UPPER bound falls to domE / P-value.  zneed[2 p] = the largest such count at or below the
      // profile's split (settled from below: more of its best pairs), zneed[2 p + 1] = the smallest one above it (settled from above:
      // its weakest pairs shown unreported); the split lies between the profile's two bounds (finalize_lazy)
      if (zneed) {
        const double z = domE / det_exp(d.lnP);
        if (z < 9.0e18) {
          const unsigned long long zf = (unsigned long long)z;
          if (zf + 2ull <= zsplit[d.prof]) atomicMax(&zneed[2 * d.prof], zf + 2ull);
          else atomicMin(&zneed[2 * d.prof + 1], zf > 2ull ? zf - 2ull : 0ull);
        } else atomicMin(&zneed[2 * d.prof + 1], (unsigned long long)9.0e18);
      }
    }
  }
  const unsigned long long m = __ballot(c);
  if (m && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(count, (unsigned long long)__builtin_popcountll(m));
}

__global__ void __launch_bounds__(64) k_pad_b10(const int64_t *__restrict__ seg_start, const int32_t *__restrict__ total, uint32_t *__restrict__ b10)
{
  const int64_t e = seg_start[blockIdx.x] + total[blockIdx.x] + threadIdx.x;      // (at most 63 records)
  if (e < seg_start[blockIdx.x + 1]) b10[e] = 0u;
}
void launch_pad_b10(int32_t P, const int64_t *seg_start, const int32_t *total, uint32_t *b10, hipStream_t st)
{
  if (P > 0) hipLaunchKernelGGL(k_pad_b10, dim3((unsigned)P), dim3(64), 0, st, seg_start, total, b10);
}
void launch_lazy_bound(const LazyArgs &a, hipStream_t st)
{
  if (a.NP > 0) hipLaunchKernelGGL(k_lazy_bound, dim3((unsigned)((a.NP + 255) / 256)), dim3(256), 0, st, a);
}
void launch_lazy_mark(const LazyArgs &a, int round, hipStream_t st)
{
  const int64_t nch = (a.NP + 63) >> 6;
  if (round == 0) {
    (void)hipMemsetAsync(a.smask, 0, (size_t)nch * sizeof(unsigned long long), st);
    if (a.ngroups > 0) hipLaunchKernelGGL(k_lazy_first, dim3((unsigned)((a.ngroups + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_select_count, dim3((unsigned)((nch + 1 + 255) / 256)), dim3(256), 0, st, a.smask, nch, a.scnt);
  } else {
    if (a.nthr > 0) hipLaunchKernelGGL(k_lazy_thr, dim3((unsigned)((a.nthr + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lazy_mark, dim3(select_grid(a.NP)), dim3(256), 0, st, a);
  }
}
void launch_lazy_scatter(const PairRec *pairs, int64_t NP, const unsigned long long *smask, const int32_t *spos, const int64_t *seg_old, const int64_t *seg_new,
                         PairRec *out, hipStream_t st, int32_t *src)
{
  const int64_t nch = (NP + 63) >> 6, per_block = 4 * SCATTER_CHUNKS;
  if (NP > 0) hipLaunchKernelGGL(k_lazy_scatter, dim3((unsigned)((nch + per_block - 1) / per_block)), dim3(256), 0, st, pairs, NP, smask, spos, seg_old, seg_new, out, src);
}
void launch_finalize_lazy(itsx_domain *dom, int64_t n, const int64_t *zlb, const int64_t *zub, double domE, const int32_t *usample, int P, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_finalize_lazy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dom, n, zlb, zub, domE, usample, P);
}
void launch_lazy_sure(const itsx_domain *dom, int64_t n, const int8_t *cls, int ncls, unsigned long long *sure, int32_t *has, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_lazy_sure, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dom, n, cls, ncls, sure, has);
}
void launch_lazy_pending(const itsx_domain *dom, int64_t n, const int8_t *cls, int ncls, const unsigned long long *sure, const int32_t *has,
                         unsigned long long *count, int32_t *prof_flag, uint8_t *uniq_flag, unsigned long long *zneed, const unsigned long long *zsplit, double domE, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_lazy_pending, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dom, n, cls, ncls, sure, has, count, prof_flag, uniq_flag, zneed, zsplit, domE);
}
// evaluated pairs (done flags) of the listed profiles' segments: cnt[slot] (zeroed); grid (blocks per profile, slots)
__global__ void __launch_bounds__(256) k_topup_count(const uint8_t *__restrict__ done, const int64_t *__restrict__ seg_start, const int32_t *__restrict__ total,
                                                     const int32_t *__restrict__ prof_of_slot, unsigned long long *__restrict__ cnt)
{
  const int sl = blockIdx.y, p = prof_of_slot[sl];
  const int64_t base = seg_start[p], n = total[p];
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) c += done[base + i] != 0;
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt[sl], c);
}
void launch_topup_count(const uint8_t *done, const int64_t *seg_start, const int32_t *total, const int32_t *prof_of_slot, int nslots, unsigned long long *cnt, hipStream_t st)
{
  if (nslots > 0) hipLaunchKernelGGL(k_topup_count, dim3(512, (unsigned)nslots), dim3(256), 0, st, done, seg_start, total, prof_of_slot, cnt);
}

// ---- the top-up round (itsx_search_finalize): the unevaluated pairs of the profiles that have undecided rows, best bound first
// pass 0 (spos == nullptr): the bit of pair i = it belongs to a profile with undecided rows and has not been evaluated (smask / scnt as in
// k_lazy_mark); pass 1: the key [slot | ~bound] of every marked pair into the compact list at its rank
__global__ void __launch_bounds__(256) k_topup_keys(const PairRec *__restrict__ pairs, int64_t NP, const uint8_t *__restrict__ done, const uint32_t *__restrict__ b10,
                                                    const int32_t *__restrict__ slot_of_prof, unsigned long long *__restrict__ smask, int32_t *__restrict__ scnt,
                                                    const int32_t *__restrict__ spos, unsigned long long *__restrict__ keys, int32_t *__restrict__ vals)
{
  const int lane = threadIdx.x & 63;
  const int64_t nch = (NP + 63) >> 6;
  const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * MARK_K;
  if (c0 > nch) return;
  if (!spos) {
    PairRec pr[MARK_K]; uint8_t dn[MARK_K];
#pragma unroll
    for (int k = 0; k < MARK_K; k++) {
      const int64_t i = (c0 + k) * 64 + lane;
      pr[k].useq = 0; pr[k].prof = -1; pr[k].xj = -1; pr[k].L = 0; dn[k] = 1;
      if (i < NP) { pr[k] = pairs[i]; dn[k] = done[i]; }
    }
    int sl[MARK_K];
#pragma unroll
    for (int k = 0; k < MARK_K; k++) { sl[k] = -1; if (pr[k].prof >= 0 && pr[k].xj >= 0 && !dn[k]) sl[k] = slot_of_prof[pr[k].prof]; }
#pragma unroll
    for (int k = 0; k < MARK_K; k++) {
      if (c0 + k > nch) break;
      select_store((c0 + k) * 64 + lane, nch, sl[k] >= 0, smask, scnt);
    }
    return;
  }
  // (a chunk without a set bit costs its wave one 8-byte load)
  unsigned long long m[MARK_K];
#pragma unroll
  for (int k = 0; k < MARK_K; k++) m[k] = c0 + k < nch ? smask[c0 + k] : 0ull;
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    if (!((m[k] >> lane) & 1ull)) continue;
    const int64_t i = (c0 + k) * 64 + lane;                     // (< NP: a bit is set only for a pair)
    const int32_t at = spos[c0 + k] + (int32_t)__popcll(m[k] & ((1ull << lane) - 1ull));
    const int sl = slot_of_prof[pairs[i].prof];
    keys[at] = ((unsigned long long)sl << 32) | (unsigned long long)(0xFFFFFFFFu - b10[i]); vals[at] = (int32_t)i;
  }
}
__global__ void __launch_bounds__(256) k_topup_mark(const PairRec *__restrict__ pairs, int64_t NP, uint8_t *__restrict__ done, const uint32_t *__restrict__ b10,
                                                    const int32_t *__restrict__ slot_of_prof, const uint32_t *__restrict__ cutoff,
                                                    unsigned long long *__restrict__ smask, int32_t *__restrict__ scnt)
{
  // cutoff[2 slot] > 0: the pairs whose bound is at least that (the best ones); cutoff[2 slot + 1] > 0: those whose bound is at most that
  const int lane = threadIdx.x & 63;
  const int64_t nch = (NP + 63) >> 6;
  const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * MARK_K;
  if (c0 > nch) return;
  PairRec pr[MARK_K]; uint8_t dn[MARK_K]; uint32_t b[MARK_K];
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    const int64_t i = (c0 + k) * 64 + lane;
    pr[k].useq = 0; pr[k].prof = -1; pr[k].xj = -1; pr[k].L = 0; dn[k] = 1; b[k] = 0;
    if (i < NP) { pr[k] = pairs[i]; dn[k] = done[i]; b[k] = b10[i]; }
  }
  int sl[MARK_K];
#pragma unroll
  for (int k = 0; k < MARK_K; k++) { sl[k] = -1; if (pr[k].prof >= 0 && pr[k].xj >= 0 && !dn[k]) sl[k] = slot_of_prof[pr[k].prof]; }
  uint32_t hi[MARK_K], lo[MARK_K];
#pragma unroll
  for (int k = 0; k < MARK_K; k++) { hi[k] = 0; lo[k] = 0; if (sl[k] >= 0) { hi[k] = cutoff[2 * sl[k]]; lo[k] = cutoff[2 * sl[k] + 1]; } }
#pragma unroll
  for (int k = 0; k < MARK_K; k++) {
    if (c0 + k > nch) break;
    const int f = (hi[k] > 0 && b[k] >= hi[k]) || (lo[k] > 0 && b[k] <= lo[k]);
    if (f) done[(c0 + k) * 64 + lane] = 1;
    select_store((c0 + k) * 64 + lane, nch, f, smask, scnt);
  }
}
// (every marking launch covers chunk nch as well: its count, 0, makes the scan's last element the total)
void launch_topup_keys(const PairRec *pairs, int64_t NP, const uint8_t *done, const uint32_t *b10, const int32_t *slot_of_prof, unsigned long long *smask, int32_t *scnt,
                       const int32_t *spos, unsigned long long *keys, int32_t *vals, hipStream_t st)
{
  hipLaunchKernelGGL(k_topup_keys, dim3(select_grid(NP)), dim3(256), 0, st, pairs, NP, done, b10, slot_of_prof, smask, scnt, spos, keys, vals);
}
void launch_topup_mark(const PairRec *pairs, int64_t NP, uint8_t *done, const uint32_t *b10, const int32_t *slot_of_prof, const uint32_t *cutoff,
                       unsigned long long *smask, int32_t *scnt, hipStream_t st)
{
  hipLaunchKernelGGL(k_topup_mark, dim3(select_grid(NP)), dim3(256), 0, st, pairs, NP, done, b10, slot_of_prof, cutoff, smask, scnt);
}

// ---- the count-only top-up round.  A pair of the round's list that has a multidomain region (mrcnt > 0: k_mr_count) is DEFERRED: the
// round wants a count, and that pair's verdict would take the ensemble stage.  It leaves the list's later stages (no envelope: ndom = 0,
// so the region list, the envelope kernels and k_score pass it by), it is unevaluated again in the search's own list (done = 0 at src:
// it stays on the upper bound's side), and its bit in dmask (zeroed by the caller) lets a second sub-round take exactly these pairs.
__global__ void __launch_bounds__(256) k_topup_defer(PairOut *__restrict__ pout, const int32_t *__restrict__ mrcnt, const int32_t *__restrict__ src, int64_t npairs,
                                                     uint8_t *__restrict__ done, unsigned long long *__restrict__ dmask, unsigned long long *__restrict__ n)
{
  const int64_t pi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pi >= npairs || mrcnt[pi] <= 0) return;
  pout[pi].ndom = 0;
  const int64_t i = src[pi];
  done[i] = 0;
  const unsigned long long bit = 1ull << (i & 63);
  atomicAdd(&n[(atomicOr(&dmask[i >> 6], bit) & bit) ? 1 : 0], 1ull);      // n[0]: deferred for the first time, n[1]: again
}
// the deferred pairs as a selection of the search's list (smask / scnt as k_lazy_mark leaves them, chunk nch included), marked evaluated
__global__ void __launch_bounds__(256) k_topup_deferred_select(const unsigned long long *__restrict__ dmask, int64_t nch, unsigned long long *__restrict__ smask,
                                                               int32_t *__restrict__ scnt, uint8_t *__restrict__ done)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > nch) return;
  unsigned long long m = c < nch ? dmask[c] : 0ull;
  smask[c] = m; scnt[c] = (int32_t)__popcll(m);
  while (m) { const int b = __ffsll((long long)m) - 1; done[c * 64 + b] = 1; m &= m - 1; }
}
// the deferred pairs of the listed profiles: cnt[slot] (zeroed) = bits of dmask in the profile's segment (segments start at whole chunks)
__global__ void __launch_bounds__(256) k_topup_count_mask(const unsigned long long *__restrict__ dmask, const int64_t *__restrict__ seg_start, const int32_t *__restrict__ total,
                                                          const int32_t *__restrict__ prof_of_slot, unsigned long long *__restrict__ cnt)
{
  const int sl = blockIdx.y, p = prof_of_slot[sl];
  const int64_t c0 = seg_start[p] >> 6, n = ((int64_t)total[p] + 63) >> 6;
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) c += (unsigned long long)__popcll(dmask[c0 + i]);
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt[sl], c);
}
void launch_topup_count_mask(const unsigned long long *dmask, const int64_t *seg_start, const int32_t *total, const int32_t *prof_of_slot, int nslots, unsigned long long *cnt, hipStream_t st)
{
  if (nslots > 0) hipLaunchKernelGGL(k_topup_count_mask, dim3(64, (unsigned)nslots), dim3(256), 0, st, dmask, seg_start, total, prof_of_slot, cnt);
}
void launch_topup_defer(PairOut *pout, const int32_t *mrcnt, const int32_t *src, int64_t npairs, uint8_t *done, unsigned long long *dmask, unsigned long long *n, hipStream_t st)
{
  if (npairs > 0) hipLaunchKernelGGL(k_topup_defer, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st, pout, mrcnt, src, npairs, done, dmask, n);
}
void launch_topup_deferred_select(const unsigned long long *dmask, int64_t NP, unsigned long long *smask, int32_t *scnt, uint8_t *done, hipStream_t st)
{
  const int64_t nch = (NP + 63) >> 6;
  hipLaunchKernelGGL(k_topup_deferred_select, dim3((unsigned)((nch + 1 + 255) / 256)), dim3(256), 0, st, dmask, nch, smask, scnt, done);
}

}  // namespace itsx
