// k_cigar.hip -- the alignment behind every H row of a clustering's uc.txt (itsx_align_clusters; opt-in, after the clustering).
//
// k_cluster.hip's align_pair keeps no path: its cell packs (score, matches, counted columns) into one int64 and the identity comes
// out of the sweep alone.  Here the SAME sweep (one wave per pair, lane l owns S consecutive rows, the columns advance as an
// anti-diagonal wavefront, 64 S rows per pass; the cell arithmetic is k_cl_cell.h's, shared) runs once more for the accepted
// (member, centroid) pairs only and leaves four direction bits per cell behind:
//   bits 0-1  where H came from: 0 the diagonal, 1 E (a run that consumes centroid symbols), 2 F (a run that consumes query symbols).
//             The diagonal is taken when it reproduces the cell's packed value, else E, else F;
//   bit  2    E extends (E of the cell to the left + extension reproduces E); 0: E opens from H of the cell to the left;
//   bit  3    F extends, likewise from the cell above.
// A gap extends in preference to closing.  The bits of a lane's S cells of one step are one word (S = 5, 8: 32 bits; S = 10: 64),
// stored at [pass][step][lane]: the 64 lanes of a step write 256 (512) consecutive bytes, one whole vector store per wave and step.
// Cell (i, j) is therefore found at pass i / 64 S, lane (i % 64 S) / S, step j + lane, nibble i % S.
//
// The traceback is one thread per pair from (Lq, Lt) to (0, 0): it walks once to learn the length of the run-length text and once
// more to write it, back to front, into one text plane (k_trim.hip's shape: lengths, offsets, fill).  M: a column with a symbol of
// each read; I: a centroid symbol opposite a gap in the query; D: a query symbol opposite a gap in the centroid; a run of one
// prints its letter alone.  A member that equals its centroid symbol for symbol (k_cg_equal) is "=" and is never aligned.
#include <algorithm>
#include "engine.h"
#include "k_api.h"
#include "k_cl_cell.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "this engine ships gfx950 code only"
#endif

namespace itsx {

template <int S> struct DirWord { typedef uint32_t T; };
template <> struct DirWord<10> { typedef unsigned long long T; };

// the member on its strand equals the centroid: same length, the same 2-bit symbols and the same IUPAC codes at the same places.
// The exceptions of a read are in rising position, so the k-th of the member meets the k-th (minus strand: the k-th from the
// end, complemented) of the centroid; their places hold symbol 0 in the 2-bit plane, which on the minus strand is compared as 3
// against 0 -- exactly one mismatch per exception, and no other.  One wave per pair.
__global__ __launch_bounds__(64) void k_cg_equal(CigarArgs a, int32_t n, int32_t *eq)
{
  const int lane = threadIdx.x;
  for (int p = blockIdx.x; p < n; p += gridDim.x) {
    const int64_t rq = a.q_read[p], rt = a.t_read[p];
    const int s = a.strand[p] < 0 ? 1 : 0;
    const int Lq = a.rd.len[rq], Lt = a.rd.len[rt];
    const int64_t eoq = a.rd.excoff[rq], eot = a.rd.excoff[rt];
    const int neq = (int)(a.rd.excoff[rq + 1] - eoq), net = (int)(a.rd.excoff[rt + 1] - eot);
    bool same = Lq == Lt && neq == net;
    if (same) {
      const uint32_t *wq = a.rd.words + a.rd.woff[rq], *wt = a.rd.words + a.rd.woff[rt];
      int bad = 0;
      for (int e = lane; e < neq; e += 64) {
        const uint32_t xq = a.rd.exc[eoq + e], xt = a.rd.exc[eot + (s ? neq - 1 - e : e)];
        const int pq = (int)(xq >> 4), pt = (int)(xt >> 4);
        const uint32_t mq = s ? revmask4(mask4(xq & 15u)) : mask4(xq & 15u);
        if ((s ? Lq - 1 - pq : pq) != pt || mq != mask4(xt & 15u)) bad = 1 << 20;
      }
      int diff = 0;
      for (int x = lane; x < Lq; x += 64) {
        const int o = s ? Lq - 1 - x : x;
        const uint32_t cq = (wq[o >> 4] >> ((o & 15) * 2)) & 3u, ct = (wt[x >> 4] >> ((x & 15) * 2)) & 3u;
        diff += (s ? 3u - cq : cq) != ct ? 1 : 0;
      }
      diff += bad;
      for (int off = 32; off; off >>= 1) diff += __shfl_xor(diff, off);
      same = diff == (s ? neq : 0);
    }
    if (lane == 0) eq[p] = same ? 1 : 0;
  }
}

// align_pair (k_cluster.hip) with the direction bits; pair p of the batch [p0, p0 + np)
template <int S> __global__ __launch_bounds__(64) void k_cg_forward(CigarArgs a, int32_t p0, int32_t np)
{
  typedef typename DirWord<S>::T W;
  extern __shared__ uint8_t tmask[];
  const int lane = threadIdx.x;
  for (int w = blockIdx.x; w < np; w += gridDim.x) {
    const int p = p0 + w;
    const int64_t rq = a.q_read[p], rt = a.t_read[p];
    const int s = a.strand[p] < 0 ? 1 : 0;
    const int Lq = a.rd.len[rq], Lt = a.rd.len[rt];
    const uint32_t *wq = a.rd.words + a.rd.woff[rq];
    const uint32_t *wt = a.rd.words + a.rd.woff[rt];
    const int64_t eoq = a.rd.excoff[rq], eot = a.rd.excoff[rt];
    const int nexq = (int)(a.rd.excoff[rq + 1] - eoq), next_ = (int)(a.rd.excoff[rt + 1] - eot);
    i64 *scr = a.scratch + a.scr_off[p];
    W *dir = reinterpret_cast<W *>(a.dir + a.dir_off[p]);
    const int RB = 64 * S;
    const int npass = (Lq + 1 + RB - 1) / RB;
    const int nsteps = Lt + 1 + 63;

    // the target's IUPAC sets go to LDS once; lane l then reads the symbol of its own column every step
    __syncthreads();
    for (int o = lane; o < Lt; o += 64) tmask[o] = (uint8_t)(1u << ((wt[o >> 4] >> ((o & 15) * 2)) & 3u));
    __syncthreads();
    for (int e = lane; e < next_; e += 64) { const uint32_t ex = a.rd.exc[eot + e]; tmask[ex >> 4] = (uint8_t)mask4(ex & 15u); }
    __syncthreads();

    for (int pass = 0; pass < npass; pass++) {
      const int i0 = pass * RB + lane * S;
      uint32_t qm[S]; bool qu[S]; i64 goE[S], geE[S];
#pragma unroll
      for (int r = 0; r < S; r++) {
        const int i = i0 + r;
        uint32_t m = 0;
        if (i >= 1 && i <= Lq) {
          const int x = i - 1, o = s ? Lq - 1 - x : x;
          const uint32_t c2 = (wq[o >> 4] >> ((o & 15) * 2)) & 3u;
          m = 1u << (s ? 3u - c2 : c2);
        }
        qm[r] = m; goE[r] = (i == 0 || i == Lq) ? GOT : GOI; geE[r] = (i == 0 || i == Lq) ? GET : GEI;
      }
      for (int e = 0; e < nexq; e++) {
        const uint32_t ex = a.rd.exc[eoq + e];
        const int pos = (int)(ex >> 4);
        const int i = (s ? Lq - 1 - pos : pos) + 1;
        const uint32_t m = s ? revmask4(mask4(ex & 15u)) : mask4(ex & 15u);
#pragma unroll
        for (int r = 0; r < S; r++) if (i == i0 + r) qm[r] = m;
      }
#pragma unroll
      for (int r = 0; r < S; r++) qu[r] = unamb4(qm[r]);

      i64 Hl[S], El[S];
#pragma unroll
      for (int r = 0; r < S; r++) { Hl[r] = NEGV; El[r] = NEGV; }
      // cell (0,0) is 0: its "diagonal" enters as +1 and meets the -1 of a column without symbol
      i64 diag_carry = (pass == 0 && lane == 0) ? 1 : NEGV, pubH = NEGV, pubF = NEGV;
      W *dpass = dir + (size_t)pass * (size_t)nsteps * 64 + lane;
      const bool rows_live = i0 <= Lq;                       // a lane whose rows all lie past the query writes nothing (nobody walks there)
      for (int t = 0; t < nsteps; t++) {
        i64 upH = shfl_up64(pubH), upF = shfl_up64(pubF);
        const int j = t - lane;
        if (lane == 0) {
          if (pass > 0 && j <= Lt) {
            upH = __hip_atomic_load(&scr[2 * j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            upF = __hip_atomic_load(&scr[2 * j + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          else { upH = NEGV; upF = NEGV; }
        }
        if (j >= 0 && j <= Lt) {
          const uint32_t tm = j >= 1 ? (uint32_t)tmask[j - 1] : 0u;
          const bool tF = (j == 0 || j == Lt);
          const i64 goF = tF ? GOT : GOI, geF = tF ? GET : GEI;
          const bool tu = unamb4(tm);
          i64 aboveH = upH, aboveF = upF, dg = diag_carry;
          W word = 0;
#pragma unroll
          for (int r = 0; r < S; r++) {
            const i64 eo = Hl[r] + goE[r], ee = El[r] + geE[r];
            const i64 fo = aboveH + goF, fe = aboveF + geF;
            const i64 E = max64(eo, ee);
            const i64 F = max64(fo, fe);
            const bool compat = (qm[r] & tm) != 0u;
            const bool bu = qu[r] && tu;
            const uint32_t dlo = compat ? 0x000FFFFFu : 0xFFFFFFFFu;
            const int32_t dhiA = compat ? 0 : -1, dhiU = compat ? 512 : -1025;
            const i64 D = (i64)(((u64)(uint32_t)(bu ? dhiU : dhiA) << 32) | (u64)dlo);
            const i64 dv = dg + D;
            const i64 Hn = max64(max64(dv, E), F);
            const uint32_t bits = (dv == Hn ? 0u : E == Hn ? 1u : 2u) | (ee >= eo ? 4u : 0u) | (fe >= fo ? 8u : 0u);
            word |= (W)bits << (4 * r);
            dg = Hl[r];
            Hl[r] = Hn; El[r] = E;
            aboveH = Hn; aboveF = F;
          }
          if (rows_live) dpass[(size_t)t * 64] = word;
          pubH = aboveH; pubF = aboveF;
          diag_carry = upH;
          if (lane == 63 && pass + 1 < npass) {
            __hip_atomic_store(&scr[2 * j], aboveH, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&scr[2 * j + 1], aboveF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
      if (pass + 1 < npass) __threadfence();
      else {                                               // every row now holds its value in column Lt
#pragma unroll
        for (int r = 0; r < S; r++) if (i0 + r == Lq) { a.res[p] = Hl[r]; a.pid[p] = identity_of(Hl[r]); }
      }
    }
  }
}

__device__ __forceinline__ int cg_run_chars(int n) { int c = 1; if (n > 1) for (int v = n; v; v /= 10) c++; return c; }

// one thread per pair; fill = 0: tlen[p] = characters of the text (-1: the bits do not lead from (Lq, Lt) to (0, 0));
// fill = 1: the text at text[toff[p] .. toff[p + 1]), written from its end
template <int S> __global__ __launch_bounds__(64) void k_cg_traceback(CigarArgs a, int32_t p0, int32_t np, int fill)
{
  typedef typename DirWord<S>::T W;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= np) return;
  const int p = p0 + w;
  const int Lq = a.rd.len[a.q_read[p]], Lt = a.rd.len[a.t_read[p]];
  const W *dir = reinterpret_cast<const W *>(a.dir + a.dir_off[p]);
  const int RB = 64 * S;
  const size_t nsteps = (size_t)Lt + 64;
  if (fill && a.tlen[w] < 0) return;
  char *out = fill ? a.text + a.toff[w + 1] : nullptr;      // one past the pair's last character
  int i = Lq, j = Lt, state = 0, run = 0, nchars = 0;
  char op = 0;
  bool ok = true;
  auto flush = [&]() {
    if (!run) return;
    if (fill) {
      *--out = op;
      if (run > 1) for (int v = run; v; v /= 10) *--out = (char)('0' + v % 10);
    } else nchars += cg_run_chars(run);
  };
  auto emit = [&](char c) { if (c != op) { flush(); op = c; run = 0; } run++; };
  // (a step that only changes state is followed by one that consumes a symbol or fails: at most 2 (Lq + Lt) steps)
  while ((i > 0 || j > 0) && ok) {
    const int pass = i / RB, rem = i - pass * RB, lane = rem / S, r = rem - lane * S;
    const W word = dir[((size_t)pass * nsteps + (size_t)(j + lane)) * 64 + lane];
    const uint32_t bits = (uint32_t)(word >> (4 * r)) & 15u;
    if (state == 0) {
      const uint32_t src = bits & 3u;
      if (src == 0u) { if (i == 0 || j == 0) ok = false; else { emit('M'); i--; j--; } }
      else if (src == 1u) state = 1;
      else if (src == 2u) state = 2;
      else ok = false;
    } else if (state == 1) {
      if (j == 0) ok = false;
      else { emit('I'); j--; if (!(bits & 4u)) state = 0; }
    } else {
      if (i == 0) ok = false;
      else { emit('D'); i--; if (!(bits & 8u)) state = 0; }
    }
  }
  if (state != 0) ok = false;
  flush();
  if (!fill) a.tlen[w] = ok ? nchars : -1;
}

static size_t cg_lds(int lmax) { return ((size_t)lmax + 63) & ~(size_t)63; }

void launch_cg_equal(const CigarArgs &a, int32_t n, int32_t *eq, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_cg_equal, dim3(std::min(n, 65536)), dim3(64), 0, st, a, n, eq);
}
void launch_cg_forward(const CigarArgs &a, int32_t p0, int32_t np, int rows_per_lane, int lmax, hipStream_t st)
{
  if (np <= 0) return;
  const int grid = std::min(np, 16384);
  if (rows_per_lane <= 5) hipLaunchKernelGGL(k_cg_forward<5>, dim3(grid), dim3(64), cg_lds(lmax), st, a, p0, np);
  else if (rows_per_lane <= 8) hipLaunchKernelGGL(k_cg_forward<8>, dim3(grid), dim3(64), cg_lds(lmax), st, a, p0, np);
  else hipLaunchKernelGGL(k_cg_forward<10>, dim3(grid), dim3(64), cg_lds(lmax), st, a, p0, np);
}
void launch_cg_traceback(const CigarArgs &a, int32_t p0, int32_t np, int rows_per_lane, int fill, hipStream_t st)
{
  if (np <= 0) return;
  const int grid = (np + 63) / 64;
  if (rows_per_lane <= 5) hipLaunchKernelGGL(k_cg_traceback<5>, dim3(grid), dim3(64), 0, st, a, p0, np, fill);
  else if (rows_per_lane <= 8) hipLaunchKernelGGL(k_cg_traceback<8>, dim3(grid), dim3(64), 0, st, a, p0, np, fill);
  else hipLaunchKernelGGL(k_cg_traceback<10>, dim3(grid), dim3(64), 0, st, a, p0, np, fill);
}
// bytes of one pair's direction bits and of its border rows between passes (0: one pass), as k_cg_forward lays them out
void cg_pair_bytes(int Lq, int Lt, int rows_per_lane, size_t *dir_bytes, size_t *scr_bytes)
{
  const int S = rows_per_lane <= 5 ? 5 : rows_per_lane <= 8 ? 8 : 10;
  const size_t npass = ((size_t)Lq + 1 + 64 * S - 1) / (64 * (size_t)S);
  *dir_bytes = npass * ((size_t)Lt + 64) * 64 * (S == 10 ? 8 : 4);
  *scr_bytes = npass > 1 ? ((size_t)Lt + 1) * 2 * sizeof(long long) : 0;
}

}  // namespace itsx
