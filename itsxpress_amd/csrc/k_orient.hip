// k_orient.hip -- f4, the parts of read orientation beside k_orient (k_cluster.hip): reads too long for its LDS word set, and the
// replacement of a read set by its oriented reads on the device (itsx_orient_apply).
#include <algorithm>
#include "engine.h"
#include "k_api.h"
#include "k_scan.h"
#include "iupac.h"

namespace itsx {

// ------------------------------------------------------------------ reads of more than 12 011 bases
// k_orient's procedure -- the distinct unambiguous, unmasked 12-mers of the read, each of them and its reverse complement looked up in
// the database bitmap, count_fwd / count_rev, the 4x rule -- for reads whose distinct words (up to 65 524) do not fit its 16 384-slot LDS
// set, nor anything a CU's LDS holds.  The set is a table of OL_TAB slots per BLOCK in global memory (512 KB; the 64 tables of a launch
// add up to the eight L2s' capacity -- how much of them stays resident beside the bitmap and the reads has not been measured), reached
// with atomics only, so no stale line of it is ever read from a CU's vector cache.  A block takes
// one long read at a time from the work list; it leaves its table empty by walking the read's words a second time and removing each
// first occurrence (a bit per position in LDS remembers them) -- 512 KB are never cleared for a read that filled a tenth of them.
constexpr int OL_TAB = 131072;
constexpr int OL_BLOCKS = 64;
__device__ __forceinline__ uint32_t ol_rc24(uint32_t k)      // (rc24 of k_cluster.hip)
{
  uint32_t r = __brev(~k & 0xffffffu) >> 8;
  return ((r >> 1) & 0x555555u) | ((r & 0x555555u) << 1);
}
__device__ __forceinline__ uint32_t ol_word(const uint32_t *w, int nw, int i)
{
  const int wi = i >> 4, sh = (i & 15) * 2;
  const unsigned long long lo = w[wi], hi = wi + 1 < nw ? w[wi + 1] : 0u;
  return (uint32_t)(((hi << 32) | lo) >> sh) & 0xffffffu;
}
__global__ __launch_bounds__(256) void k_orient_long(ReadsDev rd, const int32_t *__restrict__ list, int nl, const uint32_t *__restrict__ dbbits,
                                                     const uint32_t *__restrict__ dmask, uint32_t *__restrict__ tabs, int8_t *__restrict__ strand,
                                                     int32_t *__restrict__ cfwd, int32_t *__restrict__ crev)
{
  __shared__ uint32_t bad[2048];                             // 65 536 positions
  __shared__ uint32_t first[2048];                           // positions whose word entered the table
  __shared__ int cf, cr;
  const int tid = threadIdx.x;
  uint32_t *tab = tabs + (size_t)blockIdx.x * OL_TAB;
  for (int q = blockIdx.x; q < nl; q += gridDim.x) {
    const int64_t r = list[q];
    const int L = rd.len[r];
    const uint32_t *w = rd.words + rd.woff[r];
    const int nw = (int)(rd.woff[r + 1] - rd.woff[r]);
    const int64_t eo = rd.excoff[r];
    const int nexc = (int)(rd.excoff[r + 1] - eo);
    __syncthreads();
    for (int i = tid; i < 2048; i += 256) { bad[i] = 0u; first[i] = 0u; }
    if (tid == 0) { cf = 0; cr = 0; }
    __syncthreads();
    for (int e = tid; e < nexc; e += 256) {
      const int pos = (int)(rd.exc[eo + e] >> 4);
      for (int d = 0; d < 12; d++) { const int p = pos - d; if (p >= 0) atomicOr(&bad[p >> 5], 1u << (p & 31)); }
    }
    if (dmask) {
      const uint32_t *dm = dmask + rd.woff[r];
      for (int mw = tid; mw < ((L + 31) >> 5); mw += 256) {
        uint32_t x = dm[mw];
        while (x) {
          const int pos = mw * 32 + __ffs(x) - 1; x &= x - 1;
          for (int d = 0; d < 12; d++) { const int p = pos - d; if (p >= 0) atomicOr(&bad[p >> 5], 1u << (p & 31)); }
        }
      }
    }
    __syncthreads();
    int f = 0, v = 0;
    for (int i = tid; i + 12 <= L; i += 256) {
      if ((bad[i >> 5] >> (i & 31)) & 1u) continue;
      const uint32_t k = ol_word(w, nw, i);
      for (uint32_t slot = (k * 2654435761u) >> 15;; slot = (slot + 1) & (OL_TAB - 1)) {      // (at most 65 524 of 131 072 slots fill: the walk ends)
        const uint32_t old = atomicCAS(&tab[slot], 0u, k + 1u);
        if (old == 0u) {                                     // first occurrence of this word in the read
          const uint32_t kr = ol_rc24(k);
          f += (dbbits[k >> 5] >> (k & 31)) & 1u;
          v += (dbbits[kr >> 5] >> (kr & 31)) & 1u;
          atomicOr(&first[i >> 5], 1u << (i & 31));
          break;
        }
        if (old == k + 1u) break;
      }
    }
    if (f) atomicAdd(&cf, f);
    if (v) atomicAdd(&cr, v);
    __syncthreads();
    // the table empty again: every word is taken out by the position that put it in (it is there exactly once, and nobody else removes it)
    for (int i = tid; i + 12 <= L; i += 256) {
      if (!((first[i >> 5] >> (i & 31)) & 1u)) continue;
      const uint32_t k = ol_word(w, nw, i);
      uint32_t slot = (k * 2654435761u) >> 15;
      for (int step = 0; step < OL_TAB; step++, slot = (slot + 1) & (OL_TAB - 1))
        if (atomicCAS(&tab[slot], k + 1u, 0u) == k + 1u) break;
    }
    if (tid == 0) {
      const int a = cf, b = cr;
      cfwd[r] = a; crev[r] = b;
      strand[r] = (int8_t)((a >= 1 && a >= 4 * b) ? 1 : (b >= 1 && b >= 4 * a) ? -1 : 0);
    }
  }
}
int64_t orient_long_table_words(int64_t n_long) { return n_long > 0 ? std::min<int64_t>(n_long, OL_BLOCKS) * OL_TAB : 0; }
void launch_orient_long(const ReadsDev &rd, const int32_t *list, int64_t n_long, const uint32_t *dbbits, const uint32_t *dmask, uint32_t *tabs,
                        int8_t *strand, int32_t *cfwd, int32_t *crev, hipStream_t st)
{
  if (n_long <= 0) return;
  hipLaunchKernelGGL(k_orient_long, dim3((unsigned)std::min<int64_t>(n_long, OL_BLOCKS)), dim3(256), 0, st, rd, list, (int)n_long, dbbits, dmask, tabs,
                     strand, cfwd, crev);
}

// ------------------------------------------------------------------ the oriented reads as a read set (itsx_orient_apply)
// Plan: a two-level exclusive scan over the reads of (kept ? 1 : 0, kept ? its words : 0, kept ? its exceptions : 0), shaped like the merge
// compaction (k_merge.hip): every block of OA_TILE reads sums its tile (k_oa_plan<false>), one block scans the tiles' sums (k_oa_sums),
// every block scans its tile again and writes what the kept reads need (k_oa_plan<true>).  64-bit sums throughout.
constexpr int OA_BLOCK = 256;
constexpr int OA_ITEMS = 8;
constexpr int OA_TILE = OA_BLOCK * OA_ITEMS;    // reads per block; thread t owns OA_ITEMS consecutive reads

template <bool SCATTER> __global__ __launch_bounds__(OA_BLOCK) void k_oa_plan(OrientApplyArgs a)
{
  const int64_t base = (int64_t)blockIdx.x * OA_TILE + (int64_t)threadIdx.x * OA_ITEMS;
  int32_t nw[OA_ITEMS], ne[OA_ITEMS];
  int64_t v[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < OA_ITEMS; i++) {
    const int64_t r = base + i;
    const bool ok = r < a.rd.n && a.strand[r] != 0;
    nw[i] = ok ? (int32_t)(a.rd.woff[r + 1] - a.rd.woff[r]) : -1;
    ne[i] = ok ? (int32_t)(a.rd.excoff[r + 1] - a.rd.excoff[r]) : 0;
    if (ok) { v[0]++; v[1] += nw[i]; v[2] += ne[i]; }
  }
  int64_t ex[3], tot[3];
  block_scan64<3, OA_BLOCK>(v, ex, tot);
  const int64_t nb = gridDim.x;
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk[blockIdx.x] = tot[0]; a.blk[nb + blockIdx.x] = tot[1]; a.blk[2 * nb + blockIdx.x] = tot[2]; }
    return;
  }
  int64_t j = a.blk[blockIdx.x] + ex[0], wo = a.blk[nb + blockIdx.x] + ex[1], eo = a.blk[2 * nb + blockIdx.x] + ex[2];
  int32_t s = -1; unsigned long long run = 0;                // the sample of the reads counted in `run`
#pragma unroll
  for (int i = 0; i < OA_ITEMS; i++) {
    const int64_t r = base + i;
    if (r >= a.rd.n) break;
    if (nw[i] < 0) continue;
    a.src[j] = (int32_t)r;
    a.woff[j] = wo; a.excoff[j] = eo; a.len[j] = a.rd.len[r];
    if (a.sample) {
      const int32_t sr = a.sample[r];
      if (sr != s) {
        if (run) atomicAdd(reinterpret_cast<unsigned long long *>(a.sample_count + s), run);
        run = 0; s = sr;
      }
      a.osample[j] = sr;
      run++;
    }
    j++; wo += nw[i]; eo += ne[i];
  }
  if (run) atomicAdd(reinterpret_cast<unsigned long long *>(a.sample_count + s), run);
}

// the tiles' sums -> their exclusive prefixes, in place; total[0..2] = kept reads, their words, their exceptions; the offsets' last entries
__global__ __launch_bounds__(OA_BLOCK) void k_oa_sums(int64_t *__restrict__ blk, int64_t nb, int64_t *__restrict__ total, int64_t *__restrict__ woff,
                                                      int64_t *__restrict__ excoff)
{
  int64_t carry[3] = {0, 0, 0};                              // the sums of the chunks before this one
  for (int64_t b0 = 0; b0 < nb; b0 += OA_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    int64_t v[3], ex[3], tot[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = b < nb ? blk[k * nb + b] : 0;
    block_scan64<3, OA_BLOCK>(v, ex, tot);
#pragma unroll
    for (int k = 0; k < 3; k++) { if (b < nb) blk[k * nb + b] = carry[k] + ex[k]; carry[k] += tot[k]; }
  }
  if (threadIdx.x == 0) { total[0] = carry[0]; total[1] = carry[1]; total[2] = carry[2]; woff[carry[0]] = carry[1]; excoff[carry[0]] = carry[2]; }
}

// The words: a block takes OA_RB consecutive OUTPUT reads, whose words are one contiguous stretch, and thread t takes word t, t + 256, ...
// of that stretch whichever read it belongs to (k_pack_words' layout: every lane busy on reads of a few hundred bases).  A forward read's
// word is its input word.  Word k of a reverse read holds the complements of input bases L-1-16k-i, i = 0..15: the 16 input bases from
// L-16-16k on (two neighbouring words, shifted by the read's tail offset; bases before the read's first are zeros), their 2-bit fields in
// reverse order (__brev and a swap inside every pair), complemented by NOT, and the fields past the read's last base cleared.
constexpr int OA_RB = 64;
__global__ __launch_bounds__(256) void k_oa_words(OrientApplyArgs a, int64_t m)
{
  __shared__ int32_t s_wrel[OA_RB + 1], s_src[OA_RB], s_len[OA_RB];     // s_len < 0: a reverse read
  const int tid = (int)threadIdx.x;
  const int64_t ngroups = (m + OA_RB - 1) / OA_RB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t firstj = g * OA_RB;
    const int nr = (int)(m - firstj < OA_RB ? m - firstj : OA_RB);
    const int64_t w0 = a.woff[firstj];
    __syncthreads();
    if (tid <= nr) s_wrel[tid] = (int32_t)(a.woff[firstj + tid] - w0);
    if (tid < nr) {
      const int32_t r = a.src[firstj + tid];
      s_src[tid] = r;
      s_len[tid] = a.strand[r] < 0 ? -a.rd.len[r] : a.rd.len[r];
    }
    __syncthreads();
    const int Wb = s_wrel[nr];
    for (int w = tid; w < Wb; w += 256) {
      int j = 0;                                             // the read of word w: s_wrel[j] <= w < s_wrel[j + 1]
#pragma unroll
      for (int step = OA_RB / 2; step >= 1; step >>= 1) if (j + step < nr && s_wrel[j + step] <= w) j += step;
      const int k = w - s_wrel[j];
      const uint32_t *in = a.rd.words + a.rd.woff[s_src[j]];
      uint32_t out;
      if (s_len[j] > 0) out = in[k];
      else {
        const int L = -s_len[j], nw = (L + 15) >> 4;
        const int p0 = L - 16 - 16 * k;                      // the first input base of the window
        uint32_t x;
        if (p0 >= 0) {
          const int wi = p0 >> 4, sh = (p0 & 15) * 2;
          const unsigned long long lo = in[wi], hi = wi + 1 < nw ? in[wi + 1] : 0u;
          x = (uint32_t)(((hi << 32) | lo) >> sh);
        } else x = in[0] << (2 * -p0);                      // (the read's last word: -p0 = 16 - its bases, 1..15)
        x = __brev(x);
        x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
        out = ~x;
        if (p0 < 0) out &= (1u << (2 * (16 + p0))) - 1u;
      }
      a.words[w0 + w] = out;
    }
  }
}
// The exception lists (rare: one thread per kept read, most of which leave at once): a forward read's as it is; a reverse read's walked
// from its end, position p -> L-1-p and every code replaced by its complement's, so that it ascends again -- and the 2-bit field of each
// mirrored position cleared: an exception is 0 in the 2-bit plane, and k_oa_words' NOT made it 3.
__global__ __launch_bounds__(256) void k_oa_exc(OrientApplyArgs a, int64_t m)
{
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const int32_t r = a.src[j];
  const int64_t ei = a.rd.excoff[r];
  const int ne = (int)(a.rd.excoff[r + 1] - ei);
  if (ne == 0) return;
  uint32_t *out = a.exc + a.excoff[j];
  if (a.strand[r] > 0) { for (int t = 0; t < ne; t++) out[t] = a.rd.exc[ei + t]; return; }
  const int L = a.rd.len[r];
  uint32_t *w = a.words + a.woff[j];
  for (int t = 0; t < ne; t++) {
    const uint32_t e = a.rd.exc[ei + ne - 1 - t];
    const int p = L - 1 - (int)(e >> 4);
    out[t] = ((uint32_t)p << 4) | iupac_comp_code(e & 15u);
    w[p >> 4] &= ~(3u << ((p & 15) * 2));
  }
}

int64_t orient_apply_blocks(int64_t n) { return (n + OA_TILE - 1) / OA_TILE; }
int orient_apply_tile() { return OA_TILE; }
void launch_orient_apply_plan(const OrientApplyArgs &a, hipStream_t st)
{
  if (a.rd.n <= 0) return;
  const int64_t nb = orient_apply_blocks(a.rd.n);
  hipLaunchKernelGGL(k_oa_plan<false>, dim3((unsigned)nb), dim3(OA_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_oa_sums, dim3(1), dim3(OA_BLOCK), 0, st, a.blk, nb, a.total, a.woff, a.excoff);
  hipLaunchKernelGGL(k_oa_plan<true>, dim3((unsigned)nb), dim3(OA_BLOCK), 0, st, a);
}
void launch_orient_apply_scatter(const OrientApplyArgs &a, int64_t m, hipStream_t st)
{
  if (m <= 0) return;
  hipLaunchKernelGGL(k_oa_words, dim3((unsigned)std::min<int64_t>((m + OA_RB - 1) / OA_RB, 1 << 20)), dim3(256), 0, st, a, m);
  hipLaunchKernelGGL(k_oa_exc, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a, m);
}

}  // namespace itsx
