// k_trim.hip -- SURVEY section 8f row f1 for a batch: the trimmed FASTQ text of every sample, made on the device from the records the
// context keeps (itsx_keep_records): Dedup.create_trimmed_seqs (itsxpress/SeqSample.py:886-949) as trim_host.cpp states it.
//
// Read i is written iff start >= 0 && stop >= 0 && start < stop, as title \n [primer] bases[start:stop] [primer] \n+\n [17 x ~] quals[start:stop]
// [17 x ~] \n, the slice clamped to the read as Python clamps it.  Three steps:
//   plan   one output length per read (0: not written), then a two-level exclusive scan in 64-bit offsets (k_scan.h, as k_merge.hip's
//          compaction): TrimRec[r] says where read r's record starts in the batch's text and where its three sources are.  Samples are
//          contiguous in the read set, so a sample's file is one byte range of that text (k_trim_bounds reads the ranges off the scan).
//   copy   OUTPUT-stationary: a block owns 16 KiB of the text, a wave-instruction stores 256 contiguous aligned bytes (one dword per lane).
//          A lane finds the record of its dword by bisection between the records of the tile's first and last byte; where the four bytes
//          come from one source (title, bases, qualities) they are two aligned loads and a funnel shift -- the misalignment of source
//          against destination falls on the loads -- and at the seams (newlines, '+', primers, record ends) they are assembled byte by
//          byte.  Work follows output bytes, not records: a 65 535-base read is spread over the blocks like anything else.
//   pairs  the paired plan (itsx_keep_pair_records): Dedup.create_paired_trimmed_seqs (SeqSample.py:564-790) -- the ORIGINAL R1 / R2 records
//          of a pair sliced with the coordinates of the merged read its R1 identifier names.  One TrimRec per pair and side, the same scan
//          shape, and the copy kernel as it is, once per side.
//   unit   a unit of RAW FASTQ text (the streamed writers' device path, itsx_twriter_set_device): the line index from its newline bytes
//          (popcount per thread, two scans), trusted where the unit has 4 lines per record; the plan of itsx_twriter::work's two modes;
//          and the copy kernel with all three planes = that text and a quality source of its own per record (k_trim_copy<true, .>).
//          A unit that has a record of strand -1 (itsx_twriter_strands) takes k_trim_copy<true, true>, which reads such a record's
//          lines backwards and complements its bases; every other unit, and every batch, takes the kernel without that branch.
//   orient the records of the reads itsx_orient_apply keeps: reverse reads with IUPAC-complemented reversed bases and reversed qualities.
#include <algorithm>
#include "engine.h"
#include "k_api.h"
#include "k_scan.h"
#include "k_lines.h"

namespace itsx {

constexpr int TR_BLOCK = 256;
constexpr int TR_ITEMS = 4;
constexpr int TR_TILE = TR_BLOCK * TR_ITEMS;     // reads per block of the plan's scan; thread t owns TR_ITEMS consecutive reads
constexpr int TC_BLOCK = 256;
constexpr int TC_DWORDS = 16;                    // dwords per lane of a copy tile
constexpr int64_t TC_TILE = (int64_t)TC_BLOCK * TC_DWORDS * 4;   // bytes of the text per block

__device__ __forceinline__ void trim_plan_one(const TrimPlanArgs &a, int64_t r, int32_t &tl, int32_t &lo, int32_t &slen, bool &w)
{
  const int32_t s = a.start[r * a.stride], e = a.stop[r * a.stride];
  const int64_t L = a.off[r + 1] - a.off[r];
  w = s >= 0 && e >= 0 && s < e;
  tl = (int32_t)(a.toff[r + 1] - a.toff[r]);
  const int64_t l = s < L ? s : L, h = e < L ? e : L;          // Python's [s:e] for 0 <= s < e
  lo = (int32_t)l; slen = (int32_t)(h > l ? h - l : 0);
}

template <bool SCATTER> __global__ __launch_bounds__(TR_BLOCK) void k_trim_plan(TrimPlanArgs a)
{
  const int64_t base = (int64_t)blockIdx.x * TR_TILE + (int64_t)threadIdx.x * TR_ITEMS;
  const int64_t extra = a.ccs ? 34 : 0;
  int32_t tl[TR_ITEMS], lo[TR_ITEMS], sl[TR_ITEMS]; bool w[TR_ITEMS];
  int64_t v[3] = {0, 0, 0};                      // bytes of text, records, total_len as trim_host.cpp's emit counts it
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t r = base + i;
    w[i] = false; tl[i] = lo[i] = sl[i] = 0;
    if (r < a.n) trim_plan_one(a, r, tl[i], lo[i], sl[i], w[i]);
    if (w[i]) { v[0] += (int64_t)tl[i] + 5 + 2 * ((int64_t)sl[i] + extra); v[1]++; v[2] += (int64_t)sl[i] + extra; }
  }
  int64_t ex[3], tot[3];
  block_scan64<3, TR_BLOCK>(v, ex, tot);
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk[blockIdx.x * 3 + 0] = tot[0]; a.blk[blockIdx.x * 3 + 1] = tot[1]; a.blk[blockIdx.x * 3 + 2] = tot[2]; }
    return;
  }
  int64_t o = a.blk[blockIdx.x * 3 + 0] + ex[0], c = a.blk[blockIdx.x * 3 + 1] + ex[1], t = a.blk[blockIdx.x * 3 + 2] + ex[2];
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t r = base + i;
    if (r >= a.n) break;
    TrimRec q;
    q.out = o; q.src = a.off[r] + lo[i]; q.toff = a.toff[r]; q.tl = tl[i]; q.slen = sl[i];
    a.rec[r] = q; a.cnt[r] = c; a.tot[r] = t;
    if (w[i]) { o += (int64_t)tl[i] + 5 + 2 * ((int64_t)sl[i] + extra); c++; t += (int64_t)sl[i] + extra; }
  }
}

// the tiles' sums -> their exclusive prefixes, in place; entry n of rec / cnt / tot = the batch's totals
__device__ __forceinline__ void trim_scan_tiles(int64_t *__restrict__ blk, int64_t nb, int64_t (&carry)[3])
{
  carry[0] = carry[1] = carry[2] = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += TR_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    int64_t v[3], ex[3], tot[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = b < nb ? blk[b * 3 + k] : 0;
    block_scan64<3, TR_BLOCK>(v, ex, tot);
#pragma unroll
    for (int k = 0; k < 3; k++) { if (b < nb) blk[b * 3 + k] = carry[k] + ex[k]; carry[k] += tot[k]; }
  }
}
__global__ __launch_bounds__(TR_BLOCK) void k_trim_plan_sums(TrimPlanArgs a, int64_t nb)
{
  int64_t carry[3];
  trim_scan_tiles(a.blk, nb, carry);
  if (threadIdx.x == 0) {
    TrimRec q;
    q.out = carry[0]; q.src = 0; q.toff = 0; q.tl = 0; q.slen = 0;
    a.rec[a.n] = q; a.cnt[a.n] = carry[1]; a.tot[a.n] = carry[2];
  }
}

// bounds[k][s] for k = 0 (byte offset), 1 (records), 2 (total_len) at the first read of sample s, s = 0 .. S (first[S] = n)
__global__ void k_trim_bounds(const TrimRec *__restrict__ rec, const int64_t *__restrict__ cnt, const int64_t *__restrict__ tot, const int64_t *__restrict__ first,
                              int32_t S, int64_t *__restrict__ bounds)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > S) return;
  const int64_t r = first[s];
  bounds[s] = rec[r].out; bounds[(S + 1) + s] = cnt[r]; bounds[2 * (S + 1) + s] = tot[r];
}

int64_t trim_plan_blocks(int64_t n) { return (n + TR_TILE - 1) / TR_TILE; }

void launch_trim_plan(const TrimPlanArgs &a, const int64_t *first, int32_t S, int64_t *bounds, hipStream_t st)
{
  const int64_t nb = trim_plan_blocks(a.n);
  if (nb > 0) hipLaunchKernelGGL(k_trim_plan<false>, dim3((unsigned)nb), dim3(TR_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_plan_sums, dim3(1), dim3(TR_BLOCK), 0, st, a, nb);
  if (nb > 0) hipLaunchKernelGGL(k_trim_plan<true>, dim3((unsigned)nb), dim3(TR_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_bounds, dim3((unsigned)((S + 1 + 255) / 256)), dim3(256), 0, st, a.rec, a.cnt, a.tot, first, S, bounds);
}

// ---- the paired plan ------------------------------------------------------------------------------------------------------------
// Python's seq[a:b] of a sequence of n (open: no upper bound), as trim_host.cpp's py_slice states it: a negative bound gets n added and
// is clamped at 0, a bound past the end is clamped at n, and the slice is empty when it ends before it starts
__device__ __forceinline__ void trim_py_slice(int64_t n, int64_t a, int64_t b, bool open, int32_t &lo, int32_t &slen)
{
  if (a < 0) { a += n; if (a < 0) a = 0; } else if (a > n) a = n;
  if (open) b = n;
  else if (b < 0) { b += n; if (b < 0) b = 0; } else if (b > n) b = n;
  lo = (int32_t)a; slen = (int32_t)(b > a ? b - a : 0);
}
// pair p: whether it is written, and per side the title's bytes, the slice's first base and its length
__device__ __forceinline__ void trim_pair_one(const TrimPairPlanArgs &a, int64_t p, int32_t (&tl)[2], int32_t (&lo)[2], int32_t (&sl)[2], bool &w)
{
  const int64_t k = a.pair_read[p];
  tl[0] = (int32_t)(a.toff1[p + 1] - a.toff1[p]); tl[1] = (int32_t)(a.toff2[p + 1] - a.toff2[p]);
  lo[0] = lo[1] = sl[0] = sl[1] = 0;
  w = false;
  if (k < 0 || k >= a.n_reads) return;
  const int64_t s = a.start[k * a.stride], e = a.stop[k * a.stride], t = a.tlen[k * a.stride];
  w = s >= 0 && e >= 0 && s < e;
  if (!w) return;
  trim_py_slice(a.off1[p + 1] - a.off1[p], s, e, e > t, lo[0], sl[0]);            // R1[start:stop], [start:] where stop > tlen
  trim_py_slice(a.off2[p + 1] - a.off2[p], t - e, t - s, (t - s) > t, lo[1], sl[1]);      // R2[tlen - stop : tlen - start]
}

template <bool SCATTER> __global__ __launch_bounds__(TR_BLOCK) void k_trim_pair_plan(TrimPairPlanArgs a)
{
  const int64_t base = (int64_t)blockIdx.x * TR_TILE + (int64_t)threadIdx.x * TR_ITEMS;
  const int64_t extra = a.ccs ? 34 : 0;
  int32_t tl[TR_ITEMS][2], lo[TR_ITEMS][2], sl[TR_ITEMS][2]; bool w[TR_ITEMS];
  int64_t v[3] = {0, 0, 0};                      // bytes of R1's text, of R2's text, pairs written
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t p = base + i;
    w[i] = false; tl[i][0] = tl[i][1] = lo[i][0] = lo[i][1] = sl[i][0] = sl[i][1] = 0;
    if (p < a.n) trim_pair_one(a, p, tl[i], lo[i], sl[i], w[i]);
    if (w[i]) { v[0] += (int64_t)tl[i][0] + 5 + 2 * ((int64_t)sl[i][0] + extra); v[1] += (int64_t)tl[i][1] + 5 + 2 * ((int64_t)sl[i][1] + extra); v[2]++; }
  }
  int64_t ex[3], tot[3];
  block_scan64<3, TR_BLOCK>(v, ex, tot);
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk[blockIdx.x * 3 + 0] = tot[0]; a.blk[blockIdx.x * 3 + 1] = tot[1]; a.blk[blockIdx.x * 3 + 2] = tot[2]; }
    return;
  }
  int64_t o1 = a.blk[blockIdx.x * 3 + 0] + ex[0], o2 = a.blk[blockIdx.x * 3 + 1] + ex[1], c = a.blk[blockIdx.x * 3 + 2] + ex[2];
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t p = base + i;
    if (p >= a.n) break;
    TrimRec q;
    q.out = o1; q.src = a.off1[p] + lo[i][0]; q.toff = a.toff1[p]; q.tl = tl[i][0]; q.slen = sl[i][0];
    a.rec1[p] = q;
    q.out = o2; q.src = a.off2[p] + lo[i][1]; q.toff = a.toff2[p]; q.tl = tl[i][1]; q.slen = sl[i][1];
    a.rec2[p] = q;
    a.cnt[p] = c;
    if (w[i]) { o1 += (int64_t)tl[i][0] + 5 + 2 * ((int64_t)sl[i][0] + extra); o2 += (int64_t)tl[i][1] + 5 + 2 * ((int64_t)sl[i][1] + extra); c++; }
  }
}

__global__ __launch_bounds__(TR_BLOCK) void k_trim_pair_plan_sums(TrimPairPlanArgs a, int64_t nb)
{
  int64_t carry[3];
  trim_scan_tiles(a.blk, nb, carry);
  if (threadIdx.x == 0) {
    TrimRec q;
    q.src = 0; q.toff = 0; q.tl = 0; q.slen = 0;
    q.out = carry[0]; a.rec1[a.n] = q;
    q.out = carry[1]; a.rec2[a.n] = q;
    a.cnt[a.n] = carry[2];
  }
}

// bounds[k][s] for k = 0 (R1's byte offset), 1 (R2's), 2 (pairs written) at the first pair of sample s, s = 0 .. S (first[S] = n)
__global__ void k_trim_pair_bounds(const TrimRec *__restrict__ rec1, const TrimRec *__restrict__ rec2, const int64_t *__restrict__ cnt,
                                   const int64_t *__restrict__ first, int32_t S, int64_t *__restrict__ bounds)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > S) return;
  const int64_t p = first[s];
  bounds[s] = rec1[p].out; bounds[(S + 1) + s] = rec2[p].out; bounds[2 * (S + 1) + s] = cnt[p];
}

void launch_trim_pair_plan(const TrimPairPlanArgs &a, const int64_t *first, int32_t S, int64_t *bounds, hipStream_t st)
{
  const int64_t nb = trim_plan_blocks(a.n);
  if (nb > 0) hipLaunchKernelGGL(k_trim_pair_plan<false>, dim3((unsigned)nb), dim3(TR_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_pair_plan_sums, dim3(1), dim3(TR_BLOCK), 0, st, a, nb);
  if (nb > 0) hipLaunchKernelGGL(k_trim_pair_plan<true>, dim3((unsigned)nb), dim3(TR_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_pair_bounds, dim3((unsigned)((S + 1 + 255) / 256)), dim3(256), 0, st, a.rec1, a.rec2, a.cnt, first, S, bounds);
}

// ---- the copy ------------------------------------------------------------------------------------------------------------------
__device__ const char TRIM_CCS_FWD[18] = "GACAGGTACAAGAAGGA", TRIM_CCS_REV[18] = "TTAACCCAGTCTCCAGT";

// the last record of [lo, hi) that starts at or before byte o (rec[lo].out <= o): it holds o when o is below the batch's total, because
// a record that is not written starts where its successor starts and so is never the last
__device__ __forceinline__ int64_t trim_find(const TrimRec *__restrict__ rec, int64_t lo, int64_t hi, int64_t o)
{
  while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (rec[mid].out <= o) lo = mid; else hi = mid; }
  return lo;
}
// four bytes at any address: the two aligned dwords that hold them, shifted (every source plane is padded past its end)
__device__ __forceinline__ uint32_t trim_load4(const uint8_t *p)
{
  const uint32_t *w = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3);
  const uint64_t both = ((uint64_t)w[1] << 32) | w[0];
  return (uint32_t)(both >> (8 * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3)));
}
// byte p of record q's text (qs: its first kept quality in a.qual).  fl (FLIP only): the record is flipped -- q.src / qs are where its
// slice's FIRST base / quality sits, the slice runs backwards from there, and a base goes through the complement table
template <bool FLIP> __device__ __forceinline__ uint32_t trim_byte(const TrimCopyArgs &a, const TrimRec &q, int64_t qs, int64_t p, bool fl, const uint8_t *comp)
{
  const int64_t pre = a.ccs ? 17 : 0;
  if (p < q.tl) return a.titles[q.toff + p];
  p -= q.tl;
  if (p == 0) return '\n';
  p -= 1;
  if (p < q.slen + 2 * pre) {
    if (p < pre) return (uint8_t)TRIM_CCS_FWD[p];
    p -= pre;
    if (FLIP && fl && p < q.slen) return comp[a.seq[q.src - p]];
    return p < q.slen ? a.seq[q.src + p] : (uint8_t)TRIM_CCS_REV[p - q.slen];
  }
  p -= q.slen + 2 * pre;
  if (p < 3) return p == 1 ? '+' : '\n';
  p -= 3;
  if (p < q.slen + 2 * pre) {
    p -= pre;
    if (FLIP && fl && p >= 0 && p < q.slen) return a.qual[qs - p];
    return (p >= 0 && p < q.slen) ? a.qual[qs + p] : '~';
  }
  return '\n';
}

// QS: a record's qualities start at a.qsrc[r] (a unit of raw text, where all three planes are that text), not at rec[r].src
// FLIP (a unit with strands, QS only): a.qsrc[r] < 0 marks a record written from its reverse complement; ~a.qsrc[r] and rec[r].src are
// then the source bytes of its slice's first quality and base, and output byte p comes from source byte (first - p).  A dword wholly
// inside such a line is the two aligned loads that hold source bytes s - 3 .. s, byte-reversed, and for bases four look-ups in the
// complement table (256 bytes of LDS = 64 dwords, one per bank: lanes that meet in a dword read the same dword, which is a broadcast).
// The lanes' source addresses run DOWN by one dword per lane where they ran up: the wave still reads one contiguous stretch.
// A base line never starts at byte 0 of a unit (its title precedes it), so s - 3 is inside the text.
template <bool QS, bool FLIP> __global__ __launch_bounds__(TC_BLOCK) void k_trim_copy(TrimCopyArgs a)
{
  static_assert(QS || !FLIP, "only a unit of raw text has flipped records");
  const int64_t pre = a.ccs ? 17 : 0;
  __shared__ uint8_t comp[FLIP ? 256 : 4];
  if (FLIP) { comp[threadIdx.x] = a.comp[threadIdx.x]; __syncthreads(); }
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t t0 = tile * TC_TILE, t1 = t0 + TC_TILE < a.total ? t0 + TC_TILE : a.total;
    const int64_t rlo = trim_find(a.rec, 0, a.n, t0), rhi = trim_find(a.rec, rlo, a.n, t1 - 1);      // the same in every lane
#pragma unroll 4
    for (int j = 0; j < TC_DWORDS; j++) {
      const int64_t o = t0 + ((int64_t)j * TC_BLOCK + threadIdx.x) * 4;
      if (o >= t1) break;
      int64_t r = trim_find(a.rec, rlo, rhi + 1, o);
      TrimRec q = a.rec[r];
      int64_t next = a.rec[r + 1].out;
      const int64_t p = o - q.out;
      const uint8_t *src = nullptr;
      int64_t qs = 0; bool fl = false;           // (FLIP only)
      int rev = 0;                               // 1: a flipped record's qualities, 2: its bases
      if (FLIP) { qs = a.qsrc[r]; fl = qs < 0; if (fl) qs = ~qs; }
      if (o + 4 <= next) {                       // the dword lies in one record: in one of its three sources?
        const int64_t ps = p - q.tl - 1 - pre, pq = ps - q.slen - 2 * pre - 3;
        if (p + 4 <= q.tl) src = a.titles + q.toff + p;
        else if (ps >= 0 && ps + 4 <= q.slen) {
          if (FLIP && fl) { src = a.seq + q.src - ps - 3; rev = 2; }
          else src = a.seq + q.src + ps;
        } else if (pq >= 0 && pq + 4 <= q.slen) {
          if (FLIP && fl) { src = a.qual + qs - pq - 3; rev = 1; }
          else src = a.qual + (FLIP ? qs : QS ? a.qsrc[r] : q.src) + pq;
        }
      }
      uint32_t v = 0;
      if (src) {
        v = trim_load4(src);
        if (FLIP && rev) {
          v = __builtin_bswap32(v);
          if (rev == 2) v = (uint32_t)comp[v & 255] | ((uint32_t)comp[(v >> 8) & 255] << 8) | ((uint32_t)comp[(v >> 16) & 255] << 16) | ((uint32_t)comp[v >> 24] << 24);
        }
      } else {
        for (int b = 0; b < 4; b++) {
          const int64_t ob = o + b;
          if (ob >= a.total) break;              // the text's last dword: the bytes past its end stay 0 (the buffer is padded to whole tiles)
          while (ob >= next) {
            r++; q = a.rec[r]; next = a.rec[r + 1].out;
            if (FLIP) { qs = a.qsrc[r]; fl = qs < 0; if (fl) qs = ~qs; }
          }
          v |= trim_byte<FLIP>(a, q, FLIP ? qs : QS ? a.qsrc[r] : q.src, ob - q.out, fl, comp) << (8 * b);
        }
      }
      a.out[o >> 2] = v;
    }
  }
}

int64_t trim_copy_bytes(int64_t total) { return (total + TC_TILE - 1) / TC_TILE * TC_TILE; }

void launch_trim_copy(TrimCopyArgs a, hipStream_t st)
{
  if (a.total <= 0) return;
  a.ntiles = (a.total + TC_TILE - 1) / TC_TILE;
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, 256 * 8);
  if (a.qsrc && a.comp) hipLaunchKernelGGL((k_trim_copy<true, true>), dim3(grid), dim3(TC_BLOCK), 0, st, a);
  else if (a.qsrc) hipLaunchKernelGGL((k_trim_copy<true, false>), dim3(grid), dim3(TC_BLOCK), 0, st, a);
  else hipLaunchKernelGGL((k_trim_copy<false, false>), dim3(grid), dim3(TC_BLOCK), 0, st, a);
}

// ---- a unit of raw FASTQ text (itsx_twriter_set_device) -------------------------------------------------------------------------
// The line index: a thread looks at 16 bytes (one aligned load), the newlines among them are a 16-bit mask, its popcount goes through
// the block's scan and the tiles' sums through one more, and the newline that is the k-th of the unit ends line k and starts line k + 1.
// As Records::line of trim_host.cpp: a '\r' before the newline is not part of the line, a last line without a newline counts.
constexpr int LI_BLOCK = 256;
constexpr int64_t LI_TILE = (int64_t)LI_BLOCK * 16;

template <bool SCATTER> __global__ __launch_bounds__(LI_BLOCK) void k_trim_index(TrimUnitArgs a)
{
  if (SCATTER && a.info[0] != 4 * a.count) return;             // (the same in every thread)
  const int64_t p0 = (int64_t)blockIdx.x * LI_TILE + (int64_t)threadIdx.x * 16;
  uint32_t m = trim_newlines16(a.text, a.nbytes, p0);
  int64_t v[1] = {(int64_t)__popc(m)}, ex[1], tot[1];
  block_scan64<1, LI_BLOCK>(v, ex, tot);
  if (!SCATTER) { if (threadIdx.x == 0) a.lblk[blockIdx.x] = tot[0]; return; }
  const int64_t cap = 4 * a.count;
  int64_t k = a.lblk[blockIdx.x] + ex[0];
  while (m) {
    const int64_t p = p0 + (__ffs((int)m) - 1);
    m &= m - 1;
    if (k < cap) { a.le[k] = (int32_t)(p - ((p > 0 && a.text[p - 1] == '\r') ? 1 : 0)); a.ls[k + 1] = (int32_t)(p + 1); }
    k++;
  }
}
// the tiles' newline counts -> their exclusive prefixes, in place; info[0] = the unit's lines; the first line's start and, where the
// text does not end in a newline, the last line's end
__global__ __launch_bounds__(LI_BLOCK) void k_trim_index_sums(TrimUnitArgs a, int64_t nb)
{
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += LI_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    int64_t v[1] = {b < nb ? a.lblk[b] : 0}, ex[1], tot[1];
    block_scan64<1, LI_BLOCK>(v, ex, tot);
    if (b < nb) a.lblk[b] = carry + ex[0];
    carry += tot[0];
  }
  if (threadIdx.x == 0) {
    const bool open = a.nbytes > 0 && a.text[a.nbytes - 1] != '\n';
    const int64_t lines = carry + (open ? 1 : 0);
    a.info[0] = lines;
    if (lines == 4 * a.count && a.count > 0) {
      a.ls[0] = 0;
      if (open) a.le[carry] = (int32_t)(a.nbytes - (a.text[a.nbytes - 1] == '\r' ? 1 : 0));
    }
  }
}

// record r of the unit = lines 4 r .. 4 r + 3: whether it is written and its slice, as itsx_twriter::work decides both (mode 0: written
// iff start >= 0 && stop >= 0 && start < stop; mode 1: iff stop != INT32_MIN, INT32_MAX an open end), and whether it is a record at all
// flip (a.strand, mode 0): the record's strand is -1 -- its slice is that of the reversed read, so its first base and quality are source
// byte L - 1 - lo of their lines and the copy walks down from there (fs: that offset instead of lo); the output's length is the same
struct TrimUnitOne { int32_t t0, s0, q0, tl, lo, sl, fs; bool w, bad, flip; };
__device__ __forceinline__ TrimUnitOne trim_unit_one(const TrimUnitArgs &a, int64_t r)
{
  TrimUnitOne u;
  const int32_t p0 = a.ls[4 * r + 2];
  u.t0 = a.ls[4 * r]; u.s0 = a.ls[4 * r + 1]; u.q0 = a.ls[4 * r + 3];
  u.tl = a.le[4 * r] - u.t0;
  const int32_t L = a.le[4 * r + 1] - u.s0, pl = a.le[4 * r + 2] - p0, ql = a.le[4 * r + 3] - u.q0;
  u.bad = u.tl <= 0 || a.text[u.t0] != '@' || pl <= 0 || a.text[p0] != '+' || ql != L;
  const int64_t s = a.start[r], e = a.stop[r];
  if (a.mode == 1) { u.w = e != (int64_t)INT32_MIN; trim_py_slice(L, s, e, e == (int64_t)INT32_MAX, u.lo, u.sl); }
  else { u.w = s >= 0 && e >= 0 && s < e; trim_py_slice(L, s, e, false, u.lo, u.sl); }
  if (u.bad) { u.w = false; u.lo = u.sl = 0; }
  u.flip = a.strand && a.mode == 0 && !u.bad && a.strand[r] < 0;
  u.fs = u.flip ? L - 1 - u.lo : u.lo;
  return u;
}

template <bool SCATTER> __global__ __launch_bounds__(TR_BLOCK) void k_trim_unit_plan(TrimUnitArgs a)
{
  if (a.info[0] != 4 * a.count) return;                        // (the same in every thread)
  const int64_t base = (int64_t)blockIdx.x * TR_TILE + (int64_t)threadIdx.x * TR_ITEMS;
  const int64_t extra = a.ccs ? 34 : 0;
  TrimUnitOne u[TR_ITEMS];
  int64_t v[3] = {0, 0, 0};                      // bytes of text, records, total_len as itsx_twriter::work counts it
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t r = base + i;
    u[i].w = false; u[i].bad = false; u[i].flip = false;
    if (r < a.count) u[i] = trim_unit_one(a, r);
    if (u[i].w) { v[0] += (int64_t)u[i].tl + 5 + 2 * ((int64_t)u[i].sl + extra); v[1]++; v[2] += (int64_t)u[i].sl + extra; }
    if (!SCATTER && u[i].bad) a.info[1] = 1;
  }
  int64_t ex[3], tot[3];
  block_scan64<3, TR_BLOCK>(v, ex, tot);
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk[blockIdx.x * 3 + 0] = tot[0]; a.blk[blockIdx.x * 3 + 1] = tot[1]; a.blk[blockIdx.x * 3 + 2] = tot[2]; }
    return;
  }
  int64_t o = a.blk[blockIdx.x * 3 + 0] + ex[0];
#pragma unroll
  for (int i = 0; i < TR_ITEMS; i++) {
    const int64_t r = base + i;
    if (r >= a.count) break;
    TrimRec q;
    q.out = o; q.src = (int64_t)u[i].s0 + u[i].fs; q.toff = u[i].t0; q.tl = u[i].tl; q.slen = u[i].sl;
    a.rec[r] = q; a.qsrc[r] = u[i].flip ? ~((int64_t)u[i].q0 + u[i].fs) : (int64_t)u[i].q0 + u[i].fs;
    if (u[i].w) o += (int64_t)u[i].tl + 5 + 2 * ((int64_t)u[i].sl + extra);
  }
}
__global__ __launch_bounds__(TR_BLOCK) void k_trim_unit_plan_sums(TrimUnitArgs a, int64_t nb)
{
  if (a.info[0] != 4 * a.count) return;
  int64_t carry[3];
  trim_scan_tiles(a.blk, nb, carry);
  if (threadIdx.x == 0) {
    TrimRec q;
    q.out = carry[0]; q.src = 0; q.toff = 0; q.tl = 0; q.slen = 0;
    a.rec[a.count] = q; a.qsrc[a.count] = 0;
    a.info[2] = carry[0]; a.info[3] = carry[1]; a.info[4] = carry[2];
  }
}

int64_t trim_index_blocks(int64_t nbytes) { return (nbytes + LI_TILE - 1) / LI_TILE; }

void launch_trim_unit(const TrimUnitArgs &a, hipStream_t st)
{
  (void)hipMemsetAsync(a.info, 0, sizeof(int64_t) * TRIM_UNIT_INFO, st);
  const int64_t nbi = trim_index_blocks(a.nbytes), nbp = trim_plan_blocks(a.count);
  if (nbi > 0) hipLaunchKernelGGL(k_trim_index<false>, dim3((unsigned)nbi), dim3(LI_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_index_sums, dim3(1), dim3(LI_BLOCK), 0, st, a, nbi);
  if (nbi > 0) hipLaunchKernelGGL(k_trim_index<true>, dim3((unsigned)nbi), dim3(LI_BLOCK), 0, st, a);
  if (nbp > 0) hipLaunchKernelGGL(k_trim_unit_plan<false>, dim3((unsigned)nbp), dim3(TR_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_trim_unit_plan_sums, dim3(1), dim3(TR_BLOCK), 0, st, a, nbp);
  if (nbp > 0) hipLaunchKernelGGL(k_trim_unit_plan<true>, dim3((unsigned)nbp), dim3(TR_BLOCK), 0, st, a);
}

// ---- itsx_orient_apply with records: kept read j = read from[j] of the old planes, reversed (bases complemented) where its strand is -1;
// one wave per read, lanes along it
__global__ __launch_bounds__(256) void k_trim_orient(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual, const int64_t *__restrict__ off,
                                                     const int32_t *__restrict__ from, const int8_t *__restrict__ strand, const uint8_t *__restrict__ comp,
                                                     const int64_t *__restrict__ noff, int64_t m, uint8_t *__restrict__ nseq, uint8_t *__restrict__ nqual)
{
  const int lane = threadIdx.x & 63;
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < m; j += (int64_t)gridDim.x * 4) {
    const int64_t r = from[j], so = off[r], d0 = noff[j], len = noff[j + 1] - d0;
    if (strand[r] > 0) for (int64_t k = lane; k < len; k += 64) { nseq[d0 + k] = seq[so + k]; nqual[d0 + k] = qual[so + k]; }
    else for (int64_t k = lane; k < len; k += 64) { nseq[d0 + k] = comp[seq[so + len - 1 - k]]; nqual[d0 + k] = qual[so + len - 1 - k]; }
  }
}

void launch_trim_orient(const uint8_t *seq, const uint8_t *qual, const int64_t *off, const int32_t *from, const int8_t *strand, const uint8_t *comp,
                        const int64_t *noff, int64_t m, uint8_t *nseq, uint8_t *nqual, hipStream_t st)
{
  if (m <= 0) return;
  hipLaunchKernelGGL(k_trim_orient, dim3((unsigned)std::min<int64_t>((m + 3) / 4, 65535)), dim3(256), 0, st, seq, qual, off, from, strand, comp, noff, m, nseq, nqual);
}

}  // namespace itsx
