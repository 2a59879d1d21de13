// k_merge.hip -- SURVEY section 8f row f2: paired-end read merging on the device.
//
// Replaces `vsearch --fastq_mergepairs R1 --reverse R2 --fastqout seq.fq --fastq_maxdiffs 40 --fastq_maxee 2
// --fastq_qmax 93 [--fastq_allowmergestagger]` (reference call site itsxpress/SeqSample.py:266-365).  The procedure is
// the one the CPU test oracle restates (PARITY UNPINNED: the reference's merged fixture was made by another tool):
// ungapped diagonals sharing >= 4 5-mers are scored with quality-aware log-odds, walked from the forward read's 3' end;
// the single diagonal scoring >= 16 wins; overlap bases/qualities follow Edgar & Flyvbjerg (2015); expected errors of
// the merged read <= maxee.
//
// One wave per pair.  Both reads (the reverse one reverse-complemented) and their 5-mer codes live in LDS; lane l owns
// diagonals l, l+64, ...: counting shared 5-mers is a compare of two LDS streams (one of them a broadcast), scoring a
// candidate is a sequential double sum in exactly the oracle's order (the tables are built on the host with the same
// libm calls and read through L2), so scores, and therefore every accept/reject decision, are bit-identical.  The merged
// read is written by all lanes; its expected-error sum is again sequential (lane 0).  Byte/integer work plus a few
// hundred double adds per pair: latency-bound, hidden by running many waves per CU.
#include <algorithm>
#include "engine.h"
#include "k_api.h"
#include "k_scan.h"

namespace itsx {

// the kernel's view of a base is its upper case (include/itsx_hip.h): applied where a read enters LDS
__device__ __forceinline__ uint8_t upper_base(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
__device__ __forceinline__ int base_code(uint8_t c)
{
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : 4;
}
__device__ __forceinline__ uint8_t comp_base(uint8_t c)
{
  return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : (c == 'T' || c == 'U') ? 'A' : 'N';
}

// INDEXED: the shared 5-mers of every diagonal come from a 5-mer -> positions index of the forward read (LDS: 1024 chain
// heads + one link per position), O(fl + rl + matches) instead of one compare per (diagonal, position); needs 13 B of LDS
// per base, so pairs longer than 4096 bases in total take the plain variant.
// JOIN (itsx_set_merge_join): a pair whose mates do not overlap -- reason 1, 3 or 5 -- is kept as R1 + "NNNNNNNN" + revcomp(R2) with
// qualities Q1 + "IIIIIIII" + reversed Q2, vsearch --fastq_join's padding as its manual gives it (PARITY UNPINNED, as the merge: no
// vsearch build was at hand).  Both mates are in LDS when the verdict falls, so the join is five copies by all lanes; no LDS is added.
// The joined read is 8 bytes longer than its mates, so with JOIN pair i's slot starts at foff[i] + roff[i] + 8 i.  No expected-error
// filter (--fastq_join has none); reason[i] keeps its code, joined[i] marks the read.
constexpr int JOIN_PAD = 8;
template <bool INDEXED, bool JOIN> __global__ __launch_bounds__(64) void k_merge(MergeArgs a)
{
  extern __shared__ uint8_t lds[];
  const int lane = threadIdx.x;
  for (int64_t pr = blockIdx.x; pr < a.n; pr += gridDim.x) {
    const int64_t fo = a.foff[pr], ro = a.roff[pr];
    const int fl = (int)(a.foff[pr + 1] - fo), rl = (int)(a.roff[pr + 1] - ro);
    const int64_t oo = fo + ro + (JOIN ? (int64_t)JOIN_PAD * pr : 0);      // merged reads are at most fl + rl long, joined ones fl + 8 + rl
    __syncthreads();
    if (fl < 1 || rl < 1 || fl + rl > a.max_total) {
      if (lane == 0) { a.out_len[pr] = 0; a.reason[pr] = 8; a.score[pr] = 0.0; a.shift[pr] = 0; if (JOIN) a.joined[pr] = 0; }
      continue;
    }
    uint8_t *fs = lds, *fq = fs + fl, *rs = fq + fl, *rq = rs + rl, *mq = rq + rl;       // mq: merged qualities (fl + rl)
    uint16_t *f5 = reinterpret_cast<uint16_t *>(lds + ((2 * fl + 2 * rl + fl + rl + 1) & ~1));
    uint16_t *r5 = f5 + fl;
    int32_t *head = reinterpret_cast<int32_t *>(lds + ((5 * (fl + rl) + 8) & ~3));      // INDEXED only: [1024], then next[fl], diag[fl + rl - 1]
    int32_t *nextp = head + 1024, *diag = nextp + fl;
    for (int p = lane; p < fl; p += 64) { fs[p] = upper_base(a.fseq[fo + p]); fq[p] = a.fqual[fo + p]; }
    for (int j = lane; j < rl; j += 64) { rs[j] = comp_base(upper_base(a.rseq[ro + rl - 1 - j])); rq[j] = a.rqual[ro + rl - 1 - j]; }
    __syncthreads();
    for (int p = lane; p < fl; p += 64) {
      int v = 0; bool ok = p + 5 <= fl;
      for (int t = 0; t < 5 && ok; t++) { const int c = base_code(fs[p + t]); if (c > 3) ok = false; v = v * 4 + c; }
      f5[p] = ok ? (uint16_t)v : (uint16_t)0xFFFF;
    }
    for (int p = lane; p < rl; p += 64) {
      int v = 0; bool ok = p + 5 <= rl;
      for (int t = 0; t < 5 && ok; t++) { const int c = base_code(rs[p + t]); if (c > 3) ok = false; v = v * 4 + c; }
      r5[p] = ok ? (uint16_t)v : (uint16_t)0xFFFE;             // a different sentinel: two invalid 5-mers never match
    }
    __syncthreads();
    const int ndiag = fl + rl - 1;
    if (INDEXED) {
      for (int i = lane; i < 1024; i += 64) head[i] = -1;
      for (int i = lane; i < ndiag; i += 64) diag[i] = 0;
      __syncthreads();
      for (int p = lane; p < fl; p += 64) if (f5[p] != 0xFFFF) nextp[p] = atomicExch(&head[f5[p]], p);
      __syncthreads();
      for (int j = lane; j < rl; j += 64) {
        if (r5[j] == 0xFFFE) continue;
        for (int p = head[r5[j]]; p >= 0; p = nextp[p]) atomicAdd(&diag[fl - 1 - (p - j)], 1);
      }
      __syncthreads();
    }
    // ---- diagonals: idx 0 = the largest shift (fl - 1), ascending idx = the oracle's order
    double best = 0.0; int best_idx = 0x7fffffff, best_diffs = 0, hits = 0, kmers = 0;
    for (int idx = lane; idx < ndiag; idx += 64) {
      const int shift = fl - 1 - idx;
      const int lo = shift > 0 ? shift : 0, hi = (shift + rl < fl) ? shift + rl : fl;
      int cnt = 0;
      if (INDEXED) cnt = diag[idx];
      else for (int p = lo; p < hi; p++) cnt += (f5[p] == r5[p - shift]) ? 1 : 0;
      if (cnt < 4) continue;
      kmers = 1;
      double score = 0.0, high = 0.0, drop = 0.0;
      int diffs = 0;
      for (int p = hi - 1; p >= lo; p--) {
        const int qa = fq[p], qb = rq[p - shift];
        if (fs[p] == rs[p - shift]) score += a.match[qa * 128 + qb];
        else { score += a.mism[qa * 128 + qb]; diffs++; }
        if (score > high) high = score;
        if (high - score > drop) drop = high - score;
      }
      if (drop >= 16.0) score = -1000.0;
      if (score >= 16.0) hits++;
      if (best_idx == 0x7fffffff || score > best) { best = score; best_idx = idx; best_diffs = diffs; }
    }
    // ---- best over the wave: higher score, then the smaller idx (= evaluated first)
    for (int off = 32; off; off >>= 1) {
      const double os = __shfl_xor(best, off); const int oi = __shfl_xor(best_idx, off), od = __shfl_xor(best_diffs, off);
      hits += __shfl_xor(hits, off); kmers |= __shfl_xor(kmers, off);
      const bool take = oi != 0x7fffffff && (best_idx == 0x7fffffff || os > best || (os == best && oi < best_idx));
      if (take) { best = os; best_idx = oi; best_diffs = od; }
    }
    const int shift = best_idx == 0x7fffffff ? 0 : fl - 1 - best_idx;
    const int lo = shift > 0 ? shift : 0, hi = (shift + rl < fl) ? shift + rl : fl;
    int reason = 0;
    if (!kmers) reason = 1;
    else if (hits > 1) reason = 2;
    else if (best < 16.0) reason = 3;
    else if (best_diffs > a.maxdiffs) reason = 4;
    else if (hi - lo < 10) reason = 5;
    else if (!a.allow_stagger && shift < 0) reason = 6;
    int mlen = 0;
    if (reason == 0) {
      const int tail = (shift + rl >= fl) ? rl - (hi - shift) : 0;       // reverse-read bases after the overlap
      mlen = hi + tail;
      for (int n = lane; n < mlen; n += 64) {
        uint8_t s, q;
        if (n < lo) { s = fs[n]; q = fq[n]; }
        else if (n < hi) {
          const uint8_t f = fs[n], r = rs[n - shift], qa = fq[n], qb = rq[n - shift];
          if (r == 'N') { s = f; q = qa; }
          else if (f == 'N') { s = r; q = qb; }
          else if (f == r) { s = f; q = a.qsame[qa * 128 + qb]; }
          else if (qa > qb) { s = f; q = a.qdiff[qa * 128 + qb]; }
          else { s = r; q = a.qdiff[qb * 128 + qa]; }
        } else { const int j = n - shift; s = rs[j]; q = rq[j]; }
        a.out_seq[oo + n] = s; a.out_qual[oo + n] = q; mq[n] = q;
      }
    }
    bool join = false;
    if (JOIN && (reason == 1 || reason == 3 || reason == 5)) {       // (the verdict is the same in every lane)
      join = true;
      mlen = fl + JOIN_PAD + rl;
      uint8_t *os = a.out_seq + oo, *oq = a.out_qual + oo;
      for (int p = lane; p < fl; p += 64) { os[p] = fs[p]; oq[p] = fq[p]; }
      if (lane < JOIN_PAD) { os[fl + lane] = 'N'; oq[fl + lane] = 'I'; }
      for (int j = lane; j < rl; j += 64) { os[fl + JOIN_PAD + j] = rs[j]; oq[fl + JOIN_PAD + j] = rq[j]; }
    }
    __syncthreads();
    if (lane == 0) {
      if (reason == 0) {
        double ee = 0.0;
        for (int n = 0; n < mlen; n++) ee += a.q2p[mq[n]];
        if (ee > a.maxee) { reason = 7; mlen = 0; }
      }
      a.out_len[pr] = mlen; a.reason[pr] = reason; a.score[pr] = best_idx == 0x7fffffff ? 0.0 : best; a.shift[pr] = shift;
      if (JOIN) a.joined[pr] = join ? 1 : 0;
    }
  }
}

void launch_merge(const MergeArgs &a, hipStream_t st)
{
  if (a.n <= 0) return;
  const int grid = (int)std::min<int64_t>(a.n, 65536);
  if (a.max_total <= 4096) {
    const size_t lds = (size_t)a.max_total * 13 + 4096 + 64;  // + chain heads, links and diagonal counters (4 B each)
    if (a.join) hipLaunchKernelGGL((k_merge<true, true>), dim3(grid), dim3(64), lds, st, a);
    else hipLaunchKernelGGL((k_merge<true, false>), dim3(grid), dim3(64), lds, st, a);
  } else {
    const size_t lds = (size_t)a.max_total * 5 + 16;          // bases, qualities, merged qualities (1 B each x 3) + 5-mer codes (2 B)
    if (a.join) hipLaunchKernelGGL((k_merge<false, true>), dim3(grid), dim3(64), lds, st, a);
    else hipLaunchKernelGGL((k_merge<false, false>), dim3(grid), dim3(64), lds, st, a);
  }
}

// ---- compaction of the merge kernel's output: which pairs merged, where their reads go ------------------------------------------
// The merge kernel leaves pair i's read (if reason[i] == 0) at foff[i] + roff[i], out_len[i] bases long.  The read set wants the merged
// reads gap-free, in pair order, and -- for a batch of samples -- to know each read's sample.  A two-level exclusive scan over the
// pairs of (merged ? 1 : 0, merged ? out_len : 0): every block of MC_TILE pairs sums its tile (k_merge_compact<false>), one block scans
// the tiles' sums (k_merge_compact_sums), and every block scans its tile again and scatters (k_merge_compact<true>).  Counts and byte
// offsets are 64-bit throughout: a batch's text can pass 2^31 bytes.  After a merge that joins (MergeCompactArgs::join) a read is a
// pair with out_len > 0 -- merged or joined -- and pair i's read sits 8 i bytes further on.
constexpr int MC_BLOCK = 256;
constexpr int MC_ITEMS = 8;
constexpr int MC_TILE = MC_BLOCK * MC_ITEMS;   // pairs per block; thread t owns MC_ITEMS consecutive pairs

// exclusive prefix of (c, l) over the block's threads in thread order, and the block's sums (k_scan.h)
__device__ __forceinline__ void mc_block_scan(int64_t c, int64_t l, int64_t &ec, int64_t &el, int64_t &tc, int64_t &tl)
{
  const int64_t v[2] = {c, l};
  int64_t ex[2], tot[2];
  block_scan64<2, MC_BLOCK>(v, ex, tot);
  ec = ex[0]; el = ex[1]; tc = tot[0]; tl = tot[1];
}

template <bool SCATTER> __global__ __launch_bounds__(MC_BLOCK) void k_merge_compact(MergeCompactArgs a)
{
  const int64_t base = (int64_t)blockIdx.x * MC_TILE + (int64_t)threadIdx.x * MC_ITEMS;
  int32_t len[MC_ITEMS];
  int64_t c = 0, l = 0;
#pragma unroll
  for (int i = 0; i < MC_ITEMS; i++) {
    const int64_t p = base + i;
    const bool ok = p < a.n && (a.join ? a.out_len[p] > 0 : a.reason[p] == 0);      // join: merged and joined pairs alike
    len[i] = ok ? a.out_len[p] : -1;
    if (ok) { c++; l += len[i]; }
  }
  int64_t ec, el, tc, tl;
  mc_block_scan(c, l, ec, el, tc, tl);
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk_cnt[blockIdx.x] = tc; a.blk_len[blockIdx.x] = tl; }
    return;
  }
  int64_t j = a.blk_cnt[blockIdx.x] + ec, d = a.blk_len[blockIdx.x] + el;     // this thread's first read and its first byte
  int32_t s = -1; unsigned long long run = 0;                               // the sample of the reads counted in `run`
#pragma unroll
  for (int i = 0; i < MC_ITEMS; i++) {
    const int64_t p = base + i;
    if (p >= a.n) break;
    if (len[i] < 0) { a.pair_index[p] = -1; continue; }
    a.pair_index[p] = (int32_t)j;
    a.srcoff[j] = a.foff[p] + a.roff[p] + (a.join ? (int64_t)JOIN_PAD * p : 0);
    a.dstoff[j] = d;
    if (a.n_samples > 1) {
      if (s < 0 || p >= a.pair_start[s + 1]) {
        if (run) atomicAdd(reinterpret_cast<unsigned long long *>(a.sample_count + s), run);
        run = 0;
        // the sample whose pairs [pair_start[s], pair_start[s + 1]) hold p (empty samples repeat a start: the last of them is taken)
        int32_t lo = 0, hi = a.n_samples;
        while (hi - lo > 1) { const int32_t mid = (lo + hi) >> 1; if (a.pair_start[mid] <= p) lo = mid; else hi = mid; }
        s = lo;
      }
      a.sample[j] = s;
      run++;
    }
    j++; d += len[i];
  }
  if (run) atomicAdd(reinterpret_cast<unsigned long long *>(a.sample_count + s), run);
}

// the tiles' sums -> their exclusive prefixes, in place; total[0] = merged reads, total[1] = their bytes; dstoff[total[0]] = total[1]
__global__ __launch_bounds__(MC_BLOCK) void k_merge_compact_sums(int64_t *__restrict__ blk_cnt, int64_t *__restrict__ blk_len, int64_t nb,
                                                                 int64_t *__restrict__ total, int64_t *__restrict__ dstoff)
{
  int64_t cc = 0, cl = 0;                        // the sums of the chunks before this one
  for (int64_t b0 = 0; b0 < nb; b0 += MC_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    const int64_t c = b < nb ? blk_cnt[b] : 0, l = b < nb ? blk_len[b] : 0;
    int64_t ec, el, tc, tl;
    mc_block_scan(c, l, ec, el, tc, tl);
    if (b < nb) { blk_cnt[b] = cc + ec; blk_len[b] = cl + el; }
    cc += tc; cl += tl;
  }
  if (threadIdx.x == 0) { total[0] = cc; total[1] = cl; dstoff[cc] = cl; }
}

int64_t merge_compact_blocks(int64_t n) { return (n + MC_TILE - 1) / MC_TILE; }

void launch_merge_compact(const MergeCompactArgs &a, int64_t *total, hipStream_t st)
{
  if (a.n <= 0) return;
  const int64_t nb = merge_compact_blocks(a.n);
  hipLaunchKernelGGL(k_merge_compact<false>, dim3((unsigned)nb), dim3(MC_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_merge_compact_sums, dim3(1), dim3(MC_BLOCK), 0, st, a.blk_cnt, a.blk_len, nb, total, a.dstoff);
  hipLaunchKernelGGL(k_merge_compact<true>, dim3((unsigned)nb), dim3(MC_BLOCK), 0, st, a);
}

}  // namespace itsx
