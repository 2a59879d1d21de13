// k_fastq.hip -- FASTQ text taken apart on the device (itsx_parse_device; the whole-file loaders of a context that opted in with
// itsx_set_device_parse).  The rule is fastq_rec.h's, the one routine the host runs too.  Every position is 64-bit: a 10 M-read file
// is 3.6 GB of text.  Four steps, all bandwidth-bound (the text is read about three times and written about once):
//   count   a thread looks at 16 aligned bytes, the newlines among them are a 16-bit mask (k_lines.h), its popcount goes through the
//           block's scan: one count per 4096-byte tile, then one block turns the tiles' counts into their exclusive prefixes.
//   index   the same masks again: the newline that is the k-th of the text goes to nl[k].  Line k is (nl[k - 1], nl[k]); a last line
//           without a newline ends at nl[k] = nbytes.
//   plan    record r = lines 4 r .. 4 r + 3: checked (the lowest bad record and its reason: one atomicMin on a 64-bit word), its bases
//           and its title line measured, and two scans of the same shape as k_trim_unit_plan's give off[r] and toff[r].
//   gather  OUTPUT-stationary, once per plane (bases, qualities, title lines): a lane owns 16 aligned bytes of the plane and stores them
//           with one instruction, a wave-instruction 1 KiB.  It finds the record of its first byte by bisection between the records of
//           the tile's ends; where its 16 bytes come from one line they are five aligned dwords funnel-shifted into four -- the
//           misalignment of source against destination falls on the loads -- and at the seams between records they are copied byte by
//           byte.  Work follows output bytes: a 65 535-base read is spread over the lanes like anything else.
// A pair of texts (the paired merge loaders, itsx_parse_pairs_device) takes one more pass, a kernel of its own over both sides' finished
// planes (k_fastq_pairs): what the host path does between its parser and the merge kernel -- bases to upper case, qualities checked
// against 33..126, the longest pair measured.
#include <algorithm>
#include "engine.h"
#include "k_api.h"
#include "k_scan.h"
#include "k_lines.h"
#include "fastq_rec.h"

namespace itsx {

using namespace itsx_fq;

constexpr int FI_BLOCK = 256;
constexpr int64_t FI_TILE = (int64_t)FI_BLOCK * 16;          // bytes of the text per block of the index
constexpr int FP_BLOCK = 256;
constexpr int FP_ITEMS = 4;
constexpr int FP_TILE = FP_BLOCK * FP_ITEMS;                 // records per block of the plan's scan; thread t owns FP_ITEMS consecutive records
constexpr int FG_BLOCK = 256;
constexpr int FG_ITEMS = 4;                                  // 16-byte groups per lane of a gather tile
constexpr int64_t FG_TILE = (int64_t)FG_BLOCK * FG_ITEMS * 16;

// ---- the line index ------------------------------------------------------------------------------------------------------------
template <bool SCATTER> __global__ __launch_bounds__(FI_BLOCK) void k_fastq_index(FastqArgs a)
{
  const int64_t p0 = (int64_t)blockIdx.x * FI_TILE + (int64_t)threadIdx.x * 16;
  uint32_t m = trim_newlines16(a.text, a.nbytes, p0);
  int64_t v[1] = {(int64_t)__popc(m)}, ex[1], tot[1];
  block_scan64<1, FI_BLOCK>(v, ex, tot);
  if (!SCATTER) { if (threadIdx.x == 0) a.lblk[blockIdx.x] = tot[0]; return; }
  int64_t k = a.lblk[blockIdx.x] + ex[0];
  while (m) {
    const int64_t p = p0 + (__ffs((int)m) - 1);
    m &= m - 1;
    if (k < a.nnl) a.nl[k] = p;
    k++;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.nlines > a.nnl) a.nl[a.nnl] = a.nbytes;      // the unterminated last line
}

// the tiles' newline counts -> their exclusive prefixes, in place; info[1] = the text's newlines, info[0] = its lines
__global__ __launch_bounds__(FI_BLOCK) void k_fastq_index_sums(FastqArgs a, int64_t nb)
{
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += FI_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    int64_t v[1] = {b < nb ? a.lblk[b] : 0}, ex[1], tot[1];
    block_scan64<1, FI_BLOCK>(v, ex, tot);
    if (b < nb) a.lblk[b] = carry + ex[0];
    carry += tot[0];
  }
  if (threadIdx.x == 0) {
    const bool open = a.nbytes > 0 && a.text[a.nbytes - 1] != '\n';
    a.info[0] = carry + (open ? 1 : 0);
    a.info[1] = carry;
  }
}

// ---- the records: check and plan -----------------------------------------------------------------------------------------------
template <bool SCATTER> __global__ __launch_bounds__(FP_BLOCK) void k_fastq_plan(FastqArgs a)
{
  const int64_t base = (int64_t)blockIdx.x * FP_TILE + (int64_t)threadIdx.x * FP_ITEMS;
  int64_t sl[FP_ITEMS], tl[FP_ITEMS];
  int64_t v[2] = {0, 0};                         // bases, title bytes
  unsigned long long worst = FQ_VERDICT_NONE;
#pragma unroll
  for (int i = 0; i < FP_ITEMS; i++) {
    const int64_t r = base + i;
    sl[i] = tl[i] = 0;
    if (r < a.n) {
      const FqRec q = fq_record(a.text, a.nl, r);
      sl[i] = q.sl; tl[i] = q.tl;
      if (q.bad) { const unsigned long long w = fq_verdict(r, q.bad); worst = w < worst ? w : worst; }
    }
    v[0] += sl[i]; v[1] += tl[i];
  }
  if (!SCATTER && worst != FQ_VERDICT_NONE) atomicMin(reinterpret_cast<unsigned long long *>(a.info + 4), worst);
  int64_t ex[2], tot[2];
  block_scan64<2, FP_BLOCK>(v, ex, tot);
  if (!SCATTER) {
    if (threadIdx.x == 0) { a.blk[blockIdx.x * 2 + 0] = tot[0]; a.blk[blockIdx.x * 2 + 1] = tot[1]; }
    return;
  }
  int64_t o = a.blk[blockIdx.x * 2 + 0] + ex[0], t = a.blk[blockIdx.x * 2 + 1] + ex[1];
#pragma unroll
  for (int i = 0; i < FP_ITEMS; i++) {
    const int64_t r = base + i;
    if (r >= a.n) break;
    a.off[r] = o; a.toff[r] = t;
    o += sl[i]; t += tl[i];
  }
}

// the tiles' sums -> their exclusive prefixes, in place; entry n of off / toff and info[2], info[3] = the text's totals
__global__ __launch_bounds__(FP_BLOCK) void k_fastq_plan_sums(FastqArgs a, int64_t nb)
{
  int64_t carry[2] = {0, 0};
  for (int64_t b0 = 0; b0 < nb; b0 += FP_BLOCK) {
    const int64_t b = b0 + threadIdx.x;
    int64_t v[2], ex[2], tot[2];
#pragma unroll
    for (int k = 0; k < 2; k++) v[k] = b < nb ? a.blk[b * 2 + k] : 0;
    block_scan64<2, FP_BLOCK>(v, ex, tot);
#pragma unroll
    for (int k = 0; k < 2; k++) { if (b < nb) a.blk[b * 2 + k] = carry[k] + ex[k]; carry[k] += tot[k]; }
  }
  if (threadIdx.x == 0) { a.off[a.n] = carry[0]; a.toff[a.n] = carry[1]; a.info[2] = carry[0]; a.info[3] = carry[1]; }
}

int64_t fastq_index_blocks(int64_t nbytes) { return (nbytes + FI_TILE - 1) / FI_TILE; }
int64_t fastq_plan_blocks(int64_t n) { return (n + FP_TILE - 1) / FP_TILE; }

void launch_fastq_count(const FastqArgs &a, hipStream_t st)
{
  (void)hipMemsetAsync(a.info, 0, sizeof(int64_t) * FASTQ_INFO, st);
  (void)hipMemsetAsync(a.info + 4, 0xff, sizeof(int64_t), st);                  // FQ_VERDICT_NONE
  const int64_t nb = fastq_index_blocks(a.nbytes);
  if (nb > 0) hipLaunchKernelGGL(k_fastq_index<false>, dim3((unsigned)nb), dim3(FI_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_fastq_index_sums, dim3(1), dim3(FI_BLOCK), 0, st, a, nb);
}

void launch_fastq_index(const FastqArgs &a, hipStream_t st)
{
  const int64_t nb = fastq_index_blocks(a.nbytes);
  if (nb > 0) hipLaunchKernelGGL(k_fastq_index<true>, dim3((unsigned)nb), dim3(FI_BLOCK), 0, st, a);
}

void launch_fastq_plan(const FastqArgs &a, hipStream_t st)
{
  const int64_t nb = fastq_plan_blocks(a.n);
  if (nb > 0) hipLaunchKernelGGL(k_fastq_plan<false>, dim3((unsigned)nb), dim3(FP_BLOCK), 0, st, a);
  hipLaunchKernelGGL(k_fastq_plan_sums, dim3(1), dim3(FP_BLOCK), 0, st, a, nb);
  if (nb > 0) hipLaunchKernelGGL(k_fastq_plan<true>, dim3((unsigned)nb), dim3(FP_BLOCK), 0, st, a);
}

// ---- the gather ----------------------------------------------------------------------------------------------------------------
struct FastqGatherArgs {
  const uint8_t *text; const int64_t *nl; const int64_t *doff; int64_t n; int32_t which;
  uint8_t *dst; int64_t gbase, total, g0, ntiles;            // g0: gbase rounded down to a 16-byte group
};

// the last record of [lo, hi) that starts at or before byte o of the plane (doff[lo] <= o): it holds o when o is below the total, because
// a record of no bytes starts where its successor starts and so is never the last
__device__ __forceinline__ int64_t fastq_find(const int64_t *__restrict__ doff, int64_t lo, int64_t hi, int64_t o)
{
  while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (doff[mid] <= o) lo = mid; else hi = mid; }
  return lo;
}
// where line `which` of record r starts in the text
__device__ __forceinline__ int64_t fastq_src(const FastqGatherArgs &a, int64_t r)
{
  const int64_t k = 4 * r + a.which;
  return k > 0 ? a.nl[k - 1] + 1 : 0;
}

__global__ __launch_bounds__(FG_BLOCK) void k_fastq_gather(FastqGatherArgs a)
{
  const int64_t gend = a.gbase + a.total;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t G0 = a.g0 + tile * FG_TILE, G1 = G0 + FG_TILE < gend ? G0 + FG_TILE : gend;
    const int64_t olo = (G0 > a.gbase ? G0 : a.gbase) - a.gbase, ohi = G1 - a.gbase;      // this tile's bytes of the plane: [olo, ohi), never empty
    const int64_t rlo = fastq_find(a.doff, 0, a.n, olo), rhi = fastq_find(a.doff, rlo, a.n, ohi - 1);      // the same in every lane
#pragma unroll
    for (int j = 0; j < FG_ITEMS; j++) {
      const int64_t G = G0 + ((int64_t)j * FG_BLOCK + threadIdx.x) * 16;
      if (G >= G1) break;
      const int64_t o = G - a.gbase;                                  // (below 0 in the first group where gbase is no multiple of 16)
      const int64_t b0 = o > 0 ? o : 0, b1 = o + 16 < a.total ? o + 16 : a.total;
      int64_t r = fastq_find(a.doff, rlo, rhi + 1, b0);
      int64_t d0 = a.doff[r], next = a.doff[r + 1];
      if (o >= 0 && o + 16 <= a.total && o + 16 <= next) {            // 16 bytes of one line: five aligned dwords hold them
        const uint8_t *p = a.text + fastq_src(a, r) + (o - d0);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3);
        const unsigned sh = 8 * (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
        uint4 v;
        v.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
        v.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
        v.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
        v.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> sh);
        *reinterpret_cast<uint4 *>(a.dst + G) = v;
      } else {                                                        // a seam between records, or an end of the plane's new bytes
        int64_t s0 = fastq_src(a, r);
        for (int64_t b = b0; b < b1; b++) {
          while (b >= next) { r++; d0 = next; next = a.doff[r + 1]; s0 = fastq_src(a, r); }
          a.dst[a.gbase + b] = a.text[s0 + (b - d0)];
        }
      }
    }
  }
}

void launch_fastq_gather(const uint8_t *text, const int64_t *nl, const int64_t *doff, int64_t n, int which, uint8_t *dst, int64_t gbase, int64_t total, hipStream_t st)
{
  if (total <= 0 || n <= 0) return;
  FastqGatherArgs a;
  a.text = text; a.nl = nl; a.doff = doff; a.n = n; a.which = which; a.dst = dst; a.gbase = gbase; a.total = total;
  a.g0 = gbase & ~(int64_t)15;
  a.ntiles = (gbase + total - a.g0 + FG_TILE - 1) / FG_TILE;
  const unsigned grid = (unsigned)std::min<int64_t>(a.ntiles, 256 * 8);
  hipLaunchKernelGGL(k_fastq_gather, dim3(grid), dim3(FG_BLOCK), 0, st, a);
}

// ---- the pass over a pair's planes -----------------------------------------------------------------------------------------------
// OUTPUT-stationary like the gather: a lane owns 16 aligned bytes of a plane, four dwords through fastq_rec.h's byte-parallel routines,
// and stores them only where upper-casing changed one.  A plane starts at an allocation's first byte, so only its last group can be
// partial: that one goes byte by byte, and nothing at or past `total` is read or written.  Then the pairs: fl + rl from the two offset
// arrays, the block's maximum through one atomicMax.  The flags of a wave are folded with shuffles into one atomicOr at most.
constexpr int FQP_BLOCK = 256;

__global__ __launch_bounds__(FQP_BLOCK) void k_fastq_pairs(FastqPairArgs a)
{
  const int64_t t0 = (int64_t)blockIdx.x * FQP_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * FQP_BLOCK;
  uint32_t flags = 0;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    uint8_t *seq = a.seq[s]; const uint8_t *qual = a.qual[s];
    const int64_t total = a.total[s], groups = (total + 15) >> 4;
    for (int64_t g = t0; g < groups; g += stride) {
      const int64_t p = g << 4;
      if (p + 16 <= total) {
        const uint4 v = *reinterpret_cast<const uint4 *>(seq + p), q = *reinterpret_cast<const uint4 *>(qual + p);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
        if (fq_upper16(w)) { *reinterpret_cast<uint4 *>(seq + p) = make_uint4(w[0], w[1], w[2], w[3]); flags |= (uint32_t)FQ_PAIR_LOWER1 << s; }
        if (!fq_qual_ok16(qw)) flags |= (uint32_t)FQ_PAIR_QUAL1 << s;
      } else {
        for (int64_t b = p; b < total; b++) {
          const uint8_t c = seq[b], u = fq_upper1(c);
          if (u != c) { seq[b] = u; flags |= (uint32_t)FQ_PAIR_LOWER1 << s; }
          if (!fq_qual_ok1(qual[b])) flags |= (uint32_t)FQ_PAIR_QUAL1 << s;
        }
      }
    }
  }
  int64_t longest = 0;
  for (int64_t i = t0; i < a.n; i += stride) {
    const int64_t t = (a.off[0][i + 1] - a.off[0][i]) + (a.off[1][i + 1] - a.off[1][i]);
    longest = t > longest ? t : longest;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    flags |= (uint32_t)__shfl_xor((int)flags, d, 64);
    const int64_t o = __shfl_xor(longest, d, 64);
    longest = o > longest ? o : longest;
  }
  __shared__ int64_t part[FQP_BLOCK / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    part[wid] = longest;
    if (flags) atomicOr(a.info, (unsigned long long)flags);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < FQP_BLOCK / 64; w++) longest = part[w] > longest ? part[w] : longest;
    if (longest > 0) atomicMax(a.info + 1, (unsigned long long)longest);
  }
}

void launch_fastq_pairs(const FastqPairArgs &a, hipStream_t st)
{
  (void)hipMemsetAsync(a.info, 0, 2 * sizeof(unsigned long long), st);
  const int64_t items = std::max(std::max((a.total[0] + 15) >> 4, (a.total[1] + 15) >> 4), a.n);
  if (items <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((items + FQP_BLOCK - 1) / FQP_BLOCK, 256 * 8);
  hipLaunchKernelGGL(k_fastq_pairs, dim3(grid), dim3(FQP_BLOCK), 0, st, a);
}

}  // namespace itsx
