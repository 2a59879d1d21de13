// k_deflate.hip -- gzip members made on the device (the batch writers' compression == 3, itsx_deflate_device).
// One workgroup per block of at most DF_B bytes of text; every block becomes one independent gzip member (10-byte header, deflate
// data, CRC-32, ISIZE), so a file is its blocks' members one after another, as the host writers' files are (fastq_io.h).
// Per block, with the whole text of the block in LDS:
//   1. CRC-32: every thread the table CRC of its 64 bytes, joined in thread order by "append k zero bytes" (deflate_codes.h).
//   2. LZ77: tiles of DF_BLOCK positions.  A position hashes its 4 bytes into an LDS table of latest positions and measures the
//      match against what EARLIER tiles left there (so no candidate depends on the order of this tile's insertions, and the table
//      itself is filled with atomicMax: the same bytes every run).  No candidate is more than 32768 back or before the block.
//      Wave 0 then walks the tile greedily -- 64 positions a step: literals up to the first position that has a match, the match,
//      on from its end -- and appends the tokens to the workgroup's slot of global scratch; the walk carries the next uncovered
//      position from tile to tile.
//   3. Dynamic Huffman codes: symbol counts with LDS atomic adds, the used symbols ranked in parallel, then one lane runs
//      deflate_codes.h (lengths limited to 15 / 7 bits, canonical codes, the run-length coded header).
//   4. Bits: every thread sums the bit lengths of its run of tokens, one block scan turns the sums into bit offsets, and the codes are
//      ORed into the LDS image of the output (the text's own LDS, no longer needed) with LDS atomics; the image leaves as dwords.
//   5. A stored block (BTYPE 0) instead whenever that is not larger: a member never exceeds len + 5 + 18 bytes.
// k_deflate_pack then moves the members of a wave of blocks from their worst-case slots to where the offsets say (64-bit).
#include "k_api.h"
#include "k_scan.h"
#include "deflate_codes.h"

#include <algorithm>

namespace itsx {

using namespace itsx_dc;

constexpr int DF_BLOCK = 1024;                   // threads of a workgroup = positions of a tile
constexpr int DF_B = DEFLATE_BLOCK_BYTES;
constexpr int DF_HASH_BITS = 13;
constexpr int DF_MIN_MATCH = 4;                  // what the 4-byte hash can find
constexpr int DF_LEAD = 2;                       // a member starts here in its slot, so that its deflate data (10 bytes on) is dword aligned
constexpr int DF_TEXT = 64 * DF_BLOCK;           // bytes of the LDS text: a thread's CRC piece is 64 bytes
static_assert(DF_B <= DF_TEXT && DF_B <= 65535 && DF_TEXT <= DEFLATE_TOKEN_SLOT, "a block fits the LDS text and one stored block");
static_assert(DEFLATE_SLOT_BYTES % 4 == 0 && DEFLATE_SLOT_BYTES >= DF_LEAD + DF_B + 5 + 18, "a slot holds the stored form of a full block");

struct DeflateShared {
  uint32_t text[DF_TEXT / 4];                     // the block's text; from step 4 on the image of the deflate data
  uint32_t hash[1 << DF_HASH_BITS];              // latest position + 1 of a hash value, 0 = none
  uint16_t mlen[DF_BLOCK], mdist[DF_BLOCK];      // the tile's matches
  uint32_t fl[MAX_SYMS], fd[32];                 // symbol counts
  uint8_t lll[MAX_SYMS], dl[32];                 // code lengths
  uint16_t llc[MAX_SYMS], dc[32];                // codes, reversed
  uint32_t work[WORK_WORDS];
  uint32_t crc[DF_BLOCK], crctab[256], xp[CRC_POWERS];
  DcHeader hdr;
  int ntok, next, nused;
};

__device__ __forceinline__ uint32_t df_load4(const uint32_t *t, int p)        // the 4 bytes at byte p of an LDS text
{
  const int w = p >> 2, s = (p & 3) * 8;
  const uint32_t lo = t[w];
  if (s == 0) return lo;
  return (lo >> s) | (t[w + 1] << (32 - s));
}
__device__ __forceinline__ void df_put(uint32_t *img, uint32_t off, uint32_t val, int nb)
{
  if (nb == 0) return;
  const uint64_t v = (uint64_t)val << (off & 31);
  atomicOr(&img[off >> 5], (uint32_t)v);
  if (v >> 32) atomicOr(&img[(off >> 5) + 1], (uint32_t)(v >> 32));
}
// a token: a literal byte, or 1 << 31 | (distance - 1) << 8 | (length - 3)
__device__ __forceinline__ uint32_t df_token_bits(const DeflateShared &sh, uint32_t t)
{
  if (!(t >> 31)) return sh.lll[t];
  int eb, eb2; uint32_t ev;
  const int ls = dc_length_symbol((int)(t & 255u) + 3, &eb, &ev), ds = dc_distance_symbol((int)((t >> 8) & 32767u) + 1, &eb2, &ev);
  return (uint32_t)sh.lll[ls] + (uint32_t)eb + (uint32_t)sh.dl[ds] + (uint32_t)eb2;
}
// the used symbols of freq[0..n) in order of (count, symbol) into work + 4 n, in parallel: a symbol's place is the number of used
// symbols before it in that order (what dc_sort_symbols leaves)
__device__ void df_rank_symbols(const uint32_t *freq, int n, uint32_t *work, int *nused)
{
  const int i = threadIdx.x;
  if (i < n && freq[i]) {
    const uint32_t f = freq[i];
    int r = 0;
    for (int k = 0; k < n; k++) { const uint32_t g = freq[k]; r += g != 0 && (g < f || (g == f && k < i)); }
    work[4 * n + r] = (uint32_t)i;
    atomicAdd(nused, 1);
  }
}

__global__ __launch_bounds__(DF_BLOCK) void k_deflate(DeflateArgs a)
{
  __shared__ DeflateShared sh;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid < 256) sh.crctab[tid] = dc_crc_table_entry((uint32_t)tid);
  if (tid == 256) dc_crc_powers(sh.xp);
  uint32_t *tok = a.tokens + (size_t)blockIdx.x * DEFLATE_TOKEN_SLOT;
  const uint8_t *textb = reinterpret_cast<const uint8_t *>(sh.text);
  for (int b = blockIdx.x; b < a.nblk; b += gridDim.x) {
    __syncthreads();
    const DeflateBlock d = a.blk[b];
    const int n = d.len;
    uint8_t *slot = a.slots + (size_t)b * DEFLATE_SLOT_BYTES;
    uint8_t *mem = slot + DF_LEAD;                                           // the member; its deflate data at mem + 10
    if (n == 0) {                                                            // an empty text: one empty fixed-code block
      if (tid == 0) {
        const uint8_t e[20] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 20; k++) mem[k] = e[k];
        a.sizes[b] = 20;
      }
      continue;
    }
    // ---- the text into LDS: aligned dwords of the source, shifted to the block's first byte; bytes past its end are 0
    {
      const uint8_t *src = a.text + d.src;
      const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
      const uint32_t *src4 = reinterpret_cast<const uint32_t *>(src - mis);
      const int nw = (n + 3) >> 2;
      for (int i = tid; i < nw; i += DF_BLOCK) {
        uint32_t v = src4[i];
        if (mis) v = (v >> (8 * mis)) | (src4[i + 1] << (32 - 8 * mis));
        const int left = n - 4 * i;
        if (left < 4) v &= (1u << (8 * left)) - 1;
        sh.text[i] = v;
      }
    }
    for (int i = tid; i < (1 << DF_HASH_BITS); i += DF_BLOCK) sh.hash[i] = 0;
    if (tid < MAX_SYMS) sh.fl[tid] = tid == 256 ? 1u : 0u;
    if (tid < 32) sh.fd[tid] = 0;
    if (tid == 0) { sh.ntok = 0; sh.next = 0; }
    __syncthreads();
    // ---- 1. CRC-32
    {
      uint32_t c = 0xffffffffu;
      const int left = n - 64 * tid;
      for (int j = 0; j < 16 && 4 * j < left; j++) {
        uint32_t v = sh.text[16 * tid + j];
        const int nb = left - 4 * j < 4 ? left - 4 * j : 4;
        for (int k = 0; k < nb; k++) { c = sh.crctab[(c ^ v) & 255u] ^ (c >> 8); v >>= 8; }
      }
      sh.crc[tid] = ~c;                                                      // a piece of no bytes: 0
    }
    __syncthreads();
    for (int s = 1; s < DF_BLOCK; s <<= 1) {
      if ((tid & (2 * s - 1)) == 0) {
        int rl = n - 64 * (tid + s);                                         // bytes of the pieces tid + s .. tid + 2 s - 1
        rl = rl < 0 ? 0 : rl > 64 * s ? 64 * s : rl;
        if (rl > 0) sh.crc[tid] = dc_crc_append(sh.xp, sh.crc[tid], sh.crc[tid + s], (uint32_t)rl);
      }
      __syncthreads();
    }
    const uint32_t crc = sh.crc[0];
    // ---- 2. matches and the greedy parse, tile by tile
    for (int t0 = 0; t0 < n; t0 += DF_BLOCK) {
      const int p = t0 + tid;
      const bool can = p + 4 <= n;
      uint32_t h = 0;
      int ml = 0, md = 0;
      if (can) {
        h = (df_load4(sh.text, p) * 2654435761u) >> (32 - DF_HASH_BITS);
        const int c = (int)sh.hash[h] - 1;                                   // from an earlier tile, so c < t0 <= p
        if (c >= 0 && p - c <= 32768) {
          const int maxl = n - p < 258 ? n - p : 258;
          int l = 0;
          bool open = true;
          while (open && l + 4 <= maxl) {
            const uint32_t x = df_load4(sh.text, p + l) ^ df_load4(sh.text, c + l);
            if (x) { l += (__ffs((int)x) - 1) >> 3; open = false; } else l += 4;
          }
          while (open && l < maxl && textb[p + l] == textb[c + l]) l++;
          if (l >= DF_MIN_MATCH) { ml = l; md = p - c; }
        }
      }
      sh.mlen[tid] = (uint16_t)ml; sh.mdist[tid] = (uint16_t)(md - 1);
      __syncthreads();
      if (can) atomicMax(&sh.hash[h], (uint32_t)(p + 1));
      if (wid == 0) {
        const int tend = t0 + DF_BLOCK < n ? t0 + DF_BLOCK : n;
        int pos = sh.next, nt = sh.ntok;
        if (pos < t0) pos = t0;
        while (pos < tend) {
          const int q = pos + lane;
          const int l = q < tend ? (int)sh.mlen[q - t0] : 0;
          const unsigned long long m = __ballot(l >= DF_MIN_MATCH);
          if (m) {
            const int k = __ffsll((long long)m) - 1;
            if (lane < k) tok[nt + lane] = textb[q];
            if (lane == k) tok[nt + k] = 0x80000000u | ((uint32_t)sh.mdist[q - t0] << 8) | (uint32_t)(l - 3);
            nt += k + 1; pos += k + __shfl(l, k, 64);
          } else {
            const int nl = tend - pos < 64 ? tend - pos : 64;
            if (lane < nl) tok[nt + lane] = textb[q];
            nt += nl; pos += nl;
          }
        }
        if (lane == 0) { sh.next = pos; sh.ntok = nt; }
      }
      __syncthreads();
    }
    const int ntok = sh.ntok;
    // ---- 3. the codes
    for (int i = tid; i < ntok; i += DF_BLOCK) {
      const uint32_t t = tok[i];
      if (t >> 31) {
        int eb; uint32_t ev;
        atomicAdd(&sh.fl[dc_length_symbol((int)(t & 255u) + 3, &eb, &ev)], 1u);
        atomicAdd(&sh.fd[dc_distance_symbol((int)((t >> 8) & 32767u) + 1, &eb, &ev)], 1u);
      } else atomicAdd(&sh.fl[t], 1u);
    }
    if (tid == 0) sh.nused = 0;
    __syncthreads();
    if (tid == 0) dc_at_least_two(sh.fd, NDIST);
    df_rank_symbols(sh.fl, NLL, sh.work, &sh.nused);
    __syncthreads();
    if (tid == 0) { dc_lengths_from_sorted(sh.fl, NLL, 15, sh.lll, sh.work, sh.nused); dc_canonical_codes(sh.lll, NLL, sh.llc); sh.nused = 0; }
    __syncthreads();
    df_rank_symbols(sh.fd, NDIST, sh.work, &sh.nused);
    __syncthreads();
    if (tid == 0) {
      dc_lengths_from_sorted(sh.fd, NDIST, 15, sh.dl, sh.work, sh.nused); dc_canonical_codes(sh.dl, NDIST, sh.dc);
      dc_build_header(sh.lll, sh.dl, &sh.hdr, sh.work);
    }
    __syncthreads();
    // ---- 4. bit offsets: thread t owns tokens [t per, (t + 1) per)
    const int per = (ntok + DF_BLOCK - 1) / DF_BLOCK;
    const int i0 = tid * per < ntok ? tid * per : ntok, i1 = i0 + per < ntok ? i0 + per : ntok;
    int64_t v[1] = {0}, ex[1], tot[1];
    for (int i = i0; i < i1; i++) v[0] += df_token_bits(sh, tok[i]);
    block_scan64<1, DF_BLOCK>(v, ex, tot);
    const uint32_t head = 3 + sh.hdr.bits;
    const int64_t dynbits = (int64_t)head + tot[0] + sh.lll[256];
    const int dyn = (int)((dynbits + 7) >> 3), stored = n + 5;
    int payload;
    if (stored <= dyn || dyn > DF_TEXT) {
      // ---- 5. one stored block, straight from the text in LDS
      payload = stored;
      for (int i = tid; i < stored; i += DF_BLOCK) {
        uint8_t x;
        if (i == 0) x = 1;                                                   // BFINAL, BTYPE 0
        else if (i == 1) x = (uint8_t)n;
        else if (i == 2) x = (uint8_t)(n >> 8);
        else if (i == 3) x = (uint8_t)~n;
        else if (i == 4) x = (uint8_t)(~n >> 8);
        else x = textb[i - 5];
        mem[10 + i] = x;
      }
    } else {
      payload = dyn;
      __syncthreads();                                                       // the text has been read for the last time
      const int nw = (dyn + 3) >> 2;
      for (int i = tid; i < nw; i += DF_BLOCK) sh.text[i] = 0;
      __syncthreads();
      if (tid == 0) {
        const DcHeader &hd = sh.hdr;
        uint32_t o = 0;
        df_put(sh.text, o, 1u | (2u << 1), 3); o += 3;                        // BFINAL, BTYPE 2
        df_put(sh.text, o, (uint32_t)(hd.hlit - 257), 5); o += 5;
        df_put(sh.text, o, (uint32_t)(hd.hdist - 1), 5); o += 5;
        df_put(sh.text, o, (uint32_t)(hd.hclen - 4), 4); o += 4;
        for (int k = 0; k < hd.hclen; k++) { df_put(sh.text, o, hd.cl_len[dc_cl_order(k)], 3); o += 3; }
        for (int k = 0; k < hd.nsym; k++) {
          const int s = hd.sym[k], xb = dc_cl_extra_bits(s);
          df_put(sh.text, o, hd.cl_code[s], hd.cl_len[s]); o += hd.cl_len[s];
          df_put(sh.text, o, hd.ext[k], xb); o += (uint32_t)xb;
        }
        df_put(sh.text, head + (uint32_t)tot[0], sh.llc[256], sh.lll[256]);   // end of block
      }
      uint32_t o = head + (uint32_t)ex[0];
      for (int i = i0; i < i1; i++) {
        const uint32_t t = tok[i];
        if (t >> 31) {
          int eb; uint32_t ev;
          int s = dc_length_symbol((int)(t & 255u) + 3, &eb, &ev);
          df_put(sh.text, o, (uint32_t)sh.llc[s] | (ev << sh.lll[s]), sh.lll[s] + eb); o += (uint32_t)(sh.lll[s] + eb);
          s = dc_distance_symbol((int)((t >> 8) & 32767u) + 1, &eb, &ev);
          df_put(sh.text, o, (uint32_t)sh.dc[s] | (ev << sh.dl[s]), sh.dl[s] + eb); o += (uint32_t)(sh.dl[s] + eb);
        } else { df_put(sh.text, o, sh.llc[t], sh.lll[t]); o += sh.lll[t]; }
      }
      __syncthreads();
      uint32_t *out4 = reinterpret_cast<uint32_t *>(mem + 10);               // slot + 12: aligned
      for (int i = tid; i < (dyn >> 2); i += DF_BLOCK) out4[i] = sh.text[i];
      if (tid == 0) for (int i = dyn & ~3; i < dyn; i++) mem[10 + i] = textb[i];
    }
    if (tid == 0) {
      const uint8_t g[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 0xff};         // no name, no time, OS unknown
      for (int k = 0; k < 10; k++) mem[k] = g[k];
      uint8_t *tr = mem + 10 + payload;
      for (int k = 0; k < 4; k++) { tr[k] = (uint8_t)(crc >> (8 * k)); tr[4 + k] = (uint8_t)((uint32_t)n >> (8 * k)); }
      a.sizes[b] = 18 + payload;
    }
  }
}

__global__ __launch_bounds__(256) void k_deflate_pack(const uint8_t *__restrict__ slots, const int32_t *__restrict__ sizes, const int64_t *__restrict__ dst,
                                                      int32_t nblk, uint8_t *__restrict__ out)
{
  for (int b = blockIdx.x; b < nblk; b += gridDim.x) {
    const uint8_t *src = slots + (size_t)b * DEFLATE_SLOT_BYTES + DF_LEAD;
    uint8_t *to = out + dst[b];
    const int n = sizes[b];
    for (int i = threadIdx.x; i < n; i += 256) to[i] = src[i];
  }
}

void launch_deflate(const DeflateArgs &a, int grid, hipStream_t st)
{
  if (a.nblk <= 0) return;
  hipLaunchKernelGGL(k_deflate, dim3((unsigned)std::max(1, std::min(grid, a.nblk))), dim3(DF_BLOCK), 0, st, a);
}

void launch_deflate_pack(const uint8_t *slots, const int32_t *sizes, const int64_t *dst, int32_t nblk, uint8_t *out, hipStream_t st)
{
  if (nblk <= 0) return;
  hipLaunchKernelGGL(k_deflate_pack, dim3((unsigned)std::min(nblk, 4096)), dim3(256), 0, st, slots, sizes, dst, nblk, out);
}

}  // namespace itsx
