// deflate_codes.h -- the code-construction arithmetic of the device deflate (k_deflate.hip), as __host__ __device__ functions so that
// the CPU tests and the stand-alone check (scripts/deflate_codes_check.cpp) run the very code one lane of the kernel runs per block:
// length-limited Huffman code lengths, canonical code assignment (bit-reversed, DEFLATE emits codes MSB first into an LSB-first stream),
// the run-length coded code-length header of a dynamic block (RFC 1951 section 3.2.7), the length / distance symbol maps, and the
// arithmetic that joins the CRC-32s of a member's pieces.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DC_HD __host__ __device__ inline
#else
#define DC_HD inline
#endif

namespace itsx_dc {

constexpr int NLL = 286, NDIST = 30, NCL = 19;     // the three alphabets
constexpr int MAX_SYMS = 288;                      // dc_huffman_lengths takes up to this many symbols ...
constexpr int WORK_WORDS = 5 * MAX_SYMS;           // ... and this many words of scratch
constexpr int MAX_HDR = NLL + NDIST;               // code-length symbols of one header at most (no run: one per length)

// ---- length-limited Huffman code lengths.  len[i] = 0 where freq[i] = 0; one used symbol gets length 1; otherwise a complete code
// (Kraft sum exactly 1) with no length above maxbits, and the unlimited Huffman code itself whenever that already fits.
// dc_sort_symbols puts the used symbols in order of (frequency, symbol); dc_lengths_from_sorted builds the tree from that order with
// two queues (leaves, and inner nodes in the order they were made: both non-decreasing), so the lengths are a function of the
// frequencies alone.  A tree that is too deep is clamped to maxbits and repaired on its Kraft sum K (scaled by 2^maxbits): lengthen
// the cheapest symbol of the greatest length below maxbits until K <= 2^maxbits, then shorten symbols, the largest step that fits
// first, until K = 2^maxbits.  (Every K is a multiple of the smallest step on offer, so the second loop ends exactly; it asks
// n <= 2^maxbits.)  The frequencies must sum below 2^32.  work: WORK_WORDS words (5 n are used); order = work + 4 n.
DC_HD int dc_sort_symbols(const uint32_t *freq, int n, uint32_t *order)
{
  int m = 0;
  for (int i = 0; i < n; i++) if (freq[i]) {
    int k = m++;
    while (k > 0 && freq[order[k - 1]] > freq[i]) { order[k] = order[k - 1]; k--; }      // equal counts keep symbol order
    order[k] = (uint32_t)i;
  }
  return m;
}
DC_HD void dc_lengths_from_sorted(const uint32_t *freq, int n, int maxbits, uint8_t *len, uint32_t *work, int m)
{
  uint32_t *w = work, *parent = work + 2 * n;
  const uint32_t *order = work + 4 * n;
  for (int i = 0; i < n; i++) len[i] = 0;
  if (m == 0) return;
  if (m == 1) { len[order[0]] = 1; return; }
  for (int k = 0; k < m; k++) w[k] = freq[order[k]];                     // nodes 0..m-1: the leaves in order, m..2m-2: inner nodes
  int i = 0, j = m, next = m;
  while (next < 2 * m - 1) {
    uint32_t sum = 0;
    for (int t = 0; t < 2; t++) {
      const bool leaf = i < m && (j >= next || w[i] <= w[j]);
      const int pick = leaf ? i++ : j++;
      sum += w[pick]; parent[pick] = (uint32_t)next;
    }
    w[next++] = sum;
  }
  const int root = next - 1;
  w[root] = 0;                                                           // from here w[inner node] = its depth
  for (int k = root - 1; k >= m; k--) w[k] = w[parent[k]] + 1;
  bool deep = false;
  for (int k = 0; k < m; k++) {
    uint32_t d = w[parent[k]] + 1;
    if (d > (uint32_t)maxbits) { d = (uint32_t)maxbits; deep = true; }
    len[order[k]] = (uint8_t)d;
  }
  if (!deep) return;
  const uint32_t one = 1u << maxbits;
  uint32_t K = 0;
  for (int s = 0; s < n; s++) if (len[s]) K += one >> len[s];
  while (K > one) {
    int pick = -1;
    for (int s = 0; s < n; s++) if (len[s] && len[s] < maxbits)
      if (pick < 0 || len[s] > len[pick] || (len[s] == len[pick] && freq[s] <= freq[pick])) pick = s;
    if (pick < 0) return;                                                // n > 2^maxbits: not a case this is asked for
    len[pick]++; K -= one >> len[pick];
  }
  while (K < one) {
    const uint32_t room = one - K;
    int pick = -1;
    for (int s = 0; s < n; s++) if (len[s] >= 2 && (one >> len[s]) <= room)
      if (pick < 0 || len[s] < len[pick] || (len[s] == len[pick] && freq[s] > freq[pick])) pick = s;
    if (pick < 0) return;
    K += one >> len[pick]; len[pick]--;
  }
}
DC_HD void dc_huffman_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *len, uint32_t *work)
{
  const int m = dc_sort_symbols(freq, n, work + 4 * n);
  dc_lengths_from_sorted(freq, n, maxbits, len, work, m);
}

// A decoder need not take a code with fewer than two codewords (zlib takes it for distances only): give a spare symbol a count.
DC_HD void dc_at_least_two(uint32_t *freq, int n)
{
  int used = 0;
  for (int i = 0; i < n; i++) used += freq[i] != 0;
  for (int i = 0; i < n && used < 2; i++) if (!freq[i]) { freq[i] = 1; used++; }
}

// ---- canonical codes from lengths (RFC 1951 3.2.2), each reversed over its length: ready to be ORed into an LSB-first bit stream
DC_HD void dc_canonical_codes(const uint8_t *len, int n, uint16_t *code)
{
  uint32_t count[16], nextc[16];
  for (int b = 0; b < 16; b++) count[b] = 0;
  for (int i = 0; i < n; i++) count[len[i]]++;
  count[0] = 0;
  uint32_t c = 0;
  nextc[0] = 0;
  for (int b = 1; b < 16; b++) { c = (c + count[b - 1]) << 1; nextc[b] = c; }
  for (int i = 0; i < n; i++) {
    const int l = len[i];
    uint32_t v = 0;
    if (l) {
      const uint32_t w = nextc[l]++;
      for (int b = 0; b < l; b++) v |= ((w >> b) & 1u) << (l - 1 - b);
    }
    code[i] = (uint16_t)v;
  }
}

// ---- the symbol maps: a match length 3..258 and a distance 1..32768 as (symbol, number of extra bits, their value)
DC_HD int dc_length_symbol(int mlen, int *ebits, uint32_t *eval)
{
  const uint32_t l = (uint32_t)(mlen - 3);
  if (l == 255) { *ebits = 0; *eval = 0; return 285; }
  int e = 0;
  if (l >= 8) { int hb = 3; while ((l >> (hb + 1)) != 0) hb++; e = hb - 2; }
  *ebits = e; *eval = l & ((1u << e) - 1);
  return 257 + 4 * e + (int)(l >> e);
}
DC_HD int dc_distance_symbol(int dist, int *ebits, uint32_t *eval)
{
  const uint32_t d = (uint32_t)(dist - 1);
  if (d < 4) { *ebits = 0; *eval = 0; return (int)d; }
  int hb = 2; while ((d >> (hb + 1)) != 0) hb++;
  const int e = hb - 1;
  *ebits = e; *eval = d & ((1u << e) - 1);
  return 2 * e + 2 + (int)((d >> e) & 1u);
}

// ---- the header of a dynamic block after its three BFINAL/BTYPE bits: HLIT, HDIST, HCLEN, the code-length code's lengths in the
// order below, then the hlit + hdist code lengths as one run-length coded sequence (16: the last length 3..6 times again, 17: 3..10
// zeros, 18: 11..138 zeros; a run may cross from the literal/length lengths into the distance lengths).
struct DcHeader {
  int hlit, hdist, hclen, nsym;            // symbols in ll_len / d_len that are sent, code-length code lengths sent, entries of sym[]
  uint32_t bits;                           // the header's length in bits
  uint8_t sym[MAX_HDR], ext[MAX_HDR];      // the code-length symbols in order and the value of each one's extra bits
  uint8_t cl_len[NCL]; uint16_t cl_code[NCL];
};
DC_HD int dc_cl_order(int k)
{
  const uint8_t order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[k];
}
DC_HD int dc_cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
DC_HD void dc_build_header(const uint8_t *ll_len, const uint8_t *d_len, DcHeader *h, uint32_t *work)
{
  int hlit = NLL, hdist = NDIST;
  while (hlit > 257 && ll_len[hlit - 1] == 0) hlit--;
  while (hdist > 1 && d_len[hdist - 1] == 0) hdist--;
  h->hlit = hlit; h->hdist = hdist;
  const int total = hlit + hdist;
  uint32_t clf[NCL];
  for (int k = 0; k < NCL; k++) clf[k] = 0;
  int ns = 0, i = 0;
  while (i < total) {
    const int v = i < hlit ? ll_len[i] : d_len[i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? ll_len[i + run] : d_len[i + run - hlit]) == v) run++;
    int left = run;
    if (v == 0) {
      while (left >= 11) { const int r = left < 138 ? left : 138; h->sym[ns] = 18; h->ext[ns++] = (uint8_t)(r - 11); clf[18]++; left -= r; }
      if (left >= 3) { h->sym[ns] = 17; h->ext[ns++] = (uint8_t)(left - 3); clf[17]++; left = 0; }
    } else {
      h->sym[ns] = (uint8_t)v; h->ext[ns++] = 0; clf[v]++; left--;
      while (left >= 3) { const int r = left < 6 ? left : 6; h->sym[ns] = 16; h->ext[ns++] = (uint8_t)(r - 3); clf[16]++; left -= r; }
    }
    while (left > 0) { h->sym[ns] = (uint8_t)v; h->ext[ns++] = 0; clf[v]++; left--; }
    i += run;
  }
  h->nsym = ns;
  dc_at_least_two(clf, NCL);
  dc_huffman_lengths(clf, NCL, 7, h->cl_len, work);
  dc_canonical_codes(h->cl_len, NCL, h->cl_code);
  int hclen = NCL;
  while (hclen > 4 && h->cl_len[dc_cl_order(hclen - 1)] == 0) hclen--;
  h->hclen = hclen;
  uint32_t bits = 5 + 5 + 4 + 3 * (uint32_t)hclen;
  for (int k = 0; k < ns; k++) bits += (uint32_t)h->cl_len[h->sym[k]] + (uint32_t)dc_cl_extra_bits(h->sym[k]);
  h->bits = bits;
}

// ---- CRC-32 (the gzip one, reflected polynomial 0xEDB88320) of a text from the CRCs of its pieces: with the polynomials kept as the
// CRC register keeps them (bit 31 = x^0), crc(A B) = crc(A) * x^(8 |B|) + crc(B) mod P -- the initial and final inversions cancel.
DC_HD uint32_t dc_gf2_mulmod(uint32_t a, uint32_t b)
{
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
  }
  return p;
}
constexpr int CRC_POWERS = 18;
DC_HD void dc_crc_powers(uint32_t *xp)              // xp[k] = x^(8 * 2^k) mod P: the operator "append 2^k zero bytes"
{
  xp[0] = 0x00800000u;
  for (int k = 1; k < CRC_POWERS; k++) xp[k] = dc_gf2_mulmod(xp[k - 1], xp[k - 1]);
}
DC_HD uint32_t dc_crc_append(const uint32_t *xp, uint32_t crc_a, uint32_t crc_b, uint32_t len_b)     // len_b < 2^CRC_POWERS
{
  for (int k = 0; len_b; k++, len_b >>= 1) if (len_b & 1u) crc_a = dc_gf2_mulmod(xp[k], crc_a);
  return crc_a ^ crc_b;
}
DC_HD uint32_t dc_crc_table_entry(uint32_t i) { for (int k = 0; k < 8; k++) i = (i >> 1) ^ ((i & 1u) ? 0xEDB88320u : 0u); return i; }

}  // namespace itsx_dc
