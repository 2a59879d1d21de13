// inflate_codes.h -- the decoder's logic of the device inflate (k_inflate.hip), as __host__ __device__ functions so that the CPU tests
// and the stand-alone sanitizer program (tests/csrc/inflate_asan.cpp) run the very code one lane of the kernel runs per member: the
// gzip header parse, the strict member-start candidate test, canonical decode tables from code lengths, the code-length alphabet of a
// dynamic block (RFC 1951 section 3.2.7), a resumable token decoder over stored, fixed and dynamic blocks, the trailer check, and one
// serial routine that inflates one member with them.  No allocation; every refusal is a reason code, nothing is clamped.
// Byte order: the bit reader loads 8 input bytes as one little-endian word (x86-64 and gfx950 both are).
#pragma once
#include <stdint.h>
#include "deflate_codes.h"

namespace itsx_ic {

#define IC_HD DC_HD

enum IcReason : int32_t {
  IC_OK = 0,
  IC_E_NOT_GZIP = 1,        // no 1f 8b at the start of the span
  IC_E_HEADER = 2,          // CM != 8, a reserved FLG bit, or a header that does not end inside the span
  IC_E_FHCRC = 3,           // FHCRC present and wrong
  IC_E_BTYPE = 4,           // BTYPE 3
  IC_E_STORED = 5,          // LEN != ~NLEN
  IC_E_COUNTS = 6,          // HLIT > 286 or HDIST > 30
  IC_E_OVERSUBSCRIBED = 7,
  IC_E_INCOMPLETE = 8,
  IC_E_REPEAT = 9,          // repeat-16 with no previous length, or a repeat past HLIT + HDIST
  IC_E_NO_EOB = 10,         // symbol 256 has length 0
  IC_E_LSYMBOL = 11,        // literal/length symbol 286 or 287
  IC_E_DSYMBOL = 12,        // distance symbol 30 or 31, or bits that are no distance codeword
  IC_E_DISTANCE = 13,       // a distance larger than the bytes this member has produced
  IC_E_OUTPUT = 14,         // output beyond isize
  IC_E_INPUT = 15,          // input beyond c_end
  IC_E_TRAILER = 16,        // the deflate data does not end exactly 8 bytes before c_end
  IC_E_SHORT = 17,          // fewer than isize bytes produced
  IC_E_CRC = 18,
  IC_E_ISIZE = 19,
  IC_E_MEMBER_LONG = 20,    // the plan: a compressed span above the cap
  IC_E_EXPANSION = 21,      // the plan: more text than deflate can expand to
  IC_E_NOMEM = 22,          // the plan: the output cannot be held
  IC_E_FIRST = 23,          // the plan: position 0 is no member start
  IC_NREASONS = 24
};
inline const char *ic_reason_name(int32_t r)
{
  static const char *const names[IC_NREASONS] = {
    "ok", "not gzip", "bad gzip header", "header CRC mismatch", "block type 3", "stored LEN is not ~NLEN", "too many length or distance symbols",
    "over-subscribed code", "incomplete code", "bad repeat in the code lengths", "no code for end of block", "literal/length symbol 286 or 287",
    "invalid distance symbol", "distance beyond the member's start", "output beyond ISIZE", "input beyond the member's end",
    "deflate data does not end 8 bytes before the member's end", "fewer bytes than ISIZE", "CRC-32 mismatch", "ISIZE mismatch", "member too long",
    "more text than deflate expands to", "no memory for the text", "no member starts at byte 0"};
  return r >= 0 && r < IC_NREASONS ? names[r] : "unknown";
}

constexpr int IC_WINDOW = 32768;
constexpr int IC_RUN = 256;                 // bytes of a stored block one token carries at most
constexpr int IC_MIN_MEMBER = 10 + 2 + 8;   // header, an empty fixed block, trailer

// ---- the gzip header of a member in g[0, n): its length (the offset of the deflate data), or 0 with *why set.  FEXTRA, FNAME, FCOMMENT
// and FHCRC are skipped inside the span; FHCRC is verified.  No load outside g[0, n).
IC_HD int64_t ic_header(const uint8_t *g, int64_t n, int32_t *why)
{
  if (n < 2 || g[0] != 0x1f || g[1] != 0x8b) { *why = IC_E_NOT_GZIP; return 0; }
  *why = IC_E_HEADER;
  if (n < 10 || g[2] != 8 || (g[3] & 0xe0)) return 0;
  const int flg = g[3];
  int64_t p = 10;
  if (flg & 4) {
    if (p + 2 > n) return 0;
    p += 2 + (int64_t)(g[p] | (g[p + 1] << 8));
    if (p > n) return 0;
  }
  for (int f = 8; f <= 16; f <<= 1) if (flg & f) {                 // FNAME, FCOMMENT: zero-terminated
    for (;;) { if (p >= n) return 0; if (g[p++] == 0) break; }
  }
  if (flg & 2) {
    if (p + 2 > n) return 0;
    uint32_t c = 0xffffffffu;
    for (int64_t i = 0; i < p; i++) c = itsx_dc::dc_crc_table_entry((c ^ g[i]) & 255u) ^ (c >> 8);
    c = ~c;
    if ((c & 0xffffu) != (uint32_t)(g[p] | (g[p + 1] << 8))) { *why = IC_E_FHCRC; return 0; }
    p += 2;
  }
  *why = IC_OK;
  return p;
}

// ---- the strict member-start test of position `at` of g[0, n): 1f 8b 08, FLG's reserved bits zero, XFL 0 | 2 | 4, OS <= 13 or 255, the
// whole header (FHCRC verified) and the first block's three bits inside the buffer, and that block's BTYPE not 3
IC_HD bool ic_candidate(const uint8_t *g, int64_t n, int64_t at)
{
  if (at < 0 || at + 10 > n) return false;
  const uint8_t *h = g + at;
  if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe0)) return false;
  if (h[8] != 0 && h[8] != 2 && h[8] != 4) return false;
  if (h[9] > 13 && h[9] != 255) return false;
  int32_t why;
  const int64_t hl = ic_header(h, n - at, &why);
  if (hl == 0 || at + hl >= n) return false;
  return ((h[hl] >> 1) & 3) != 3;
}

// ---- the bit reader: a reservoir of n valid bits (LSB first) in acc (the low 64) and hi, a word of 8 input bytes that has been loaded
// but not yet joined to it (pend, when has_pend), and the next input byte *p; nothing at or past end is ever loaded.  The word is
// loaded one refill before it is joined, so that on the device the load's latency passes while the tokens before it are decoded.
struct IcBits { const uint8_t *p, *end; uint64_t acc, hi, pend; int32_t n, has_pend; };
IC_HD void ic_bits_init(IcBits &b, const uint8_t *p, const uint8_t *end) { b.p = p; b.end = end; b.acc = b.hi = b.pend = 0; b.n = 0; b.has_pend = 0; }
IC_HD void ic_join(IcBits &b, uint64_t v, int bits)          // v's low `bits` bits on top of the reservoir; n + bits <= 128
{
  if (b.n < 64) { b.acc |= v << b.n; if (b.n) b.hi |= v >> (64 - b.n); }
  else b.hi |= v << (b.n - 64);
  b.n += bits;
}
IC_HD void ic_refill(IcBits &b)              // afterwards n >= 64, or every byte of the span is in the reservoir
{
  if (b.n <= 64 && b.has_pend) { ic_join(b, b.pend, 64); b.has_pend = 0; }
  if (!b.has_pend) {
    if (b.end - b.p >= 8) { __builtin_memcpy(&b.pend, b.p, 8); b.p += 8; b.has_pend = 1; }
    else while (b.n <= 120 && b.p < b.end) ic_join(b, (uint64_t)*b.p++, 8);
  }
  if (b.n <= 64 && b.has_pend) { ic_join(b, b.pend, 64); b.has_pend = 0; }      // (the first refills of a member, and after a stored block)
}
IC_HD void ic_drop(IcBits &b, int k)         // 0 <= k <= n, k < 64
{
  if (k) { b.acc = (b.acc >> k) | (b.hi << (64 - k)); b.hi >>= k; b.n -= k; }
}
IC_HD bool ic_take(IcBits &b, int k, uint32_t *v)      // k <= 16 bits; false: the input ends first
{
  if (k > b.n) return false;
  *v = (uint32_t)b.acc & ((1u << k) - 1u);
  ic_drop(b, k);
  return true;
}
// the input position of the reservoir's first whole byte, after the bits up to the byte boundary are dropped
IC_HD const uint8_t *ic_byte_position(IcBits &b)
{
  ic_drop(b, b.n & 7);
  return b.p - (b.has_pend ? 8 : 0) - (b.n >> 3);
}

// ---- canonical decode tables: count[l] codes of length l, the symbols sorted by (length, symbol), and a first-level table over the next
// FB bits whose entry is symbol << 4 | length (0: longer than FB bits, or no codeword)
template <int NSYM, int FB> struct IcCode { uint16_t count[16]; uint16_t sorted[NSYM]; uint16_t fast[1 << FB]; };
using IcLitLen = IcCode<288, 9>;
using IcDist = IcCode<32, 6>;
using IcCl = IcCode<19, 7>;

// over-subscribed: refused.  Incomplete: refused, but for a distance code (dist) with no codeword at all (a block of literals only) or
// with a single code of length 1, which is what zlib takes.
template <int NSYM, int FB>
IC_HD int32_t ic_build(const uint8_t *len, int n, IcCode<NSYM, FB> &t, bool dist)
{
  for (int l = 0; l < 16; l++) t.count[l] = 0;
  for (int i = 0; i < n; i++) t.count[len[i]]++;
  const int used = n - t.count[0];
  int32_t left = 1;
  for (int l = 1; l < 16; l++) {
    left = (left << 1) - (int32_t)t.count[l];
    if (left < 0) return IC_E_OVERSUBSCRIBED;
  }
  if (left > 0 && !(dist && (used == 0 || (used == 1 && t.count[1] == 1)))) return IC_E_INCOMPLETE;
  uint16_t offs[16], nextc[16];
  offs[1] = 0; nextc[1] = 0;
  for (int l = 1; l < 15; l++) { offs[l + 1] = (uint16_t)(offs[l] + t.count[l]); nextc[l + 1] = (uint16_t)((nextc[l] + t.count[l]) << 1); }
  for (int k = 0; k < (1 << FB); k++) t.fast[k] = 0;
  for (int i = 0; i < n; i++) {
    const int l = len[i];
    if (!l) continue;
    t.sorted[offs[l]++] = (uint16_t)i;
    const uint32_t w = nextc[l]++;
    if (l > FB) continue;
    uint32_t r = 0;
    for (int k = 0; k < l; k++) r |= ((w >> k) & 1u) << (l - 1 - k);
    for (uint32_t k = r; k < (1u << FB); k += 1u << l) t.fast[k] = (uint16_t)((i << 4) | l);
  }
  return IC_OK;
}
// the next symbol, or -1: the bits are no codeword, -2: the input ends inside the code.  Consumes the code's bits (at least one).
template <int NSYM, int FB>
IC_HD int32_t ic_decode(IcBits &b, const IcCode<NSYM, FB> &t)
{
  const uint32_t e = t.fast[(uint32_t)b.acc & ((1u << FB) - 1u)];
  const int l = (int)(e & 15u);
  if (l) {
    if (l > b.n) return -2;
    ic_drop(b, l);
    return (int32_t)(e >> 4);
  }
  int32_t code = 0, first = 0, index = 0;
  uint64_t a = b.acc;
  for (int k = 1; k <= 15; k++) {
    if (k > b.n) return -2;
    code |= (int32_t)(a & 1u); a >>= 1;
    const int32_t c = t.count[k];
    if (code - c < first) { ic_drop(b, k); return t.sorted[index + (code - first)]; }
    index += c; first = (first + c) << 1; code <<= 1;
  }
  return -1;
}

// ---- one member's decoder.  ic_begin parses the header; ic_next yields the member's tokens one by one, reading block headers as it
// meets them; after IC_TOK_END, ic_finish checks the trailer.  A token has passed every check when it is handed out: its bytes lie inside
// [0, isize) of the member's text and its distance inside what the member has produced, so whoever executes it needs no check of its own.
enum { IC_TOK_LIT = 0, IC_TOK_MATCH = 1, IC_TOK_STORED = 2, IC_TOK_END = 3 };
struct IcToken { uint32_t kind_len; uint32_t val; };      // kind << 16 | length; the literal byte | the distance | the run's offset from c
IC_HD int ic_tok_kind(const IcToken &t) { return (int)(t.kind_len >> 16); }
IC_HD uint32_t ic_tok_len(const IcToken &t) { return t.kind_len & 0xffffu; }

// IcHot: what every token reads and writes.  The kernel's decoding lane keeps a copy in registers for a batch of tokens; the tables
// (IcDecoder, in LDS there) change only at a block's header.
struct IcHot {
  IcBits b;
  uint32_t produced, stored_left;
  int32_t mode;                 // 0: between blocks, 1: in a stored block, 2: in a coded block, 3: the final block has ended
  int32_t final;
};
struct IcDecoder {
  IcHot h;
  const uint8_t *c;
  uint32_t isize;
  IcLitLen ll; IcDist d; IcCl cl;
  uint8_t lens[288 + 32];
};

IC_HD int32_t ic_begin(IcDecoder &s, const uint8_t *c, const uint8_t *c_end, uint32_t isize)
{
  int32_t why;
  const int64_t hl = ic_header(c, c_end - c, &why);
  if (hl == 0) return why;
  ic_bits_init(s.h.b, c + hl, c_end);
  s.c = c; s.isize = isize; s.h.produced = 0; s.h.mode = 0; s.h.final = 0; s.h.stored_left = 0;
  return IC_OK;
}

// a block's header: BFINAL, BTYPE, and what the type brings (LEN / NLEN, the fixed codes, or the dynamic codes)
IC_HD int32_t ic_block(IcDecoder &s, IcHot &h)
{
  IcBits &b = h.b;
  uint32_t v;
  ic_refill(b);
  if (!ic_take(b, 3, &v)) return IC_E_INPUT;
  h.final = (int32_t)(v & 1u);
  const int btype = (int)(v >> 1);
  if (btype == 3) return IC_E_BTYPE;
  if (btype == 0) {
    ic_bits_init(b, ic_byte_position(b), b.end);           // to the byte boundary; the whole bytes held go back to the input
    if (b.end - b.p < 4) return IC_E_INPUT;
    const uint32_t len = (uint32_t)(b.p[0] | (b.p[1] << 8)), nlen = (uint32_t)(b.p[2] | (b.p[3] << 8));
    if (len != (~nlen & 0xffffu)) return IC_E_STORED;
    b.p += 4;
    if ((uint64_t)(b.end - b.p) < len) return IC_E_INPUT;
    h.stored_left = len; h.mode = 1;
    return IC_OK;
  }
  if (btype == 1) {
    for (int i = 0; i < 288; i++) s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    for (int i = 0; i < 32; i++) s.lens[288 + i] = 5;
    (void)ic_build(s.lens, 288, s.ll, false);
    (void)ic_build(s.lens + 288, 32, s.d, true);
    h.mode = 2;
    return IC_OK;
  }
  if (!ic_take(b, 14, &v)) return IC_E_INPUT;
  const int hlit = 257 + (int)(v & 31u), hdist = 1 + (int)((v >> 5) & 31u), hclen = 4 + (int)(v >> 10);
  if (hlit > 286 || hdist > 30) return IC_E_COUNTS;
  uint8_t cll[itsx_dc::NCL];
  for (int k = 0; k < itsx_dc::NCL; k++) cll[k] = 0;
  for (int k = 0; k < hclen; k++) {
    if (b.n < 3) ic_refill(b);
    if (!ic_take(b, 3, &v)) return IC_E_INPUT;
    cll[itsx_dc::dc_cl_order(k)] = (uint8_t)v;
  }
  { const int32_t r = ic_build(cll, itsx_dc::NCL, s.cl, false); if (r) return r; }
  const int total = hlit + hdist;
  for (int i = 0; i < total;) {                            // every turn consumes a code of at least one bit, or stops
    if (b.n < 16) ic_refill(b);
    const int32_t sym = ic_decode(b, s.cl);
    if (sym < 0) return sym == -2 ? IC_E_INPUT : IC_E_INCOMPLETE;
    if (sym < 16) { s.lens[i++] = (uint8_t)sym; continue; }
    int rep; uint8_t prev = 0;
    if (sym == 16) {
      if (i == 0) return IC_E_REPEAT;
      prev = s.lens[i - 1];
      if (!ic_take(b, 2, &v)) return IC_E_INPUT;
      rep = 3 + (int)v;
    } else if (sym == 17) { if (!ic_take(b, 3, &v)) return IC_E_INPUT; rep = 3 + (int)v; }
    else { if (!ic_take(b, 7, &v)) return IC_E_INPUT; rep = 11 + (int)v; }
    if (i + rep > total) return IC_E_REPEAT;
    while (rep-- > 0) s.lens[i++] = prev;
  }
  if (s.lens[256] == 0) return IC_E_NO_EOB;
  { const int32_t r = ic_build(s.lens, hlit, s.ll, false); if (r) return r; }
  { const int32_t r = ic_build(s.lens + hlit, hdist, s.d, true); if (r) return r; }
  h.mode = 2;
  return IC_OK;
}

// The next token, or a reason.  Every turn of the loop consumes at least one input bit or returns: a block header is 3 bits at the
// least, a code one; a stored run advances p.  Input is bounded by the span, so a malformed member terminates.
IC_HD int32_t ic_next(IcDecoder &s, IcHot &h, IcToken &t)
{
  IcBits &b = h.b;
  for (;;) {
    if (h.mode == 3) { t.kind_len = (uint32_t)IC_TOK_END << 16; t.val = 0; return IC_OK; }
    if (h.mode == 0) {
      if (h.final) { h.mode = 3; continue; }
      const int32_t r = ic_block(s, h);
      if (r) return r;
      continue;
    }
    if (h.mode == 1) {
      if (h.stored_left == 0) { h.mode = 0; continue; }
      const uint32_t k = h.stored_left < (uint32_t)IC_RUN ? h.stored_left : (uint32_t)IC_RUN;
      if ((uint64_t)h.produced + k > s.isize) return IC_E_OUTPUT;
      t.kind_len = ((uint32_t)IC_TOK_STORED << 16) | k; t.val = (uint32_t)(b.p - s.c);
      b.p += k; h.stored_left -= k; h.produced += k;
      return IC_OK;
    }
    ic_refill(b);                                          // at least 64 bits or the rest of the span: a token is 48 at the most
    const int32_t sym = ic_decode(b, s.ll);
    if (sym < 0) return sym == -2 ? IC_E_INPUT : IC_E_LSYMBOL;
    if (sym < 256) {
      if (h.produced >= s.isize) return IC_E_OUTPUT;
      t.kind_len = ((uint32_t)IC_TOK_LIT << 16) | 1u; t.val = (uint32_t)sym;
      h.produced++;
      return IC_OK;
    }
    if (sym == 256) { h.mode = 0; continue; }
    if (sym >= 286) return IC_E_LSYMBOL;
    uint32_t len, dist, v;
    if (sym < 265) len = (uint32_t)sym - 254u;
    else if (sym == 285) len = 258;
    else {
      const int e = (sym - 261) >> 2;
      if (!ic_take(b, e, &v)) return IC_E_INPUT;
      len = 3u + ((4u + (uint32_t)((sym - 261) & 3)) << e) + v;
    }
    const int32_t ds = ic_decode(b, s.d);
    if (ds < 0) return ds == -2 ? IC_E_INPUT : IC_E_DSYMBOL;
    if (ds >= 30) return IC_E_DSYMBOL;
    if (ds < 4) dist = (uint32_t)ds + 1u;
    else {
      const int e = (ds >> 1) - 1;
      if (!ic_take(b, e, &v)) return IC_E_INPUT;
      dist = 1u + ((2u + (uint32_t)(ds & 1)) << e) + v;
    }
    if (dist > h.produced) return IC_E_DISTANCE;
    if ((uint64_t)h.produced + len > s.isize) return IC_E_OUTPUT;
    t.kind_len = ((uint32_t)IC_TOK_MATCH << 16) | len; t.val = dist;
    h.produced += len;
    return IC_OK;
  }
}

// after IC_TOK_END: the deflate data ends exactly 8 bytes before c_end, isize bytes came out, CRC-32 and ISIZE are the trailer's
IC_HD int32_t ic_finish(const IcDecoder &s, IcHot &h, uint32_t crc)
{
  const uint8_t *q = ic_byte_position(h.b);
  if (h.b.end - q < 8) return IC_E_INPUT;
  if (h.b.end - q != 8) return IC_E_TRAILER;
  if (h.produced != s.isize) return IC_E_SHORT;
  const uint32_t want = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
  const uint32_t size = (uint32_t)q[4] | ((uint32_t)q[5] << 8) | ((uint32_t)q[6] << 16) | ((uint32_t)q[7] << 24);
  if (want != crc) return IC_E_CRC;
  if (size != s.isize) return IC_E_ISIZE;
  return IC_OK;
}

// ---- one member, serially: the compressed span [c, c_end), the text to o[0, isize) (o null: nowhere, a verification), a window of
// IC_WINDOW bytes that every back-reference is read from, and the 256-entry CRC table.  Invariants of the loop: no load lies outside
// [c, c_end) (the bit reader and the stored runs stop at c_end; the window is read at masked indices) and no store outside o[0, isize)
// (ic_next hands out no token that goes further); every turn takes a token, which consumed at least one input bit, or stops.
IC_HD int32_t ic_inflate_member(const uint8_t *c, const uint8_t *c_end, uint8_t *o, uint32_t isize, uint8_t *window, const uint32_t *crctab,
                                IcDecoder &s)
{
  { const int32_t r = ic_begin(s, c, c_end, isize); if (r) return r; }
  uint32_t pos = 0, crc = 0xffffffffu;
  for (;;) {
    IcToken t;
    { const int32_t r = ic_next(s, s.h, t); if (r) return r; }
    const int kind = ic_tok_kind(t);
    if (kind == IC_TOK_END) break;
    const uint32_t len = ic_tok_len(t);
    for (uint32_t j = 0; j < len; j++, pos++) {
      const uint8_t x = kind == IC_TOK_LIT ? (uint8_t)t.val : kind == IC_TOK_STORED ? c[t.val + j] : window[(pos - t.val) & (IC_WINDOW - 1)];
      window[pos & (IC_WINDOW - 1)] = x;
      if (o) o[pos] = x;
      crc = crctab[(crc ^ x) & 255u] ^ (crc >> 8);
    }
  }
  return ic_finish(s, s.h, ~crc);
}

// ---- a whole file of members on the host, one thread (itsx_debug_inflate_host, the sanitizer program): candidates found by walking
// the bytes, members in order, each verified into the window alone before its text is written, so that out holds nothing of a member
// that did not verify.  *text_len / *n_members count the members that verified; the reason is the first refusal's.
struct IcHostScratch { IcDecoder dec; uint8_t window[IC_WINDOW]; uint32_t crctab[256]; };
inline int32_t ic_inflate_file_host(const uint8_t *gz, int64_t n, uint8_t *out, int64_t out_cap, int64_t *text_len, int64_t *n_members,
                                    IcHostScratch &w)
{
  *text_len = 0; *n_members = 0;
  for (uint32_t i = 0; i < 256; i++) w.crctab[i] = itsx_dc::dc_crc_table_entry(i);
  if (n < 2 || gz[0] != 0x1f || gz[1] != 0x8b) return IC_E_NOT_GZIP;
  if (!ic_candidate(gz, n, 0)) { int32_t why = IC_OK; (void)ic_header(gz, n, &why); return why ? why : IC_E_FIRST; }
  int64_t at = 0;
  while (at < n) {
    int64_t next = at + 1;
    while (next < n && !ic_candidate(gz, n, next)) next++;
    if (next - at < IC_MIN_MEMBER) return IC_E_INPUT;
    const uint8_t *q = gz + next - 4;
    const uint32_t isize = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    { const int32_t r = ic_inflate_member(gz + at, gz + next, nullptr, isize, w.window, w.crctab, w.dec); if (r) return r; }
    if ((int64_t)isize > out_cap - *text_len) return IC_E_NOMEM;
    { const int32_t r = ic_inflate_member(gz + at, gz + next, out + *text_len, isize, w.window, w.crctab, w.dec); if (r) return r; }
    *text_len += isize; (*n_members)++;
    at = next;
  }
  return IC_OK;
}

}  // namespace itsx_ic
