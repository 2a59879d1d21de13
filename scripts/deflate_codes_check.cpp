// deflate_codes_check.cpp -- a stand-alone check of itsxpress_amd/csrc/deflate_codes.h on the host, meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I itsxpress_amd/csrc scripts/deflate_codes_check.cpp -lz -o deflate_codes_check
// It runs the code-length limit where it must engage (Fibonacci counts), the one-symbol case, and a serial coder that puts the header's
// functions together the way k_deflate.hip does (tokens -> counts -> lengths -> codes -> header -> bits) and has zlib inflate the result.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <zlib.h>
#include "deflate_codes.h"

using namespace itsx_dc;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void check_lengths(const char *what, const std::vector<uint32_t> &f, int maxbits)
{
  std::vector<uint8_t> len(f.size());
  std::vector<uint32_t> work(WORK_WORDS);
  dc_huffman_lengths(f.data(), (int)f.size(), maxbits, len.data(), work.data());
  uint64_t kraft = 0; int used = 0, deepest = 0;
  for (size_t i = 0; i < f.size(); i++) {
    CHECK((f[i] == 0) == (len[i] == 0), "%s: symbol %zu count %u length %d", what, i, f[i], len[i]);
    if (len[i]) { used++; kraft += 1ull << (maxbits - len[i]); if (len[i] > deepest) deepest = len[i]; }
  }
  CHECK(deepest <= maxbits, "%s: length %d over %d", what, deepest, maxbits);
  if (used == 1) CHECK(deepest == 1, "%s: one symbol of length %d", what, deepest);
  if (used >= 2) CHECK(kraft == (1ull << maxbits), "%s: Kraft sum %llu / %llu", what, (unsigned long long)kraft, 1ull << maxbits);
  printf("%-28s used %3d deepest %2d\n", what, used, deepest);
}

struct Bits {
  std::vector<uint8_t> out; uint64_t acc = 0; int n = 0;
  void put(uint32_t v, int nb) { acc |= (uint64_t)v << n; n += nb; while (n >= 8) { out.push_back((uint8_t)acc); acc >>= 8; n -= 8; } }
  void flush() { if (n) { out.push_back((uint8_t)acc); acc = 0; n = 0; } }
};

// one final dynamic block over the whole text; greedy matches from a 4-byte hash of the latest position
static void check_roundtrip(const char *what, const std::vector<uint8_t> &text)
{
  const int n = (int)text.size();
  std::vector<uint32_t> tok;                 // a literal byte, or 1<<31 | (dist - 1) << 8 | (len - 3)
  std::vector<int> head(1 << 13, -1);
  auto hash = [&](int p) { uint32_t v; memcpy(&v, &text[(size_t)p], 4); return (v * 2654435761u) >> 19; };
  for (int p = 0; p < n;) {
    int best = 0, dist = 0;
    if (p + 4 <= n) {
      const int c = head[hash(p)];
      if (c >= 0 && p - c <= 32768) { int l = 0; while (l < 258 && p + l < n && text[(size_t)(c + l)] == text[(size_t)(p + l)]) l++; if (l >= 4) { best = l; dist = p - c; } }
    }
    const int step = best ? best : 1;
    tok.push_back(best ? (1u << 31 | (uint32_t)(dist - 1) << 8 | (uint32_t)(best - 3)) : text[(size_t)p]);
    for (int q = p; q < p + step; q++) if (q + 4 <= n) head[hash(q)] = q;
    p += step;
  }
  std::vector<uint32_t> fl(NLL, 0), fd(NDIST, 0), work(WORK_WORDS);
  int eb; uint32_t ev;
  for (uint32_t t : tok) {
    if (t >> 31) { fl[(size_t)dc_length_symbol((int)(t & 255) + 3, &eb, &ev)]++; fd[(size_t)dc_distance_symbol((int)((t >> 8) & 32767) + 1, &eb, &ev)]++; }
    else fl[t]++;
  }
  fl[256]++;
  dc_at_least_two(fd.data(), NDIST);
  uint8_t ll_len[NLL], d_len[NDIST]; uint16_t ll_code[NLL], d_code[NDIST];
  dc_huffman_lengths(fl.data(), NLL, 15, ll_len, work.data());
  dc_huffman_lengths(fd.data(), NDIST, 15, d_len, work.data());
  dc_canonical_codes(ll_len, NLL, ll_code);
  dc_canonical_codes(d_len, NDIST, d_code);
  DcHeader h;
  dc_build_header(ll_len, d_len, &h, work.data());
  Bits b;
  b.put(1, 1); b.put(2, 2);
  b.put((uint32_t)h.hlit - 257, 5); b.put((uint32_t)h.hdist - 1, 5); b.put((uint32_t)h.hclen - 4, 4);
  for (int k = 0; k < h.hclen; k++) b.put(h.cl_len[dc_cl_order(k)], 3);
  for (int k = 0; k < h.nsym; k++) { b.put(h.cl_code[h.sym[k]], h.cl_len[h.sym[k]]); b.put(h.ext[k], dc_cl_extra_bits(h.sym[k])); }
  CHECK((uint64_t)b.out.size() * 8 + (uint64_t)b.n == 3 + (uint64_t)h.bits, "%s: header of %llu bits, %u said", what, (unsigned long long)(b.out.size() * 8 + b.n) - 3, h.bits);
  for (uint32_t t : tok) {
    if (t >> 31) {
      int s = dc_length_symbol((int)(t & 255) + 3, &eb, &ev);
      b.put(ll_code[s], ll_len[s]); b.put(ev, eb);
      s = dc_distance_symbol((int)((t >> 8) & 32767) + 1, &eb, &ev);
      b.put(d_code[s], d_len[s]); b.put(ev, eb);
    } else b.put(ll_code[t], ll_len[t]);
  }
  b.put(ll_code[256], ll_len[256]);
  b.flush();
  std::vector<uint8_t> back((size_t)n + 16);
  z_stream z; memset(&z, 0, sizeof z);
  CHECK(inflateInit2(&z, -15) == Z_OK, "%s: inflateInit2", what);
  z.next_in = b.out.data(); z.avail_in = (uInt)b.out.size(); z.next_out = back.data(); z.avail_out = (uInt)back.size();
  const int rc = inflate(&z, Z_FINISH);
  CHECK(rc == Z_STREAM_END, "%s: inflate says %d (%s)", what, rc, z.msg ? z.msg : "");
  CHECK((int)z.total_out == n && (n == 0 || memcmp(back.data(), text.data(), (size_t)n) == 0), "%s: %lu bytes back of %d", what, z.total_out, n);
  inflateEnd(&z);
  printf("%-28s %7d bytes -> %7zu, %zu tokens\n", what, n, b.out.size(), tok.size());
}

int main()
{
  {
    std::vector<uint32_t> fib30(30), fib19(19);
    uint32_t a = 1, b = 1;
    for (int i = 0; i < 30; i++) { fib30[(size_t)i] = a; if (i < 19) fib19[(size_t)i] = a; const uint32_t c = a + b; a = b; b = c; }
    check_lengths("fibonacci 30 / 15 bits", fib30, 15);
    check_lengths("fibonacci 19 / 7 bits", fib19, 7);
    std::vector<uint32_t> one(286, 0); one[256] = 1;
    check_lengths("symbol 256 alone", one, 15);
    check_lengths("286 equal", std::vector<uint32_t>(286, 7), 15);
    std::vector<uint32_t> skew(286, 1); skew[0] = 65536;
    check_lengths("one heavy among 285", skew, 15);
    check_lengths("none", std::vector<uint32_t>(30, 0), 15);
  }
  for (int l = 3; l <= 258; l++) {          // the symbol maps against the tables of RFC 1951 3.2.5
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    int eb; uint32_t ev;
    const int s = dc_length_symbol(l, &eb, &ev);
    CHECK(s >= 257 && s <= 285 && eb == extra[s - 257] && base[s - 257] + (int)ev == l && (int)ev < (1 << eb), "length %d: symbol %d, %d extra bits of value %u", l, s, eb, ev);
  }
  for (int d = 1; d <= 32768; d++) {
    int eb; uint32_t ev;
    const int s = dc_distance_symbol(d, &eb, &ev);
    const int xb = s < 4 ? 0 : s / 2 - 1, base = s < 4 ? s + 1 : 1 + ((2 + (s & 1)) << xb);
    CHECK(s >= 0 && s < 30 && eb == xb && base + (int)ev == d && (int)ev < (1 << eb), "distance %d: symbol %d, %d extra bits of value %u", d, s, eb, ev);
  }
  {
    uint32_t seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    std::vector<uint8_t> t;
    std::vector<std::string> recs;
    for (int r = 0; r < 8; r++) { std::string s; const int L = 200 + (int)(rnd() % 260); for (int i = 0; i < L; i++) s += "ACGT"[rnd() & 3]; recs.push_back(s); }
    while (t.size() < 60000) { const std::string &s = recs[rnd() & 7]; t.insert(t.end(), s.begin(), s.end()); t.push_back('\n'); }
    check_roundtrip("repeated records", t);
    t.assign(65536, 0); check_roundtrip("zeros", t);
    t.clear(); for (int i = 0; i < 40000; i++) t.push_back((uint8_t)rnd()); check_roundtrip("random bytes", t);
    t.clear(); for (int i = 0; i < 259 * 9; i++) t.push_back((uint8_t)(i % 259 % 251)); check_roundtrip("period 259", t);
    t.clear(); { uint32_t fa = 1, fb = 1; for (int i = 0; i < 22; i++) { for (uint32_t k = 0; k < fa; k++) t.push_back((uint8_t)i); const uint32_t c = fa + fb; fa = fb; fb = c; } }
    for (size_t i = t.size() - 1; i > 0; i--) { const size_t j = rnd() % (i + 1); const uint8_t x = t[i]; t[i] = t[j]; t[j] = x; }
    check_roundtrip("fibonacci byte counts", t);
    t.assign(1, 'A'); check_roundtrip("one byte", t);
    t.assign(5, 'A'); check_roundtrip("five bytes", t);
  }
  {                                          // a text's CRC-32 from its pieces' against zlib's
    uint32_t xp[CRC_POWERS]; dc_crc_powers(xp);
    uint32_t seed = 99; std::vector<uint8_t> t(70001);
    for (auto &c : t) { seed = seed * 1664525u + 1013904223u; c = (uint8_t)(seed >> 24); }
    for (uInt i = 0; i < 256; i++) CHECK(dc_crc_table_entry(i) == get_crc_table()[i], "crc table entry %u", i);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4097, (size_t)65536, t.size()}) {
      uint32_t c = 0;
      for (size_t o = 0; o < n; o += 64) { const size_t b = n - o < 64 ? n - o : 64; c = dc_crc_append(xp, c, (uint32_t)crc32(0, t.data() + o, (uInt)b), (uint32_t)b); }
      CHECK(c == crc32(0, t.data(), (uInt)n), "crc of %zu bytes from 64-byte pieces", n);
      const size_t h = n / 3;
      CHECK(dc_crc_append(xp, (uint32_t)crc32(0, t.data(), (uInt)h), (uint32_t)crc32(0, t.data() + h, (uInt)(n - h)), (uint32_t)(n - h)) == crc32(0, t.data(), (uInt)n), "crc of %zu bytes from two pieces", n);
    }
    printf("crc pieces                   ok\n");
  }
  if (g_fail) { fprintf(stderr, "%d check(s) failed\n", g_fail); return 1; }
  printf("all checks passed\n");
  return 0;
}
