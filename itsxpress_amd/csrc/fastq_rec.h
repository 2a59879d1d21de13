// fastq_rec.h -- the rule by which FASTQ text is taken apart on the device (k_fastq.hip), in a form the host can run too (tests, the
// sanitizer program): no HIP, no allocation in the per-line and per-record routines.
//
// A text is a sequence of lines: a newline ends a line, a last line without a newline counts, and a '\r' before the line's end is not
// part of a non-empty line.  Record r is lines 4 r .. 4 r + 3.  The text is ACCEPTED only when
//   * it has exactly 4 n lines (a text of no bytes: n = 0),
//   * every title line is non-empty and starts with '@',
//   * every third line is non-empty and starts with '+',
//   * every quality line is as long as its sequence line.
// Under these rules the engine's host parser (parse_fastx_range) walks exactly the same lines: it skips blank lines only where it
// expects a title, and no title line is blank.  So "accepted" means "the host parser's records, byte for byte".  Everything else --
// FASTA, blank lines anywhere, a malformed record -- is DECLINED with a reason and the lowest record it shows at; what the host parser
// makes of such a text (it may well accept it) is the host path's business.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

#if defined(__HIPCC__)
#define FQ_HD __host__ __device__ __forceinline__
#else
#define FQ_HD inline
#endif

namespace itsx_fq {

enum : int32_t {
  FQ_OK = 0,
  FQ_E_LINES = 1,        // the line count is not 4 n (trailing blank lines, FASTA with an odd line count, a text that is only a newline)
  FQ_E_TITLE = 2,        // a title line is empty or does not start with '@' (FASTA, a blank line where a record starts)
  FQ_E_PLUS = 3,         // a third line is empty or does not start with '+'
  FQ_E_QUAL = 4,         // a quality line and its sequence line differ in length
  FQ_E_NOMEM = 5,        // device memory for the index or the planes could not be had
  FQ_E_CAP = 6,          // (host routine only) the caller's buffers are too small
  FQ_E_PAIRS = 7,        // (a pair of texts only) R1 and R2 hold different numbers of records
};

inline const char *fq_reason_name(int32_t why)
{
  switch (why) {
    case FQ_OK: return "ok";
    case FQ_E_LINES: return "line count is not a multiple of four";
    case FQ_E_TITLE: return "title line is empty or lacks '@'";
    case FQ_E_PLUS: return "third line is empty or lacks '+'";
    case FQ_E_QUAL: return "quality and sequence differ in length";
    case FQ_E_NOMEM: return "no memory";
    case FQ_E_CAP: return "buffers too small";
    case FQ_E_PAIRS: return "R1 and R2 hold different numbers of records";
  }
  return "unknown";
}

// line k = bytes [b, e) of the text.  nl[j] = the position of the j-th newline; for an unterminated last line nl[its index] = nbytes.
FQ_HD void fq_line(const uint8_t *text, const int64_t *nl, int64_t k, int64_t &b, int64_t &e)
{
  b = k > 0 ? nl[k - 1] + 1 : 0;
  e = nl[k];
  if (e > b && text[e - 1] == '\r') e--;
}

struct FqRec { int64_t t0, tl, s0, sl, q0; int32_t bad; };      // title [t0, t0 + tl), bases [s0, s0 + sl), qualities [q0, q0 + sl) where bad == 0

FQ_HD FqRec fq_record(const uint8_t *text, const int64_t *nl, int64_t r)
{
  FqRec q;
  int64_t te, se, p0, pe, qe;
  fq_line(text, nl, 4 * r, q.t0, te);
  fq_line(text, nl, 4 * r + 1, q.s0, se);
  fq_line(text, nl, 4 * r + 2, p0, pe);
  fq_line(text, nl, 4 * r + 3, q.q0, qe);
  q.tl = te - q.t0; q.sl = se - q.s0;
  q.bad = (q.tl <= 0 || text[q.t0] != '@') ? FQ_E_TITLE : (pe - p0 <= 0 || text[p0] != '+') ? FQ_E_PLUS : (qe - q.q0 != q.sl) ? FQ_E_QUAL : FQ_OK;
  return q;
}

// the verdict word the plan kernel folds with atomicMin: the lowest bad record and its reason
constexpr unsigned long long FQ_VERDICT_NONE = ~0ull;
FQ_HD unsigned long long fq_verdict(int64_t r, int32_t why) { return ((unsigned long long)r << 3) | (unsigned long long)why; }

// The whole rule on one host thread.  Returns FQ_OK or the reason; *bad_record = the record it shows at (-1: the text as a whole).
// n_records / n_bases / n_title_bytes are set on FQ_OK and on FQ_E_CAP (what the buffers must hold: off and toff n + 1 entries, seq and
// qual n_bases bytes, titles n_title_bytes); nothing is written to a buffer unless all of them are large enough.  qual == null: no
// qualities are kept.
inline int32_t fq_parse_host(const uint8_t *text, int64_t nbytes, int64_t *off, int64_t *toff, int64_t cap_records, uint8_t *seq, uint8_t *qual, int64_t cap_bases,
                             uint8_t *titles, int64_t cap_titles, int64_t *n_records, int64_t *n_bases, int64_t *n_title_bytes, int64_t *bad_record)
{
  *n_records = *n_bases = *n_title_bytes = 0; *bad_record = -1;
  std::vector<int64_t> nl;
  for (int64_t p = 0; p < nbytes;) {
    const void *q = memchr(text + p, '\n', (size_t)(nbytes - p));
    if (!q) break;
    p = (int64_t)((const uint8_t *)q - text);
    nl.push_back(p);
    p++;
  }
  if (nbytes > 0 && text[nbytes - 1] != '\n') nl.push_back(nbytes);
  const int64_t lines = (int64_t)nl.size();
  if (lines % 4 != 0) return FQ_E_LINES;
  const int64_t n = lines / 4;
  int64_t nb = 0, nt = 0;
  for (int64_t r = 0; r < n; r++) {
    const FqRec q = fq_record(text, nl.data(), r);
    if (q.bad) { *bad_record = r; return q.bad; }
    nb += q.sl; nt += q.tl;
  }
  *n_records = n; *n_bases = nb; *n_title_bytes = nt;
  if (cap_records < n || cap_bases < nb || cap_titles < nt) return FQ_E_CAP;
  nb = nt = 0;
  for (int64_t r = 0; r < n; r++) {
    const FqRec q = fq_record(text, nl.data(), r);
    off[r] = nb; toff[r] = nt;
    if (q.sl) { memcpy(seq + nb, text + q.s0, (size_t)q.sl); if (qual) memcpy(qual + nb, text + q.q0, (size_t)q.sl); }
    memcpy(titles + nt, text + q.t0, (size_t)q.tl);
    nb += q.sl; nt += q.tl;
  }
  off[n] = nb; toff[n] = nt;
  return FQ_OK;
}

// ---- the pass over a pair's planes (k_fastq.hip: k_fastq_pairs; the paired merge loaders of a context that opted in).  What the host
// path does to R1 / R2 between its parser and the merge kernel, per 16 aligned bytes of a plane held as four little-endian dwords:
//   bases      'a'..'z' -> 'A'..'Z' and nothing else (the host parser's toupper in the C locale); "changed" is reported,
//   qualities  every byte must lie in 33..126 (merge_core's check).
// Byte-parallel arithmetic on the low seven bits of each byte, so no carry crosses a byte: bit 7 of a byte of (h + 0x1f) says h >= 'a',
// of (h + 0x05) says h > 'z', of (h + 0x5f) says h >= 33, of (h + 0x01) says h == 127; a byte above 127 is neither a letter nor a quality.
enum : int32_t { FQ_PAIR_LOWER1 = 1, FQ_PAIR_LOWER2 = 2, FQ_PAIR_QUAL1 = 4, FQ_PAIR_QUAL2 = 8 };      // the flags of a pair of texts

FQ_HD uint32_t fq_upper4(uint32_t x)
{
  const uint32_t h = x & 0x7f7f7f7fu;
  const uint32_t lower = (h + 0x1f1f1f1fu) & ~(h + 0x05050505u) & ~x & 0x80808080u;
  return x ^ (lower >> 2);
}
FQ_HD uint32_t fq_qual_bad4(uint32_t x)
{
  const uint32_t h = x & 0x7f7f7f7fu;
  return (x | ~(h + 0x5f5f5f5fu) | (h + 0x01010101u)) & 0x80808080u;
}
// true: a base changed
FQ_HD bool fq_upper16(uint32_t (&w)[4])
{
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { const uint32_t u = fq_upper4(w[k]); diff |= u ^ w[k]; w[k] = u; }
  return diff != 0;
}
FQ_HD bool fq_qual_ok16(const uint32_t (&w)[4]) { return (fq_qual_bad4(w[0]) | fq_qual_bad4(w[1]) | fq_qual_bad4(w[2]) | fq_qual_bad4(w[3])) == 0; }
// the same by bytes: the last, partial group of a plane
FQ_HD uint8_t fq_upper1(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
FQ_HD bool fq_qual_ok1(uint8_t c) { return c >= 33 && c <= 126; }

// one side on one host thread, group by group as the kernel's lanes go: bytes [0, total) of seq are upper-cased in place (stored only
// where a byte changed), nothing else is touched.  Returns FQ_PAIR_LOWER1 | FQ_PAIR_QUAL1 as they apply.
inline int32_t fq_pair_side_host(uint8_t *seq, const uint8_t *qual, int64_t total)
{
  int32_t flags = 0;
  int64_t p = 0;
  for (; p + 16 <= total; p += 16) {
    uint32_t w[4];
    memcpy(w, seq + p, 16);
    if (fq_upper16(w)) { memcpy(seq + p, w, 16); flags |= FQ_PAIR_LOWER1; }
    memcpy(w, qual + p, 16);
    if (!fq_qual_ok16(w)) flags |= FQ_PAIR_QUAL1;
  }
  for (; p < total; p++) {
    const uint8_t u = fq_upper1(seq[p]);
    if (u != seq[p]) { seq[p] = u; flags |= FQ_PAIR_LOWER1; }
    if (!fq_qual_ok1(qual[p])) flags |= FQ_PAIR_QUAL1;
  }
  return flags;
}
// the longest pair: max over i of (off1[i + 1] - off1[i]) + (off2[i + 1] - off2[i]); no pairs: 0
inline int64_t fq_pair_max_total(const int64_t *off1, const int64_t *off2, int64_t n)
{
  int64_t m = 0;
  for (int64_t i = 0; i < n; i++) { const int64_t t = (off1[i + 1] - off1[i]) + (off2[i + 1] - off2[i]); m = t > m ? t : m; }
  return m;
}

// Two texts as a pair, on one host thread: each by fq_parse_host into its own buffers (caps per side), then the pass.  Returns FQ_OK, a
// side's reason (*bad_side = 0 / 1, *bad_record as fq_parse_host gives it), FQ_E_PAIRS (*bad_side = -1), or FQ_E_CAP; sizes[4] = bases
// and title bytes of R1, then of R2 (set on FQ_OK and FQ_E_CAP, like *n_pairs).  Nothing is written to a buffer unless FQ_OK is returned.
struct FqSideBufs { int64_t *off, *toff; uint8_t *seq, *qual, *titles; };
inline int32_t fq_parse_pairs_host(const uint8_t *text1, int64_t nbytes1, const uint8_t *text2, int64_t nbytes2, const FqSideBufs &b1, const FqSideBufs &b2,
                                   int64_t cap_records, int64_t cap_bases, int64_t cap_titles, int64_t *n_pairs, int64_t *sizes, int32_t *flags, int64_t *max_total,
                                   int32_t *bad_side, int64_t *bad_record)
{
  const uint8_t *text[2] = {text1, text2}; const int64_t nbytes[2] = {nbytes1, nbytes2}; const FqSideBufs *b[2] = {&b1, &b2};
  int64_t n[2] = {0, 0};
  *n_pairs = 0; sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0; *flags = 0; *max_total = 0; *bad_side = -1; *bad_record = -1;
  for (int s = 0; s < 2; s++) {                  // measured first (no room at all: nothing can be written)
    const int32_t why = fq_parse_host(text[s], nbytes[s], nullptr, nullptr, -1, nullptr, nullptr, -1, nullptr, -1, &n[s], &sizes[2 * s], &sizes[2 * s + 1], bad_record);
    if (why != FQ_E_CAP) { *bad_side = s; sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0; return why; }
  }
  if (n[0] != n[1]) { sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0; return FQ_E_PAIRS; }
  *n_pairs = n[0];
  if (cap_records < n[0] || cap_bases < sizes[0] || cap_bases < sizes[2] || cap_titles < sizes[1] || cap_titles < sizes[3]) return FQ_E_CAP;
  for (int s = 0; s < 2; s++) {
    int64_t nn, nb, nt, rec;
    const int32_t why = fq_parse_host(text[s], nbytes[s], b[s]->off, b[s]->toff, cap_records, b[s]->seq, b[s]->qual, cap_bases, b[s]->titles, cap_titles, &nn, &nb, &nt, &rec);
    if (why != FQ_OK) { *bad_side = s; *bad_record = rec; return why; }
    *flags |= fq_pair_side_host(b[s]->seq, b[s]->qual, nb) << s;
  }
  *max_total = fq_pair_max_total(b1.off, b2.off, n[0]);
  return FQ_OK;
}

}  // namespace itsx_fq
