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

}  // namespace itsx_fq
