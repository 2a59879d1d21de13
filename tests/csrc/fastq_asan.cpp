// fastq_asan.cpp -- csrc/fastq_rec.h (the rule the device parse runs per record) on the host, over the corpus tests/fastq_cases.py writes,
// with every buffer allocated at exactly the size it needs: built with -fsanitize=address,undefined by tests/test_device_parse_cpu.py, so a
// read or write one byte outside the text, the offsets or a plane ends the program.  usage: fastq_asan corpus.bin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "fastq_rec.h"

using namespace itsx_fq;

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
// a heap block of exactly n bytes (n == 0: one byte nobody may touch is not needed -- a null pointer is never dereferenced)
static uint8_t *exact(size_t n) { return n ? (uint8_t *)malloc(n) : nullptr; }

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: fastq_asan corpus.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int good = 0, bad = 0, failed = 0;
  for (int k = 0;; k++) {
    int32_t want = 0; int64_t want_rec = 0, nbytes = 0;
    if (fread(&want, 4, 1, f) != 1) break;
    if (!get(f, &want_rec, 8) || !get(f, &nbytes, 8)) { fprintf(stderr, "case %d: truncated corpus\n", k); return 2; }
    uint8_t *text = exact((size_t)nbytes);
    if (!get(f, text, (size_t)nbytes)) { fprintf(stderr, "case %d: truncated corpus\n", k); return 2; }
    int64_t n = 0, nb = 0, nt = 0, rec = -2;
    int64_t one[1] = {-7}, two[1] = {-7};
    // sizes first (no room at all: nothing may be written), then the exact buffers
    int32_t why = fq_parse_host(text, nbytes, one, two, -1, nullptr, nullptr, 0, nullptr, 0, &n, &nb, &nt, &rec);
    bool ok = one[0] == -7 && two[0] == -7;
    if (want != FQ_OK) {
      ok = ok && why == want && rec == want_rec && n == 0 && nb == 0 && nt == 0;
      bad++;
    } else {
      ok = ok && why == FQ_E_CAP;
      int64_t en = 0, enb = 0, ent = 0;
      if (!get(f, &en, 8)) return 2;
      std::vector<int64_t> eoff((size_t)en + 1), etoff((size_t)en + 1);
      if (!get(f, eoff.data(), (size_t)(en + 1) * 8) || !get(f, etoff.data(), (size_t)(en + 1) * 8) || !get(f, &enb, 8)) return 2;
      std::vector<uint8_t> eseq((size_t)enb), equal((size_t)enb);
      if (!get(f, eseq.data(), (size_t)enb) || !get(f, equal.data(), (size_t)enb) || !get(f, &ent, 8)) return 2;
      std::vector<uint8_t> etitles((size_t)ent);
      if (!get(f, etitles.data(), (size_t)ent)) return 2;
      ok = ok && n == en && nb == enb && nt == ent;
      if (ok) {
        for (int pass = 0; pass < 2; pass++) {          // with and without the quality plane
          int64_t *off = (int64_t *)exact((size_t)(n + 1) * 8), *toff = (int64_t *)exact((size_t)(n + 1) * 8);
          uint8_t *seq = exact((size_t)nb), *qual = pass ? nullptr : exact((size_t)nb), *titles = exact((size_t)nt);
          why = fq_parse_host(text, nbytes, off, toff, n, seq, qual, nb, titles, nt, &n, &nb, &nt, &rec);
          ok = ok && why == FQ_OK && rec == -1 && n == en && nb == enb && nt == ent;
          ok = ok && memcmp(off, eoff.data(), (size_t)(n + 1) * 8) == 0 && memcmp(toff, etoff.data(), (size_t)(n + 1) * 8) == 0;
          ok = ok && (nb == 0 || (memcmp(seq, eseq.data(), (size_t)nb) == 0 && (pass || memcmp(qual, equal.data(), (size_t)nb) == 0)));
          ok = ok && (nt == 0 || memcmp(titles, etitles.data(), (size_t)nt) == 0);
          free(off); free(toff); free(seq); free(qual); free(titles);
        }
      }
      good++;
    }
    if (!ok) { failed++; printf("case %d: FAILED (wanted reason %d at record %lld, got %d at %lld; %lld records)\n", k, want, (long long)want_rec, why, (long long)rec, (long long)n); }
    free(text);
  }
  fclose(f);
  printf("%d good, %d bad, %d failed\n", good, bad, failed);
  return failed ? 1 : 0;
}
