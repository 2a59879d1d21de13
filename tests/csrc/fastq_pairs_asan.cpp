// fastq_pairs_asan.cpp -- csrc/fastq_rec.h's pair routines (fq_parse_pairs_host: fq_parse_host per text, then the host twin of the pass
// k_fastq_pairs makes over the planes: fq_upper16, fq_qual_ok16, the byte routines of the last group, the longest pair) over the catalogue
// tests/fastq_pair_cases.py writes, with every buffer allocated at exactly the size it needs: built with -fsanitize=address,undefined by
// tests/test_device_parse_pairs_cpu.py, so a read or write one byte outside a text, the offsets or a plane ends the program.
// usage: fastq_pairs_asan corpus.bin
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "fastq_rec.h"

using namespace itsx_fq;

static bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static uint8_t *exact(size_t n) { return n ? (uint8_t *)malloc(n) : nullptr; }
struct Side { std::vector<int64_t> off, toff; std::vector<uint8_t> seq, qual, titles; };

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: fastq_pairs_asan corpus.bin\n"); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  int good = 0, bad = 0, failed = 0;
  for (int k = 0;; k++) {
    int32_t want = 0, want_side = 0; int64_t nbytes[2] = {0, 0};
    uint8_t *text[2] = {nullptr, nullptr};
    if (fread(&want, 4, 1, f) != 1) break;
    if (!get(f, &want_side, 4)) return 2;
    for (int s = 0; s < 2; s++) {
      if (!get(f, &nbytes[s], 8)) return 2;
      text[s] = exact((size_t)nbytes[s]);
      if (!get(f, text[s], (size_t)nbytes[s])) { fprintf(stderr, "case %d: truncated corpus\n", k); return 2; }
    }
    int64_t n = -1, sizes[4], mx = -1, rec = -2; int32_t flags = -1, side = -2;
    int64_t guard[4] = {-7, -7, -7, -7};
    // measured first (no room at all: nothing may be written), then the exact buffers
    const FqSideBufs none1{&guard[0], &guard[1], nullptr, nullptr, nullptr}, none2{&guard[2], &guard[3], nullptr, nullptr, nullptr};
    int32_t why = fq_parse_pairs_host(text[0], nbytes[0], text[1], nbytes[1], none1, none2, -1, 0, 0, &n, sizes, &flags, &mx, &side, &rec);
    bool ok = guard[0] == -7 && guard[1] == -7 && guard[2] == -7 && guard[3] == -7;
    if (want != FQ_OK) {
      ok = ok && why == want && side == want_side && n == 0 && sizes[0] == 0 && sizes[2] == 0;
      bad++;
    } else {
      ok = ok && why == FQ_E_CAP;
      int64_t en = 0, emx = 0; int32_t eflags = 0;
      if (!get(f, &en, 8) || !get(f, &eflags, 4) || !get(f, &emx, 8)) return 2;
      Side e[2];
      for (int s = 0; s < 2; s++) {
        int64_t nb = 0, nt = 0;
        e[s].off.resize((size_t)en + 1); e[s].toff.resize((size_t)en + 1);
        if (!get(f, e[s].off.data(), (size_t)(en + 1) * 8) || !get(f, e[s].toff.data(), (size_t)(en + 1) * 8) || !get(f, &nb, 8)) return 2;
        e[s].seq.resize((size_t)nb); e[s].qual.resize((size_t)nb);
        if (!get(f, e[s].seq.data(), (size_t)nb) || !get(f, e[s].qual.data(), (size_t)nb) || !get(f, &nt, 8)) return 2;
        e[s].titles.resize((size_t)nt);
        if (!get(f, e[s].titles.data(), (size_t)nt)) return 2;
      }
      ok = ok && n == en && sizes[0] == (int64_t)e[0].seq.size() && sizes[1] == (int64_t)e[0].titles.size() && sizes[2] == (int64_t)e[1].seq.size() && sizes[3] == (int64_t)e[1].titles.size();
      if (ok) {
        // one call's caps hold for both sides: each side's buffers are exact for that side, so the caps are the larger side's and the
        // routine must still stay inside the smaller side's blocks
        const int64_t cb = sizes[0] > sizes[2] ? sizes[0] : sizes[2], ct = sizes[1] > sizes[3] ? sizes[1] : sizes[3];
        FqSideBufs b[2];
        for (int s = 0; s < 2; s++)
          b[s] = FqSideBufs{(int64_t *)exact((size_t)(n + 1) * 8), (int64_t *)exact((size_t)(n + 1) * 8), exact((size_t)sizes[2 * s]), exact((size_t)sizes[2 * s]), exact((size_t)sizes[2 * s + 1])};
        why = fq_parse_pairs_host(text[0], nbytes[0], text[1], nbytes[1], b[0], b[1], n, cb, ct, &n, sizes, &flags, &mx, &side, &rec);
        ok = ok && why == FQ_OK && n == en && flags == eflags && mx == emx;
        for (int s = 0; s < 2 && ok; s++) {
          const size_t nb = e[s].seq.size(), nt = e[s].titles.size();
          ok = ok && memcmp(b[s].off, e[s].off.data(), (size_t)(n + 1) * 8) == 0 && memcmp(b[s].toff, e[s].toff.data(), (size_t)(n + 1) * 8) == 0;
          ok = ok && (nb == 0 || (memcmp(b[s].seq, e[s].seq.data(), nb) == 0 && memcmp(b[s].qual, e[s].qual.data(), nb) == 0));
          ok = ok && (nt == 0 || memcmp(b[s].titles, e[s].titles.data(), nt) == 0);
        }
        for (int s = 0; s < 2; s++) { free(b[s].off); free(b[s].toff); free(b[s].seq); free(b[s].qual); free(b[s].titles); }
      }
      good++;
    }
    if (!ok) { failed++; printf("case %d: FAILED (wanted reason %d on side %d, got %d on side %d; %lld pairs, flags %d, longest %lld)\n", k, want, want_side, why, side, (long long)n, flags, (long long)mx); }
    free(text[0]); free(text[1]);
  }
  fclose(f);
  // the 16-byte routines against the byte routines: every byte value at every position of a group
  int groups = 0;
  for (int v = 0; v < 256; v++)
    for (int at = 0; at < 16; at++) {
      uint8_t g[16], q[16];
      memset(g, 'A', 16); memset(q, 'I', 16);
      g[at] = q[at] = (uint8_t)v;
      uint32_t w[4], qw[4];
      memcpy(w, g, 16); memcpy(qw, q, 16);
      const bool changed = fq_upper16(w), fine = fq_qual_ok16(qw);
      uint8_t u[16];
      memcpy(u, w, 16);
      bool same = changed == (fq_upper1((uint8_t)v) != v) && fine == fq_qual_ok1((uint8_t)v);
      for (int j = 0; j < 16; j++) same = same && u[j] == fq_upper1(g[j]);
      if (!same) { failed++; printf("byte %d at %d: the 16-byte routines and the byte routines differ\n", v, at); }
      groups++;
    }
  printf("%d good, %d bad, %d groups, %d failed\n", good, bad, groups, failed);
  return failed ? 1 : 0;
}
