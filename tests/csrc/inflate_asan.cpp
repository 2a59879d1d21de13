// inflate_asan.cpp -- csrc/inflate_codes.h under AddressSanitizer and UBSan, stand-alone: reads the corpus file that
// tests/inflate_cases.py writes and runs every case with its input and its output allocated at their exact sizes, so that one load
// past the compressed bytes or one store past the text is a report.  A good case must give its text; a bad case must be refused, give
// the text of the members before the refusal and nothing more, and is then decoded once more as ONE member over the whole input with
// the ISIZE its last four bytes claim (capped), the output exactly that long: the refusal itself stays inside the buffers.
// usage: inflate_asan corpus.bin     exit 0: every case as expected
#include "inflate_codes.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace itsx_ic;

static bool rd(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s corpus.bin\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  uint32_t count = 0;
  if (!rd(f, &count, 4)) return 2;
  IcHostScratch *w = new IcHostScratch;
  int failed = 0, good = 0, bad = 0;
  for (uint32_t k = 0; k < count; k++) {
    uint32_t nl = 0; uint8_t flag = 0; uint64_t gl = 0, tl = 0;
    if (!rd(f, &nl, 4)) return 2;
    std::string name(nl, ' ');
    if (!rd(f, &name[0], nl) || !rd(f, &flag, 1) || !rd(f, &gl, 8)) return 2;
    uint8_t *gz = (uint8_t *)malloc(gl ? gl : 1);                       // exact: the allocator's redzone begins at gz + gl
    if (!rd(f, gz, gl) || !rd(f, &tl, 8)) return 2;
    std::vector<uint8_t> text(tl);
    if (!rd(f, text.data(), tl)) return 2;
    uint8_t *out = (uint8_t *)malloc(tl ? tl : 1);
    int64_t got = -1, members = -1;
    const int32_t r = ic_inflate_file_host(gz, (int64_t)gl, out, (int64_t)tl, &got, &members, *w);
    bool ok = got == (int64_t)tl && (tl == 0 || memcmp(out, text.data(), tl) == 0) && (flag ? r == IC_OK : r != IC_OK);
    free(out);
    if (!flag) {
      bad++;
      uint32_t isize = 0;
      if (gl >= 4) memcpy(&isize, gz + gl - 4, 4);
      if (isize > (1u << 20)) isize = 1u << 20;
      uint8_t *o2 = (uint8_t *)malloc(isize ? isize : 1);
      const int32_t r2 = ic_inflate_member(gz, gz + gl, o2, isize, w->window, w->crctab, w->dec);
      free(o2);
      printf("bad  %-60s file: %-40s one member: %s\n", name.c_str(), ic_reason_name(r), ic_reason_name(r2));
    } else good++;
    if (!ok) { failed++; printf("FAILED %s: reason %d (%s), %lld of %llu bytes, %lld members\n", name.c_str(), r, ic_reason_name(r), (long long)got, (unsigned long long)tl, (long long)members); }
    free(gz);
  }
  delete w;
  fclose(f);
  printf("%d good, %d bad, %d failed\n", good, bad, failed);
  return failed ? 1 : 0;
}
