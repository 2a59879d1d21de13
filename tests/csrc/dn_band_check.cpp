// dn_band_check.cpp -- k_dn_band.h (the banded bit-vector distance of csrc/k_denoise.hip) held to a full Levenshtein matrix on the host:
// random pairs of related and unrelated strings, every cut-off from the length difference to 31, the match table in one piece and in
// 64-column windows.  dn_band_check [PAIRS]; prints `ok N` (N = (pair, cut-off) cases) or the first mismatch.  tests/test_denoise_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <algorithm>
#include <random>
#include "k_dn_band.h"
using namespace itsx;

static int lev(const std::string &a, const std::string &b)
{
  std::vector<int> p(b.size() + 1), c(b.size() + 1);
  for (size_t j = 0; j <= b.size(); j++) p[j] = (int)j;
  for (size_t i = 1; i <= a.size(); i++) {
    c[0] = (int)i;
    for (size_t j = 1; j <= b.size(); j++) c[j] = std::min({p[j - 1] + (a[i - 1] != b[j - 1]), p[j] + 1, c[j - 1] + 1});
    p.swap(c);
  }
  return p[b.size()];
}
// the kernel's way: windowed table; CH columns per window
static int banded(const std::string &q, const std::string &t, int k, int CH)
{
  const int m = (int)q.size(), n = (int)t.size();
  const int NW = CH / 64 + 3;
  std::vector<uint64_t> tab((size_t)16 * NW);
  DnBand s; dn_band_init(s, k, m, n);
  for (int J0 = 0; J0 < n; J0 += CH) {
    const int base = J0 - 64;
    std::fill(tab.begin(), tab.end(), 0);
    for (int P = 0; P < NW * 64; P++) { const int p = base + P; if (p >= 0 && p < m) tab[(size_t)dn_code(q[p]) * NW + (P >> 6)] |= 1ull << (P & 63); }
    for (int j = J0 + 1; j <= std::min(n, J0 + CH); j++) {
      const int P = (j - k - 1) - base;
      if (P < 0 || (P >> 6) + 1 >= NW) { printf("P out of range %d\n", P); exit(1); }
      dn_band_step(s, dn_band_eq(&tab[(size_t)dn_code(t[j - 1]) * NW], P));
      if (s.score > k) return -1;
    }
  }
  return s.score <= k ? s.score : -1;
}
int main(int argc, char **argv)
{
  const int pairs = argc > 1 ? atoi(argv[1]) : 400000;
  std::mt19937 rng(5);
  const char *alpha = "ACGTN";
  long checked = 0;
  for (int it = 0; it < pairs; it++) {
    const int m = 1 + rng() % (it % 7 == 0 ? 300 : 40);
    std::string q;
    const int na = 2 + rng() % 4;
    for (int i = 0; i < m; i++) q += alpha[rng() % na];
    std::string t = q;
    const int ne = rng() % 8;
    for (int e = 0; e < ne && !t.empty(); e++) {
      const int op = rng() % 3, at = rng() % (t.size() + (op == 1));
      const int where = rng() % 4;
      const int pos = where == 0 ? 0 : where == 1 ? (int)t.size() - (op != 1) : at;
      if (op == 0) t[pos] = alpha[rng() % na]; else if (op == 1) t.insert(t.begin() + pos, alpha[rng() % na]); else if (t.size() > 1) t.erase(t.begin() + pos);
    }
    if (it % 5 == 0) { t.clear(); const int n = 1 + rng() % 40; for (int i = 0; i < n; i++) t += alpha[rng() % na]; }
    const int d = lev(q, t), dl = std::abs((int)q.size() - (int)t.size());
    for (int k = std::max(dl, 0); k <= 31; k++) {
      if (k == 0 && dl != 0) continue;
      const int CH = (it & 1) ? 64 : 4096;
      const int got = banded(q, t, k, CH), want = d <= k ? d : -1;
      if (got != want) { printf("MISMATCH q=%s t=%s k=%d got %d want %d\n", q.c_str(), t.c_str(), k, got, want); return 1; }
      checked++;
    }
  }
  printf("ok %ld\n", checked);
  return 0;
}
