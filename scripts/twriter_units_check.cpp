// twriter_units_check.cpp -- a stand-alone check of the streamed writer's device path on the host, meant for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -pthread -I itsxpress_amd/csrc scripts/twriter_units_check.cpp \
//       itsxpress_amd/csrc/trim_host.cpp itsxpress_amd/csrc/fastq_io.cpp itsxpress_amd/csrc/pinflate.cpp itsxpress_amd/csrc/switches.cpp \
//       -lz -ldl -o twriter_units_check
// The writer object of trim_host.cpp is the real one (units, count pass, the device thread, ordered writes, late records); the context
// it borrows is this file's: twriter_dev.h's three calls stated serially -- the line index, the verdict "4 lines per record", the plan
// of both modes and the copy as csrc/k_trim.hip defines them, and zlib for the members.  Every output is inflated and compared with
// the host writer's plain file for the same text and coordinates, so the serial statement is checked against the host slicer and the
// unit bookkeeping runs under the sanitizers with text and coordinates arriving in pieces.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits.h>
#include <mutex>
#include <random>
#include <string>
#include <vector>
#include <zlib.h>
#include "twriter_dev.h"
#include "iupac.h"

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { g_fail++; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct itsx_ctx { std::mutex mu; long units = 0, fitted = 0, texts = 0; };

static const int BLOCK = 65535;
static bool gzip_members(const std::string &text, std::string &comp)
{
  comp.clear();
  for (size_t o = 0; o < text.size(); o += BLOCK) {
    const size_t n = std::min<size_t>(BLOCK, text.size() - o);
    z_stream zs; memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, 1, Z_DEFLATED, 31, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    std::vector<unsigned char> buf(deflateBound(&zs, (uLong)n) + 64);
    zs.next_in = (Bytef *)(text.data() + o); zs.avail_in = (uInt)n;
    zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
    const int rc = deflate(&zs, Z_FINISH);
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) return false;
    comp.append((const char *)buf.data(), zs.total_out);
  }
  return true;
}

// Python's seq[a:b] of a sequence of n, as k_trim.hip's trim_py_slice
static void py_slice(int64_t n, int64_t a, int64_t b, bool open, int64_t &lo, int64_t &sl)
{
  if (a < 0) { a += n; if (a < 0) a = 0; } else if (a > n) a = n;
  if (open) b = n;
  else if (b < 0) { b += n; if (b < 0) b = 0; } else if (b > n) b = n;
  lo = a; sl = b > a ? b - a : 0;
}

namespace itsx {

int twdev_reserve(itsx_ctx *, size_t, std::string &) { return ITSX_OK; }

int twdev_unit(itsx_ctx *ctx, const TwUnit &u, bool &fits, std::string &comp, int64_t &nw, int64_t &tot, std::string &err)
{
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->units++;
  fits = false; nw = tot = 0; comp.clear();
  const char *t = u.text; const int64_t n = (int64_t)u.nbytes, cap = 4 * u.count;
  // the index: the k-th newline ends line k and starts line k + 1; a '\r' before it is not part of the line; an open last line counts
  int64_t lines = 0;
  for (int64_t p = 0; p < n; p++) lines += t[p] == '\n';
  const bool open = n > 0 && t[n - 1] != '\n';
  lines += open ? 1 : 0;
  if (lines != cap) return ITSX_OK;
  std::vector<int32_t> ls((size_t)cap + 1), le((size_t)cap + 1);
  int64_t k = 0;
  ls[0] = 0;
  for (int64_t p = 0; p < n; p++)
    if (t[p] == '\n') { le[(size_t)k] = (int32_t)(p - ((p > 0 && t[p - 1] == '\r') ? 1 : 0)); ls[(size_t)k + 1] = (int32_t)(p + 1); k++; }
  if (open) le[(size_t)k] = (int32_t)(n - (t[n - 1] == '\r' ? 1 : 0));
  // the plan and the copy
  static const char *fwd = "GACAGGTACAAGAAGGA", *rev = "TTAACCCAGTCTCCAGT";
  std::string out;
  for (int64_t r = 0; r < u.count; r++) {
    const int32_t t0 = ls[4 * r], s0 = ls[4 * r + 1], p0 = ls[4 * r + 2], q0 = ls[4 * r + 3];
    const int32_t tl = le[4 * r] - t0, L = le[4 * r + 1] - s0, pl = le[4 * r + 2] - p0, ql = le[4 * r + 3] - q0;
    if (tl <= 0 || t[t0] != '@' || pl <= 0 || t[p0] != '+' || ql != L) return ITSX_OK;      // not a record: the host names it
    const int64_t s = u.start[r], e = u.stop[r];
    bool w; int64_t lo, sl;
    if (u.mode == 1) { w = e != INT32_MIN; py_slice(L, s, e, e == INT32_MAX, lo, sl); }
    else { w = s >= 0 && e >= 0 && s < e; py_slice(L, s, e, false, lo, sl); }
    if (!w) continue;
    // a record of strand -1 (itsx_twriter_strands): output byte p of the slice is source byte L - 1 - (lo + p), a base complemented
    const bool flip = u.strand && u.mode == 0 && u.strand[r] < 0;
    std::string fs, fq;
    if (flip) {
      const char *comp = iupac_complement();
      for (int64_t p = 0; p < sl; p++) { fs += comp[(unsigned char)t[s0 + L - 1 - (lo + p)]]; fq += t[q0 + L - 1 - (lo + p)]; }
    }
    out.append(t + t0, (size_t)tl); out += '\n';
    if (u.ccs) out += fwd;
    if (flip) out += fs; else out.append(t + s0 + lo, (size_t)sl);
    if (u.ccs) out += rev;
    out += "\n+\n";
    if (u.ccs) out.append(17, '~');
    if (flip) out += fq; else out.append(t + q0 + lo, (size_t)sl);
    if (u.ccs) out.append(17, '~');
    out += '\n';
    nw++; tot += sl + (u.ccs ? 34 : 0);
  }
  fits = true;
  ctx->fitted++;
  if (!out.empty() && !gzip_members(out, comp)) { err = "zlib"; return ITSX_E_DEVICE; }
  return ITSX_OK;
}

int twdev_text(itsx_ctx *ctx, const char *text, size_t nbytes, std::string &comp, std::string &err)
{
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->texts++;
  if (!gzip_members(std::string(text, nbytes), comp)) { err = "zlib"; return ITSX_E_DEVICE; }
  return ITSX_OK;
}

}  // namespace itsx

static std::string slurp(const std::string &path, bool gz)
{
  std::string out; char buf[1 << 16];
  if (gz) {
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return out;
    int n;
    while ((n = gzread(f, buf, sizeof(buf))) > 0) out.append(buf, (size_t)n);
    if (n < 0) { g_fail++; fprintf(stderr, "FAIL: %s does not inflate\n", path.c_str()); }
    gzclose(f);
  } else {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return out;
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);
    fclose(f);
  }
  return out;
}

struct Input { std::string text; std::vector<size_t> ends; std::vector<int32_t> len; };

static Input make_text(std::mt19937 &rng, int n, bool open_end)
{
  Input in;
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo)); };
  for (int i = 0; i < n; i++) {
    int ln = rnd(30, 300);
    if (i % 37 == 5) ln = 0;                                   // reads of 0 bases
    if (i == n / 2) ln = 40000;                                // longer than a unit
    if (i == n / 3) ln = 70000;                                // its output crosses a member
    const char *nl = (i % 5 == 1) ? "\r\n" : "\n";
    if (i > n / 4 && i < n / 4 + 30 && i % 3 == 0) in.text += (i % 2) ? "\n" : "\r\n\n";      // blank lines between records
    std::string seq((size_t)ln, 'A'), qual((size_t)ln, 'I');
    for (int k = 0; k < ln; k++) { seq[(size_t)k] = "ACGT"[rng() & 3]; qual[(size_t)k] = "@+IF#5~"[rng() % 7]; }
    const std::string title = "@r" + std::to_string(i) + " w";
    in.text += title + nl + seq + nl + ((i % 7 == 2) ? "+" + title.substr(1) : std::string("+")) + nl + qual + nl;
    in.ends.push_back(in.text.size()); in.len.push_back(ln);
  }
  if (open_end) { in.text.pop_back(); in.ends.back() = in.text.size(); }
  else in.text += "\n\r\n\n";
  return in;
}

static void coords(std::mt19937 &rng, const Input &in, int mode, std::vector<int32_t> &a, std::vector<int32_t> &b)
{
  const size_t n = in.len.size();
  a.resize(n); b.resize(n);
  for (size_t i = 0; i < n; i++) {
    const int L = in.len[i], kind = (int)(rng() % 10);
    int64_t s = (int64_t)(rng() % 60), e = s + 1 + (int64_t)(rng() % 300);
    if (mode == 0) {
      if (kind == 0) s = -1 - (int64_t)(rng() % 50);
      if (kind == 1) e = -1 - (int64_t)(rng() % 50);
      if (kind == 2) e = s;
      if (kind == 3) e = s - 1;
      if (kind == 4) e = L + 1 + (int64_t)(rng() % 1000);
      if (kind == 5) { s = L + 5; e = L + 9; }
      if (i + 200 > n && i + 60 < n) s = e = -1;               // whole units without a surviving record
    } else {
      s = (int64_t)(rng() % 700) - 400; e = (int64_t)(rng() % 900) - 400;
      if (kind == 0) s = -L - 1 - (int64_t)(rng() % 100);
      if (kind == 1) e = INT32_MAX;
      if (kind == 2) e = INT32_MIN;
      if (kind == 3) e = s - 1 - (int64_t)(rng() % 30);
      if (kind == 4) s = INT32_MIN;
      if (i + 200 > n && i + 60 < n) e = INT32_MIN;
    }
    if (L >= 40000) { s = 3; e = mode ? INT32_MAX : 1000000; }
    a[i] = (int32_t)s; b[i] = (int32_t)e;
  }
}

// the writer fed in pieces (rhythm < 0: all at once), with late records; returns the close code
static int feed(const std::string &path, const Input &in, const std::vector<int32_t> &a, const std::vector<int32_t> &b, int kind, int ccs, int mode,
                int rhythm, itsx_ctx *ctx, int64_t *nw, int64_t *tot, const std::vector<int8_t> *sd = nullptr)
{
  itsx_twriter *w = nullptr;
  if (itsx_twriter_open(path.c_str(), kind, ccs, &w) != ITSX_OK) return -100;
  if (mode) CHECK(itsx_twriter_set_mode(w, mode) == ITSX_OK, "set_mode");
  if (ctx) CHECK(itsx_twriter_set_device(w, ctx) == ITSX_OK, "set_device: %s", itsx_trim_last_error());
  const int64_t n = (int64_t)in.len.size();
  if (rhythm < 0) {
    if (sd) CHECK(itsx_twriter_strands(w, 0, n, sd->data()) == ITSX_OK, "strands: %s", itsx_trim_last_error());
    CHECK(itsx_twriter_text(w, in.text.data(), (int64_t)in.text.size(), 1) == ITSX_OK, "text");
    CHECK(itsx_twriter_coords(w, 0, n, a.data(), b.data(), nullptr) == ITSX_OK, "coords");
  } else {
    std::mt19937 rng(100 + (unsigned)rhythm);
    std::vector<uint8_t> dec((size_t)n, 1); std::vector<int32_t> wrong(a);
    std::vector<int64_t> late;
    for (int64_t i = 0; i < n; i++) if (rhythm > 0 && rng() % (rhythm == 1 ? 100 : 12) == 0) { dec[(size_t)i] = 0; wrong[(size_t)i] = 7; late.push_back(i); }
    int64_t lo = 0;
    for (int piece = 0; lo < n; piece++) {
      const int64_t hi = std::min<int64_t>(n, lo + 1 + (int64_t)(rng() % (unsigned)(n / 3)));
      const int64_t upto = hi == n ? (int64_t)in.text.size() : (int64_t)in.ends[(size_t)hi - 1];
      if (sd) CHECK(itsx_twriter_strands(w, lo, hi - lo, sd->data() + lo) == ITSX_OK, "strands: %s", itsx_trim_last_error());
      for (int step = 0; step < 2; step++) {
        if ((step + piece + rhythm) % 2 == 0) CHECK(itsx_twriter_text(w, in.text.data(), upto, hi == n) == ITSX_OK, "text: %s", itsx_trim_last_error());
        else CHECK(itsx_twriter_coords(w, lo, hi - lo, wrong.data() + lo, b.data() + lo, dec.data() + lo) == ITSX_OK, "coords: %s", itsx_trim_last_error());
      }
      lo = hi;
    }
    std::vector<int32_t> la, lb;
    for (int64_t i : late) { la.push_back(a[(size_t)i]); lb.push_back(b[(size_t)i]); }
    CHECK(itsx_twriter_update(w, late.data(), (int64_t)late.size(), la.data(), lb.data()) == ITSX_OK, "update");
  }
  return itsx_twriter_close(w, nw, tot);
}

int main()
{
  setenv("ITSX_WRITE_UNIT_KB", "16", 1);
  setenv("ITSX_IO_THREADS", "4", 1);
  const std::string dir = getenv("TMPDIR") ? getenv("TMPDIR") : "/tmp";
  const std::string model = dir + "/twriter_units_check.model", out = dir + "/twriter_units_check.out.gz";
  std::mt19937 rng(7);
  itsx_ctx ctx;
  for (int open_end = 0; open_end < 2; open_end++) {
    const Input in = make_text(rng, 700, open_end != 0);
    for (int mode = 0; mode < 2; mode++)
      for (int ccs = 0; ccs < (mode ? 1 : 2); ccs++) {
        std::vector<int32_t> a, b;
        coords(rng, in, mode, a, b);
        int64_t mw = 0, mt = 0;
        CHECK(feed(model, in, a, b, 0, ccs, mode, -1, nullptr, &mw, &mt) == ITSX_OK, "model: %s", itsx_trim_last_error());
        const std::string want = slurp(model, false);
        CHECK(mw > 100 && want.size() > 100000, "the model writes %lld records", (long long)mw);
        for (int rhythm = -1; rhythm < 3; rhythm++) {
          int64_t nw = 0, tot = 0;
          CHECK(feed(out, in, a, b, 1, ccs, mode, rhythm, &ctx, &nw, &tot) == ITSX_OK, "device writer: %s", itsx_trim_last_error());
          CHECK(nw == mw && tot == mt, "counts %lld %lld, model %lld %lld", (long long)nw, (long long)tot, (long long)mw, (long long)mt);
          CHECK(slurp(out, true) == want, "open_end %d mode %d ccs %d rhythm %d: the output differs from the host model", open_end, mode, ccs, rhythm);
        }
      }
    // strands (mode 0): the host writer's plain file with the strands is the model of the device thread's units; and that model differs
    // from the file without strands, and equals it where every strand is +1 or 0
    for (int ccs = 0; ccs < 2; ccs++) {
      std::vector<int32_t> a, b;
      coords(rng, in, 0, a, b);
      std::vector<int8_t> sd(in.len.size()), none(in.len.size());
      for (size_t i = 0; i < sd.size(); i++) { sd[i] = (int8_t)((int)(rng() % 3) - 1); none[i] = (int8_t)(rng() & 1); }
      int64_t mw = 0, mt = 0, pw = 0, pt = 0;
      CHECK(feed(model, in, a, b, 0, ccs, 0, -1, nullptr, &pw, &pt) == ITSX_OK, "model without strands: %s", itsx_trim_last_error());
      const std::string plain = slurp(model, false);
      CHECK(feed(model, in, a, b, 0, ccs, 0, 2, nullptr, &mw, &mt, &none) == ITSX_OK, "model, no strand -1: %s", itsx_trim_last_error());
      CHECK(slurp(model, false) == plain, "strands of +1 and 0 change the file");
      CHECK(feed(model, in, a, b, 0, ccs, 0, -1, nullptr, &mw, &mt, &sd) == ITSX_OK, "model with strands: %s", itsx_trim_last_error());
      const std::string want = slurp(model, false);
      CHECK(mw == pw && mt == pt && want.size() == plain.size() && want != plain, "strands change the bytes, not the counts");
      for (int rhythm = -1; rhythm < 3; rhythm++) {
        int64_t nw = 0, tot = 0;
        CHECK(feed(out, in, a, b, 1, ccs, 0, rhythm, &ctx, &nw, &tot, &sd) == ITSX_OK, "device writer with strands: %s", itsx_trim_last_error());
        CHECK(nw == mw && tot == mt, "counts %lld %lld, model %lld %lld", (long long)nw, (long long)tot, (long long)mw, (long long)mt);
        CHECK(slurp(out, true) == want, "open_end %d ccs %d rhythm %d with strands: the output differs from the host model", open_end, ccs, rhythm);
      }
    }
    // malformed text: reported as the host writer reports it
    Input bad = in;
    bad.text += "@broken\nACGT\n+\nII\n"; bad.ends.push_back(bad.text.size()); bad.len.push_back(4);
    std::vector<int32_t> a(bad.len.size(), 0), b(bad.len.size(), 10);
    CHECK(feed(out, bad, a, b, 1, 0, 0, 1, &ctx, nullptr, nullptr) == ITSX_E_FORMAT, "malformed text: %s", itsx_trim_last_error());
  }
  CHECK(ctx.fitted > 100 && ctx.units > ctx.fitted && ctx.texts > 0, "units %ld, fitted %ld, host-sliced texts %ld", ctx.units, ctx.fitted, ctx.texts);
  // arguments
  {
    itsx_twriter *w = nullptr;
    CHECK(itsx_twriter_open(model.c_str(), 0, 0, &w) == ITSX_OK, "open");
    CHECK(itsx_twriter_set_device(w, &ctx) == ITSX_E_ARG, "a plain writer takes no device");
    CHECK(itsx_twriter_set_device(w, nullptr) == ITSX_E_ARG && itsx_twriter_set_device(nullptr, &ctx) == ITSX_E_ARG, "null arguments");
    CHECK(itsx_twriter_text(w, nullptr, 0, 1) == ITSX_OK && itsx_twriter_close(w, nullptr, nullptr) == ITSX_OK, "the writer stays closable");
    CHECK(itsx_twriter_open(out.c_str(), 1, 0, &w) == ITSX_OK, "open");
    CHECK(itsx_twriter_text(w, "@a\nAC\n+\nII\n", 5, 0) == ITSX_OK, "text");
    CHECK(itsx_twriter_set_device(w, &ctx) == ITSX_E_ARG, "a late call");
    CHECK(itsx_twriter_text(w, nullptr, 0, 1) == ITSX_E_ARG, "the text does not move");
    (void)itsx_twriter_close(w, nullptr, nullptr);
    CHECK(itsx_twriter_open(out.c_str(), 3, 0, &w) == ITSX_E_ARG, "compression 3 is refused at open");
    const int8_t one[2] = {-1, 1}; const int32_t z[2] = {0, 0}, e[2] = {2, 2};
    CHECK(itsx_twriter_open(model.c_str(), 0, 0, &w) == ITSX_OK, "open");
    CHECK(itsx_twriter_coords(w, 0, 1, z, e, nullptr) == ITSX_OK && itsx_twriter_strands(w, 0, 2, one) == ITSX_E_ARG, "strands after coordinates");
    CHECK(itsx_twriter_strands(w, 2, 1, one) == ITSX_E_ARG && itsx_twriter_strands(w, 1, 1, one) == ITSX_OK, "strands in record order");
    CHECK(itsx_twriter_set_mode(w, 1) == ITSX_E_ARG, "a writer with strands takes no mode 1");
    CHECK(itsx_twriter_coords(w, 1, 1, z, e, nullptr) == ITSX_OK && itsx_twriter_text(w, "@a\nAC\n+\nIJ\n@b\nAC\n+\nIJ\n", 22, 1) == ITSX_OK, "text");
    CHECK(itsx_twriter_close(w, nullptr, nullptr) == ITSX_OK && slurp(model, false) == "@a\nAC\n+\nIJ\n@b\nGT\n+\nJI\n", "a late first row");
    CHECK(itsx_twriter_open(model.c_str(), 0, 0, &w) == ITSX_OK && itsx_twriter_set_mode(w, 1) == ITSX_OK, "open");
    CHECK(itsx_twriter_strands(w, 0, 2, one) == ITSX_E_ARG, "a mode-1 writer takes no strands");
    CHECK(itsx_twriter_text(w, nullptr, 0, 1) == ITSX_OK && itsx_twriter_close(w, nullptr, nullptr) == ITSX_OK, "close");
  }
  remove(model.c_str()); remove(out.c_str());
  printf("%s: %ld units, %ld through the index, %ld host-sliced texts\n", g_fail ? "FAILED" : "ok", ctx.units, ctx.fitted, ctx.texts);
  return g_fail ? 1 : 0;
}
