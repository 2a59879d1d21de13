// writers_host.cpp -- the file-compatible outputs: the --uc / --fastaout files of `vsearch --fastx_uniques` / `--cluster_size`
// (itsxpress/SeqSample.py:104-116, read back by Dedup.parse :542-562) and hmmsearch's --domtblout (SeqSample.py:190-209, read back
// by ItsPosition.parse :431-461).  Host-only text formatting, no arithmetic of the path.
//
// One formatter (writers.h) serves the context's writers (engine.hip) and the array writers below, which a driver that spreads one
// sample over several GPUs (itsxpress_amd/multi.py: ITSXPRESS_GPUS=N) or streams it (stream.py) calls with what it assembled from
// its workers: ONE uc.txt / rep.fa / domtbl.txt, byte for byte the files one GPU writes.
#include "writers.h"
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include "detmath.h"
#include "fastq_io.h"

namespace itsx {

std::string Labels::operator()(int64_t i) const
{
  if (offs) return std::string(blob + offs[i], (size_t)(offs[i + 1] - offs[i]));
  char b[32]; snprintf(b, sizeof(b), "r%09lld", (long long)i); return b;
}

namespace {

__attribute__((format(printf, 2, 3))) void appendf(std::string &out, const char *fmt, ...)
{
  char line[1024];
  va_list a, b;
  va_start(a, fmt); va_copy(b, a);
  const int len = vsnprintf(line, sizeof(line), fmt, a);
  if (len >= 0 && (size_t)len < sizeof(line)) out.append(line, (size_t)len);
  else if (len >= 0) {                                  // (labels longer than the line buffer)
    const size_t o = out.size();
    out.resize(o + (size_t)len + 1);
    vsnprintf(&out[o], (size_t)len + 1, fmt, b);
    out.resize(o + (size_t)len);
  }
  va_end(b); va_end(a);
}

// blocks of a text file formatted by a pool of threads while this thread writes the finished ones in order (a few blocks ahead at
// most).  A truncated file would silently shorten what the reference's parsers read (vsearch / hmmsearch exit non-zero on a full
// disk): any failed write, ferror or fclose is an error.
int write_blocks(const char *path, size_t nb, const std::function<void(size_t, std::string &)> &format_block, std::string &err)
{
  FILE *f = fopen(path, "w");
  if (!f) { err = std::string("cannot write ") + path; return ITSX_E_IO; }
  const int T = (int)std::min<size_t>((size_t)itsx_io::io_threads(), std::max<size_t>(nb, 1));
  bool io_ok = true;
  if (T <= 1 || nb <= 1) {
    std::string out;
    for (size_t b = 0; b < nb; b++) { out.clear(); format_block(b, out); if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) io_ok = false; }
  } else {
    std::vector<std::string> blocks(nb);
    std::vector<char> ready(nb, 0);
    std::mutex mu; std::condition_variable cv;
    size_t next = 0, written = 0;
    const size_t ahead = (size_t)T * 4;
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
      th.emplace_back([&] {
        for (;;) {
          size_t b;
          {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return next >= nb || next < written + ahead; });
            if (next >= nb) return;
            b = next++;
          }
          std::string out;
          out.reserve(32768 * 200);
          format_block(b, out);
          { std::lock_guard<std::mutex> lk(mu); blocks[b].swap(out); ready[b] = 1; }
          cv.notify_all();
        }
      });
    for (size_t b = 0; b < nb; b++) {
      std::string out;
      { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return ready[b] != 0; }); out.swap(blocks[b]); }
      if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size()) io_ok = false;
      { std::lock_guard<std::mutex> lk(mu); written = b + 1; }
      cv.notify_all();
    }
    for (auto &x : th) x.join();
  }
  if (ferror(f) != 0) io_ok = false;
  if (fclose(f) != 0) io_ok = false;
  if (!io_ok) { err = std::string("short write to ") + path; return ITSX_E_IO; }
  return ITSX_OK;
}

// H rows of exact dereplication print the literal 100.0, which is what %.1f makes of 100.0
void s_row(std::string &out, size_t c, int32_t len, const std::string &label) { appendf(out, "S\t%zu\t%d\t*\t*\t*\t*\t*\t%s\t*\n", c, len, label.c_str()); }
void h_row(std::string &out, size_t c, int32_t len, double pct, int8_t strand, const std::string &label, const std::string &seed)
{
  appendf(out, "H\t%zu\t%d\t%.1f\t%c\t0\t0\t*\t%s\t%s\n", c, len, pct, strand < 0 ? '-' : '+', label.c_str(), seed.c_str());
}
// the same row with the member's alignment in column 8 (an alignment of a long read is longer than appendf's line)
void h_row_cigar(std::string &out, size_t c, int32_t len, double pct, int8_t strand, const char *cigar, size_t ncigar, const std::string &label, const std::string &seed)
{
  appendf(out, "H\t%zu\t%d\t%.1f\t%c\t0\t0\t", c, len, pct, strand < 0 ? '-' : '+');
  out.append(cigar, ncigar);
  out.push_back('\t'); out.append(label); out.push_back('\t'); out.append(seed); out.push_back('\n');
}

}  // namespace

void cluster_order(const Clusters &c, std::vector<int32_t> &ord)
{
  ord.clear();
  ord.reserve((size_t)c.U);
  if (c.order) {
    for (int64_t i = 0; i < c.n_order; i++) {
      const int32_t r = c.order[i], u = c.uniq_of[r];
      if (c.seed_read[u] == r && (c.sel < 0 || c.sample[r] == c.sel)) ord.push_back(u);
    }
    return;
  }
  for (int32_t u = 0; u < c.U; u++) if (c.sel < 0 || c.usample[u] == c.sel) ord.push_back(u);
  std::vector<std::string> lab((size_t)c.U);
  const int T = c.U >= (1 << 17) ? std::max(1, std::min(16, itsx_io::io_threads())) : 1;
  itsx_io::on_threads(T, [&](int t) { for (int64_t u = (int64_t)c.U * t / T, hi = (int64_t)c.U * (t + 1) / T; u < hi; u++) lab[(size_t)u] = c.labels(c.seed_read[u]); });
  auto before = [&](int32_t a, int32_t b) {
    if (c.abund[a] != c.abund[b]) return c.abund[a] > c.abund[b];
    return strcmp(lab[(size_t)a].c_str(), lab[(size_t)b].c_str()) < 0;
  };
  // a stable sort in pieces (6 M labels of a 10 M-read sample: seconds on one thread): every thread orders its share, neighbouring
  // shares are merged pairwise -- std::inplace_merge keeps equal elements in order, so the result is std::stable_sort's
  const size_t n = ord.size();
  std::vector<size_t> cut((size_t)T + 1);
  for (int t = 0; t <= T; t++) cut[(size_t)t] = n * (size_t)t / (size_t)T;
  itsx_io::on_threads(T, [&](int t) { std::stable_sort(ord.begin() + (ptrdiff_t)cut[(size_t)t], ord.begin() + (ptrdiff_t)cut[(size_t)t + 1], before); });
  for (int w = 1; w < T; w *= 2) {
    std::vector<int> lefts;
    for (int t = 0; t + w < T; t += 2 * w) lefts.push_back(t);
    itsx_io::on_threads((int)lefts.size(), [&](int k) {
      const int t = lefts[(size_t)k];
      std::inplace_merge(ord.begin() + (ptrdiff_t)cut[(size_t)t], ord.begin() + (ptrdiff_t)cut[(size_t)(t + w)], ord.begin() + (ptrdiff_t)cut[(size_t)std::min(T, t + 2 * w)], before);
    });
  }
}

int write_uc(const char *path, const Clusters &c, const std::vector<int32_t> &ord, std::string &err)
{
  const size_t BLK = 16384, nbc = (ord.size() + BLK - 1) / BLK;
  auto c_rows = [&](size_t b, std::string &out) {
    for (size_t k = b * BLK; k < std::min(ord.size(), (b + 1) * BLK); k++)
      appendf(out, "C\t%zu\t%d\t*\t*\t*\t*\t*\t%s\t*\n", k, c.abund[ord[k]], c.labels(c.seed_read[ord[k]]).c_str());
  };
  if (c.order) {
    // vsearch --cluster_size writes the S and H rows as the queries are processed, then one C row per cluster
    std::vector<int32_t> cno((size_t)c.U);
    for (size_t k = 0; k < ord.size(); k++) cno[(size_t)ord[k]] = (int32_t)k;
    const size_t RBLK = 65536, nbr = (size_t)(c.n_order + (int64_t)RBLK - 1) / RBLK;
    return write_blocks(path, nbr + nbc, [&](size_t b, std::string &out) {
      if (b >= nbr) { c_rows(b - nbr, out); return; }
      for (int64_t i = (int64_t)(b * RBLK); i < std::min(c.n_order, (int64_t)((b + 1) * RBLK)); i++) {
        const int32_t r = c.order[i];
        if (c.sel >= 0 && c.sample[r] != c.sel) continue;
        const int32_t u = c.uniq_of[r], s = c.seed_read[u];
        if (s == r) s_row(out, (size_t)cno[(size_t)u], c.len[r], c.labels(r));
        else if (c.cigar_off && c.cigar_off[r + 1] > c.cigar_off[r])
          h_row_cigar(out, (size_t)cno[(size_t)u], c.len[r], c.pct[r], c.strand[r], c.cigar_text + c.cigar_off[r], (size_t)(c.cigar_off[r + 1] - c.cigar_off[r]), c.labels(r), c.labels(s));
        else h_row(out, (size_t)cno[(size_t)u], c.len[r], c.pct[r], c.strand[r], c.labels(r), c.labels(s));
      }
    }, err);
  }
  // the members of every cluster in input order (a counting sort by cluster), then blocks of clusters formatted by the pool: the S row
  // and the H rows of a cluster, cluster after cluster, then the C rows (10 M reads: 16 M lines)
  std::vector<int64_t> mstart((size_t)c.U + 1, 0);
  for (int64_t r = 0; r < c.n; r++) { const int32_t u = c.uniq_of[r]; if (u >= 0 && c.seed_read[u] != r) mstart[(size_t)u + 1]++; }
  for (int32_t u = 0; u < c.U; u++) mstart[(size_t)u + 1] += mstart[(size_t)u];
  std::vector<int64_t> member((size_t)mstart[(size_t)c.U]);
  {
    std::vector<int64_t> cur(mstart.begin(), mstart.end() - 1);
    for (int64_t r = 0; r < c.n; r++) { const int32_t u = c.uniq_of[r]; if (u >= 0 && c.seed_read[u] != r) member[(size_t)cur[(size_t)u]++] = r; }
  }
  return write_blocks(path, 2 * nbc, [&](size_t b, std::string &out) {
    if (b >= nbc) { c_rows(b - nbc, out); return; }
    for (size_t k = b * BLK; k < std::min(ord.size(), (b + 1) * BLK); k++) {
      const int32_t u = ord[k], s = c.seed_read[u];
      const std::string sl = c.labels(s);
      s_row(out, k, c.len[s], sl);
      for (int64_t m = mstart[(size_t)u]; m < mstart[(size_t)u + 1]; m++) {
        const int64_t r = member[(size_t)m];
        h_row(out, k, c.len[r], 100.0, c.strand[r], c.labels(r), sl);
      }
    }
  }, err);
}

int write_rep_fasta(const char *path, const Clusters &c, const std::vector<int32_t> &ord, const Seqs &seqs, std::string &err)
{
  const size_t BLK = 8192, nb = (ord.size() + BLK - 1) / BLK;
  return write_blocks(path, nb, [&](size_t bk, std::string &out) {
    for (size_t k = bk * BLK; k < std::min(ord.size(), (bk + 1) * BLK); k++) {
      const int32_t u = ord[k], s = c.seed_read[u];
      out.push_back('>'); out.append(c.labels(s)); out.push_back('\n');
      const int64_t o = seqs.per_unique ? seqs.off[u] : seqs.off[s], L = seqs.per_unique ? seqs.off[u + 1] - o : c.len[s];
      for (int64_t i = 0; i < L; i += 80) { out.append(seqs.bases + o + i, (size_t)std::min<int64_t>(80, L - i)); out.push_back('\n'); }
    }
  }, err);
}

int write_domtbl(const char *path, const DomTable &t, std::string &err)
{
  const itsx_domain *D = t.rows;
  // one (profile, target) group is formatted on its own, so the table is cut into blocks of whole groups
  std::vector<size_t> cut(1, 0);
  {
    size_t i = 0, last = 0;
    while (i < t.n) {
      size_t j = i;
      while (j < t.n && D[j].prof == D[i].prof && D[j].rep == D[i].rep) j++;
      if (j - last >= 32768) { cut.push_back(j); last = j; }
      i = j;
    }
    if (cut.back() != t.n) cut.push_back(t.n);
  }
  std::vector<std::string> pname((size_t)t.P);
  for (int32_t p = 0; p < t.P; p++) pname[(size_t)p] = t.prof_names(p);
  return write_blocks(path, cut.size(), [&](size_t b, std::string &out) {
    if (b == 0) {
      out += "#                                                                            --- full sequence --- -------------- this domain -------------   hmm coord   ali coord   env coord\n";
      out += "# target name        accession   tlen query name           accession   qlen   E-value  score  bias   #  of  c-Evalue  i-Evalue  score  bias  from    to  from    to  from    to  acc description of target\n";
      return;
    }
    size_t i = cut[b - 1];
    const size_t end = cut[b];
    while (i < end) {
      // a row is reported when dom_reported == 1.  Only 0 and 1 reach a writer: itsx_search_finalize's k_finalize writes 0 or 1, and
      // the compact / lazy rows fetch_domains serves are the reported ones (a lazy search's undecided 2 is refused while pending).
      size_t j = i; int nrep = 0;
      while (j < end && D[j].prof == D[i].prof && D[j].rep == D[i].rep) { nrep += D[j].dom_reported == 1; j++; }
      const int32_t smp = t.usample ? t.usample[D[i].rep] : 0;
      if (nrep == 0 || (t.sel >= 0 && smp != t.sel)) { i = j; continue; }
      const std::string tname = t.targets(t.seed_read ? (int64_t)t.seed_read[D[i].rep] : D[i].rep);
      const int p = D[i].prof;
      const double Z = (double)t.Z[smp], dz = (double)t.domz[(size_t)smp * (size_t)t.P + (size_t)p];
      int k = 0;
      for (size_t d = i; d < j; d++) {
        if (D[d].dom_reported != 1) continue;
        k++;
        const double seqE = Z * det_exp(exp_logsurv((double)D[d].seq_score, (double)t.tau[p], (double)t.lambda[p]));
        const double P = det_exp(D[d].lnP);
        // hmm/ali coordinates and acc come from the optimal-accuracy alignment where the caller has one for the row (itsx_align_domains);
        // without it the envelope coordinates are written in their place (the reference reads only env coords and the score).
        int hf = 1, ht = t.M[p], af = D[d].ienv, at = D[d].jenv; double acc = 0.0;
        if (t.ali && t.ali[d].aligned == 1) {
          const itsx_alignment &A = t.ali[d];
          hf = A.hmm_from; ht = A.hmm_to; af = A.ali_from; at = A.ali_to;
          acc = (double)A.oasc / (1.0 + std::fabs((double)(D[d].jenv - D[d].ienv)));
        }
        appendf(out, "%-20s %-10s %5d %-20s %-10s %5d %9.2g %6.1f %5.1f %3d %3d %9.2g %9.2g %6.1f %5.1f %5d %5d %5d %5d %5d %5d %4.2f %s\n",
                tname.c_str(), "-", D[d].tlen, pname[(size_t)p].c_str(), "-", t.M[p], seqE, D[d].seq_score, D[d].seq_bias,
                k, nrep, P * dz, P * Z, D[d].bitscore, D[d].dombias / 0.69314718055994529, hf, ht, af, at, D[d].ienv, D[d].jenv, acc, "-");
      }
      i = j;
    }
  }, err);
}

}  // namespace itsx

namespace {
std::string g_wr_error;
int fail(int code, const std::string &m) { g_wr_error = m; return code; }
}  // namespace

extern "C" {

const char *itsx_writers_last_error(void) { return g_wr_error.c_str(); }

// uc.txt and rep.fa of exact dereplication from per-read arrays: rep_of[i] = read index of the cluster's seed (its first
// occurrence; -1 = the read was dropped), strand[i] = +1 / -1 relative to the seed, len[i]; names (NULL: r%09d); the seeds'
// sequences concatenated in INPUT order of the seeds (seed_offs[n_seeds + 1]).  Either path may be NULL.
// The clusters are numbered by their seeds' input order, as one context numbers them.
int itsx_write_derep_arrays(const char *uc_path, const char *rep_path, int64_t n, const int64_t *rep_of, const int8_t *strand,
                            const int32_t *len, const char *names, const int64_t *name_offsets, const char *seed_bases,
                            const int64_t *seed_offs, int64_t n_seeds)
{
  if (n < 0 || (n > 0 && (!rep_of || !strand || !len))) return fail(ITSX_E_ARG, "itsx_write_derep_arrays: missing arrays");
  if (n > INT32_MAX) return fail(ITSX_E_ARG, "itsx_write_derep_arrays: more than 2^31 - 1 reads");
  std::vector<int32_t> uniq_of((size_t)n, -1), seed_read;
  for (int64_t r = 0; r < n; r++) if (rep_of[r] == r) { uniq_of[(size_t)r] = (int32_t)seed_read.size(); seed_read.push_back((int32_t)r); }
  const int64_t U = (int64_t)seed_read.size();
  if (rep_path && U != n_seeds) return fail(ITSX_E_ARG, "itsx_write_derep_arrays: " + std::to_string(U) + " seeds in rep_of, " + std::to_string(n_seeds) + " sequences given");
  std::vector<int32_t> abund((size_t)U, 0);
  for (int64_t r = 0; r < n; r++) {
    const int64_t s = rep_of[r];
    if (s < 0) continue;
    if (s >= n || rep_of[s] != s) return fail(ITSX_E_ARG, "itsx_write_derep_arrays: rep_of[" + std::to_string(r) + "] is not a seed");
    uniq_of[(size_t)r] = uniq_of[(size_t)s];
    abund[(size_t)uniq_of[(size_t)s]]++;
  }
  itsx::Clusters c;
  c.n = n; c.U = (int32_t)U; c.uniq_of = uniq_of.data(); c.seed_read = seed_read.data(); c.abund = abund.data(); c.len = len; c.strand = strand;
  if (names && name_offsets) c.labels = itsx::Labels{names, name_offsets};
  std::vector<int32_t> ord;
  itsx::cluster_order(c, ord);
  std::string err;
  if (uc_path && itsx::write_uc(uc_path, c, ord, err) != ITSX_OK) return fail(ITSX_E_IO, err);
  if (rep_path) {
    if (U > 0 && (!seed_bases || !seed_offs)) return fail(ITSX_E_ARG, "itsx_write_derep_arrays: rep.fa needs the seeds' sequences");
    if (itsx::write_rep_fasta(rep_path, c, ord, itsx::Seqs{seed_bases, seed_offs, true}, err) != ITSX_OK) return fail(ITSX_E_IO, err);
  }
  return ITSX_OK;
}

// domtbl.txt from domain rows gathered from several contexts: rows[n_rows] with rep = index into target_names (the GLOBAL unique
// list, input order of the seeds), any order (sorted here: profile, target, domain -- the context writer's order); dom_reported
// as itsx_search_finalize left it.  Z = targets searched (hmmsearch's Z: the global number of uniques), domz[n_profiles] = the
// data set's reported targets per profile; per profile its NAME, length M and the Forward tail (tau, lambda) for the E-value columns.
int itsx_write_domtbl_arrays_ali(const char *path, const itsx_domain *rows, int64_t n_rows, int64_t Z, const int64_t *domz, int32_t n_profiles,
                                 const char *prof_names, const int64_t *prof_name_offsets, const int32_t *prof_M, const float *prof_tau,
                                 const float *prof_lambda, const char *target_names, const int64_t *target_name_offsets,
                                 const itsx_alignment *ali)
{
  if (!path || n_rows < 0 || (n_rows > 0 && !rows) || n_profiles < 0 || (n_profiles > 0 && (!domz || !prof_names || !prof_name_offsets || !prof_M || !prof_tau || !prof_lambda)))
    return fail(ITSX_E_ARG, "itsx_write_domtbl_arrays: missing arrays");
  std::vector<itsx_domain> D;
  D.reserve((size_t)n_rows);
  std::vector<int64_t> src;                       // with alignments: the input row of every kept row, carried through the same sort
  for (int64_t i = 0; i < n_rows; i++) if (rows[i].dom_idx >= 0 && rows[i].prof >= 0 && rows[i].prof < n_profiles) { D.push_back(rows[i]); if (ali) src.push_back(i); }
  auto before = [](const itsx_domain &a, const itsx_domain &b) {
    if (a.prof != b.prof) return a.prof < b.prof;
    if (a.rep != b.rep) return a.rep < b.rep;
    return a.dom_idx < b.dom_idx;
  };
  std::vector<itsx_alignment> A;
  if (!ali) std::stable_sort(D.begin(), D.end(), before);
  else {
    std::vector<size_t> ord(D.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return before(D[x], D[y]); });
    std::vector<itsx_domain> Ds(D.size());
    A.resize(D.size());
    for (size_t i = 0; i < ord.size(); i++) { Ds[i] = D[ord[i]]; A[i] = ali[src[ord[i]]]; }
    D.swap(Ds);
  }
  itsx::DomTable t;
  t.rows = D.data(); t.n = D.size(); t.P = n_profiles;
  t.prof_names = itsx::Labels{prof_names, prof_name_offsets}; t.M = prof_M; t.tau = prof_tau; t.lambda = prof_lambda;
  t.Z = &Z; t.domz = domz;
  if (ali) t.ali = A.data();
  if (target_names && target_name_offsets) t.targets = itsx::Labels{target_names, target_name_offsets};
  std::string err;
  if (itsx::write_domtbl(path, t, err) != ITSX_OK) return fail(ITSX_E_IO, err);
  return ITSX_OK;
}

int itsx_write_domtbl_arrays(const char *path, const itsx_domain *rows, int64_t n_rows, int64_t Z, const int64_t *domz, int32_t n_profiles,
                             const char *prof_names, const int64_t *prof_name_offsets, const int32_t *prof_M, const float *prof_tau,
                             const float *prof_lambda, const char *target_names, const int64_t *target_name_offsets)
{
  return itsx_write_domtbl_arrays_ali(path, rows, n_rows, Z, domz, n_profiles, prof_names, prof_name_offsets, prof_M, prof_tau, prof_lambda,
                                      target_names, target_name_offsets, nullptr);
}

// The two files of a feature table (itsx_trimmed_table's arrays): blocks of features through write_blocks, like every other file here.
int itsx_write_feature_files(const char *fasta_path, const char *tsv_path, int64_t n_features, int32_t n_samples, const int32_t *feat_total,
                             const int32_t *feat_first_read, const int64_t *row_off, const int32_t *entry_sample, const int32_t *entry_count,
                             const char *bases, const int64_t *offsets, const char *labels, const int64_t *label_offsets,
                             const char *read_names, const int64_t *read_name_offsets, const char *sample_names,
                             const int64_t *sample_name_offsets)
{
  const int64_t F = n_features;
  if (F < 0 || n_samples < 0 || (F > 0 && (!feat_total || !feat_first_read))) return fail(ITSX_E_ARG, "itsx_write_feature_files: missing arrays");
  if (fasta_path && F > 0 && (!bases || !offsets)) return fail(ITSX_E_ARG, "itsx_write_feature_files: the FASTA needs the features' sequences");
  if (tsv_path && F > 0 && (!row_off || (row_off[F] > 0 && (!entry_sample || !entry_count)))) return fail(ITSX_E_ARG, "itsx_write_feature_files: the table needs its entries");
  if (tsv_path && F > 0)
    for (int64_t e = 0; e < row_off[F]; e++)
      if (entry_sample[e] < 0 || entry_sample[e] >= n_samples) return fail(ITSX_E_ARG, "itsx_write_feature_files: entry " + std::to_string(e) + " names sample " + std::to_string(entry_sample[e]) + " of " + std::to_string(n_samples));
  const itsx::Labels given{labels, label_offsets}, reads{read_names, read_name_offsets};
  auto label = [&](int64_t f) -> std::string {
    if (labels && label_offsets) return given(f);
    std::string id = reads(feat_first_read[f]);             // (without names: r%09d of the read's index)
    const size_t cut = id.find_first_of(" \t");
    if (cut != std::string::npos) id.resize(cut);
    return id;
  };
  constexpr int64_t BLOCK = 4096;                           // features per block
  const size_t nb = (size_t)((F + BLOCK - 1) / BLOCK);
  std::string err;
  if (fasta_path) {
    const int rc = itsx::write_blocks(fasta_path, nb, [&](size_t b, std::string &out) {
      for (int64_t f = (int64_t)b * BLOCK, hi = std::min(F, f + BLOCK); f < hi; f++) {
        out.push_back('>'); out.append(label(f)); itsx::appendf(out, ";size=%d\n", feat_total[f]);
        out.append(bases + offsets[f], (size_t)(offsets[f + 1] - offsets[f])); out.push_back('\n');
      }
    }, err);
    if (rc != ITSX_OK) { (void)remove(fasta_path); return fail(ITSX_E_IO, err); }
  }
  if (tsv_path) {
    const itsx::Labels snames{sample_names, sample_name_offsets};
    const int rc = itsx::write_blocks(tsv_path, nb + 1, [&](size_t b, std::string &out) {
      if (b == 0) {
        out.append("#feature");
        for (int32_t s = 0; s < n_samples; s++) { out.push_back('\t'); if (sample_names && sample_name_offsets) out.append(snames(s)); else itsx::appendf(out, "s%d", s); }
        out.push_back('\n');
        return;
      }
      std::vector<int32_t> row((size_t)n_samples);
      for (int64_t f = (int64_t)(b - 1) * BLOCK, hi = std::min(F, f + BLOCK); f < hi; f++) {
        std::fill(row.begin(), row.end(), 0);
        for (int64_t e = row_off[f]; e < row_off[f + 1]; e++) row[(size_t)entry_sample[e]] += entry_count[e];
        out.append(label(f));
        for (int32_t s = 0; s < n_samples; s++) itsx::appendf(out, "\t%d", row[(size_t)s]);
        out.push_back('\n');
      }
    }, err);
    if (rc != ITSX_OK) { (void)remove(tsv_path); return fail(ITSX_E_IO, err); }
  }
  return ITSX_OK;
}

}  // extern "C"
