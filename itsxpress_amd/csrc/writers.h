// writers.h -- the one formatter of the files the reference's parsers read: uc.txt and rep.fa of `vsearch --fastx_uniques` /
// `--cluster_size` and hmmsearch's domtbl.txt (writers_host.cpp).  Plain arrays in, no context: the context's writers (engine.hip)
// and the array writers of a multi-GPU or streamed run hand it their own numbering, so both write the same bytes by construction.
// Every writer returns ITSX_OK, or ITSX_E_IO with `err` set ("cannot write ..." / "short write to ...").
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/itsx_hip.h"

namespace itsx {

// labels: blob[offs[i], offs[i + 1]); offs == nullptr: reads handed over without names, labelled r%09lld
struct Labels {
  const char *blob = nullptr; const int64_t *offs = nullptr;
  std::string operator()(int64_t i) const;
};

// one dereplication or clustering of n reads into U clusters, numbered by its caller (never renumbered here: clusters of equal
// abundance and equal labels keep that numbering's order)
struct Clusters {
  int64_t n = 0; int32_t U = 0;
  const int32_t *uniq_of = nullptr;     // [n] cluster of every read, -1: dropped
  const int32_t *seed_read = nullptr;   // [U] the cluster's seed (centroid); its other reads are H rows
  const int32_t *abund = nullptr;       // [U]
  const int32_t *len = nullptr;         // [n]
  const int8_t *strand = nullptr;       // [n] relative to the seed
  Labels labels;                        // of the reads
  // --cluster_size: the kept reads in processing order and the identity of their H rows; order == nullptr: exact dereplication
  const int32_t *order = nullptr; int64_t n_order = 0; const double *pct = nullptr;
  // --cluster_size, optional: the alignment of every member with its centroid (column 8 of its H row), read r's at
  // cigar_text[cigar_off[r], cigar_off[r + 1]); nullptr: the column is '*'
  const int64_t *cigar_off = nullptr; const char *cigar_text = nullptr;
  // a batch of samples: the sample of every read / cluster (nullptr: one sample) and the one sample to write (-1: all)
  const int32_t *sample = nullptr, *usample = nullptr; int32_t sel = -1;
};

// vsearch's order: exact dereplication -- abundance descending, ties by strcmp of the seed's label, stable; --cluster_size -- as
// the centroids were created
void cluster_order(const Clusters &c, std::vector<int32_t> &ord);
// exact dereplication: per cluster the S row and its H rows in input order, all C rows last; --cluster_size: the S and H rows in
// processing order, then one C row per cluster
int write_uc(const char *path, const Clusters &c, const std::vector<int32_t> &ord, std::string &err);

// the seeds' sequences: per_unique -- [off[u], off[u + 1]) of cluster u; else [off[s], off[s] + len[s]) of the seed read s
struct Seqs { const char *bases = nullptr; const int64_t *off = nullptr; bool per_unique = false; };
// the seeds in cluster order, 80 columns
int write_rep_fasta(const char *path, const Clusters &c, const std::vector<int32_t> &ord, const Seqs &seqs, std::string &err);

struct DomTable {
  const itsx_domain *rows = nullptr; size_t n = 0;      // in (profile, target, domain) order
  int32_t P = 0; Labels prof_names; const int32_t *M = nullptr;
  const float *tau = nullptr, *lambda = nullptr;        // the Forward tail of every profile (E-value columns)
  const int64_t *Z = nullptr;           // [S] hmmsearch's Z: targets searched, per sample
  const int64_t *domz = nullptr;        // [S * P] hmmsearch's domZ
  const int32_t *usample = nullptr;     // [targets] sample of every target (nullptr: one sample)
  int32_t sel = -1;                     // the one sample to write (-1: all)
  const int32_t *seed_read = nullptr;   // target t is labelled targets(seed_read[t]); nullptr: targets(t)
  Labels targets;
  const itsx_alignment *ali = nullptr;  // [n] parallel to rows, or nullptr: rows with aligned == 1 get their hmm / ali / acc columns from it
};
// the two header lines, then the reported domains of every (profile, target), renumbered "k of nrep"
int write_domtbl(const char *path, const DomTable &t, std::string &err);

}  // namespace itsx
