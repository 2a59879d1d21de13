/*
 * itsx_hip.h -- C ABI of the MI355X (gfx950) ITS-trimming engine.
 *
 * Drop-in boundary for ONE path of USDA-ARS-GBRU/itsxpress: dereplicate reads ->
 * score the representatives against the ITSx profile HMMs -> per-read trim
 * coordinates.  In the reference this path is three Python methods that shell
 * out to vsearch / hmmsearch and two parsers that re-read their output files.
 * Every entry point below names the reference interface it replaces.
 * A batch of samples goes from raw files to trimmed FASTQ in a handful of calls: with itsx_keep_records on, the read set that
 * itsx_load_reads_files / itsx_merge_pairs_load_files / itsx_orient_apply leave also keeps its FASTQ records on the device, and
 * itsx_write_trimmed_samples cuts every sample's output from them -- no seq.fq / oriented.fq in between.
 *
 * Conventions: plain C types only; every call returns 0 on success or a negative
 * ITSX_E_* code, with text available from itsx_last_error(); the caller owns all
 * output arrays; nothing throws across the boundary.  One context drives one GPU
 * (one process per GPU); a context is not thread-safe.  There is no CPU fallback:
 * itsx_create fails if no gfx950 device is usable.
 */
#ifndef ITSX_HIP_H
#define ITSX_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITSX_ABI_VERSION 6      /* 6: two-sided sharing (itsx_stats grew); 5: prefix sharing (itsx_stats grew); 4: streaming loads (itsx_stream_*, itsx_keyset_*, itsx_load_reads_text), itsx_io_cache_clear; 3: rows modes (itsx_set_rows_mode, the lazy domain stage), itsx_stats grew; 2: itsx_get_stats / itsx_get_pairtraces take the caller's struct size */

enum {
  ITSX_OK            =  0,
  ITSX_E_ARG         = -1,   /* bad argument / call order */
  ITSX_E_IO          = -2,   /* file could not be read or written */
  ITSX_E_FORMAT      = -3,   /* malformed HMMER3/f or FASTA/FASTQ text, illegal residue */
  ITSX_E_DEVICE      = -4,   /* HIP error or no usable device */
  ITSX_E_UNSUPPORTED = -5,   /* e.g. model longer than 46 nodes, read longer than 65535 bases */
  ITSX_E_COLLISION   = -6,   /* 64-bit hash collision survived every reseed (never observed) */
  ITSX_E_NOMEM       = -7
};

typedef struct itsx_ctx itsx_ctx;
typedef struct itsx_stream itsx_stream;   /* a file's text, handed out while it is being inflated (itsx_stream_*) */
typedef struct itsx_keyset itsx_keyset;   /* the sequences seen so far in a streaming run (itsx_keyset_*) */
typedef struct itsx_twriter itsx_twriter; /* a trimmed-FASTQ output that takes text and coordinates piece by piece (itsx_twriter_*) */

/* One reported-or-not domain, in hmmsearch --domtblout row order (profile file order,
 * then target index, then domain index).  Replaces one text row of domtbl.txt as
 * consumed by ItsPosition.parse (itsxpress/SeqSample.py:431-461): ll[0]=target name
 * -> rep, ll[2]=tlen, ll[3]=query name -> prof, ll[13]=domain score -> bitscore,
 * ll[19]/ll[20] = env from/to -> ienv/jenv. */
typedef struct {
  int64_t rep;            /* index of the representative in the unique list (see itsx_get_uniques) */
  int32_t prof;           /* profile index in file order */
  int32_t tlen;
  int32_t ienv, jenv;     /* 1-based envelope coordinates */
  int32_t dom_idx, ndom;
  int32_t flags;          /* bit0: the envelope was defined by stochastic traceback clustering of a multidomain region
                           * (hmmsearch's region_trace_ensemble); with ITSX_NO_ENSEMBLE=1: such a region kept as ONE envelope */
  float   envsc;          /* nats */
  float   domcorrection;  /* nats */
  float   dombias;        /* nats */
  float   bitscore;       /* bits (column 14 of domtblout, before %.1f) */
  double  lnP;
  float   seq_score;      /* bits (column 8) */
  float   seq_bias;       /* bits */
  int32_t seq_reported;   /* per-sequence score >= T */
  int32_t dom_reported;   /* exp(lnP) * domZ <= domE, set by itsx_search_finalize */
} itsx_domain;

/* The optimal-accuracy alignment of one reported domain (itsx_align_domains).  Replaces the hmm from/to, ali from/to and acc
 * columns (ll[15]..ll[18], ll[21]) of the --domtblout file of itsxpress/SeqSample.py:191-209, which are placeholders without it.
 * acc = oasc / (1 + |jenv - ienv|), in double. */
typedef struct {
  int32_t hmm_from, hmm_to;   /* first and last match state of the alignment, 1-based */
  int32_t ali_from, ali_to;   /* the target residues they emit, 1-based, inside [ienv, jenv] */
  float   oasc;               /* expected number of correctly aligned residues (the optimal-accuracy score) */
  int32_t aligned;            /* 1: the row was aligned; 0: it was not (not reported), everything else is zero */
} itsx_alignment;             /* 24 bytes */

/* per (representative, profile) filter trace for parity tests; only pairs past the MSV filter */
typedef struct {
  int64_t rep; int32_t prof;
  int32_t msv_xj;         /* final xJ byte of the MSV filter; 255 = overflow (score +inf) */
  int32_t pass_msv, pass_bias, pass_fwd;
  float   msv_sc, filtersc, fwdsc, bcksc, nullsc;
  int32_t nregions, ndom;
  int32_t ran_vit, pass_vit;   /* Viterbi filter: runs only for pairs whose bias-corrected MSV P-value exceeds F2 (none when F1 == F2) */
  float   vitsc;
  int32_t pad;
} itsx_pairtrace;

typedef struct {
  int64_t n_reads, n_unique, n_dropped_short;
  int64_t n_pairs, n_past_msv, n_past_bias, n_past_fwd, n_regions, n_multidomain, n_domains;
  int64_t n_domain_overflow;      /* (rep,profile) pairs with more than 8 regions: the ones past the pair's slots live in an overflow list (none is dropped) */
  int32_t n_profiles, hash_reseeds;
  /* device time of the last call of each stage, milliseconds (HIP events on the engine's stream) */
  float   ms_derep, ms_msv, ms_filters, ms_domains, ms_finalize;
  /* dominant-kernel accounting for bench.py's roofline block */
  float   ms_msv_kernel;  int64_t msv_cells;  int64_t msv_launches;
  float   ms_fwd_kernel, ms_bwd_kernel;  int64_t fwd_rows;   /* lane-rows: sum of target lengths over surviving pairs */
  float   ms_env_kernel;  float ms_bias_kernel;  int64_t env_rows;    /* the three envelope sweeps together; lane-rows per sweep */
  int64_t n_env_unique;           /* distinct (profile, length, envelope subsequence) actually re-scored */
  float   ms_decode_kernel;  int32_t n_batches;          /* launches of each DP kernel in the last search */
  float   ms_cluster;        int32_t n_tw_units_device;  /* itsx_cluster at id < 1: whole call | a context lent to streamed writers (itsx_twriter_set_device): units indexed, planned and copied on the device (was padding) */
  int64_t cl_windows, cl_cuts, cl_alignments;            /* speculative windows, windows cut by validation, alignments */
  float   ms_merge;                                      /* k_merge of the last itsx_merge_* call */
  float   ms_trim_plan;                                  /* the plan kernels of the last itsx_write_trimmed_paired_samples call (was padding) */
  int64_t cl_certified;                                  /* candidate alignments proven rejections without the full DP */
  float   ms_pack;                                       /* last hand-over of reads: staging + upload + device packing, host wall time */
  float   ms_trim_copy;                                  /* k_trim_copy of that call, both sides together (was padding) */
  /* parity-risk counters of the last itsx_trim_coords / itsx_rep_coords call (the prefixes decide which domains count):
   * uniques / reads whose winning left or right domain came from a region hmmsearch resolves by stochastic clustering
   * (itsx_domain.flags bit 0), and uniques / reads with a (representative, profile) pair that had more regions than
   * the engine keeps (bit 1) among the domains of the two sides */
  int64_t n_uniq_multi_winner, n_reads_multi_winner, n_uniq_region_cap, n_reads_region_cap;
  /* multidomain regions of the last search: resolved by stochastic traceback clustering (k_ensemble.hip), of which
   * n_mr_failed hit a bookkeeping limit or an unsampleable matrix and yielded nothing; envelopes the clustering defined */
  int64_t n_mr_clustered, n_mr_failed, n_mr_envelopes;
  float   ms_ensemble;       float   ms_deflate;         /* k_deflate of the last device deflate, all waves together (was padding) */
  int64_t n_mr_distinct;     /* distinct (profile, target length, residues) multidomain regions actually sampled */
  int64_t n_slab_shrinks;    /* times the DP slab budget was halved because the device could not supply it */
  float   ms_vit_kernel;     int32_t n_tw_units_host;    /* Viterbi filter (F2 < F1 only) | a lent context: units the HOST sliced (lines not 4 per record, a malformed record, 2^31 bytes, the test hook) whose text the device deflated (was padding) */
  /* multidomain regions of the last search whose Forward matrix could not be sampled, by kind: [1] probabilities not normalised,
   * [5] a path left the region -- the cases in which hmmsearch's own stochastic traceback throws; itsx_search then returns
   * ITSX_E_UNSUPPORTED.  The former bookkeeping limits ([2] more than 8 domains in one sampled path, [4] more than 512 distinct
   * sampled tuples, [7] more than 4 envelopes in one region) no longer fail anything: such regions take the ensemble stage's overflow
   * path (n_mr_overflow), and a pair's regions past its 8 slots an overflow list (n_domain_overflow counts those pairs). */
  int64_t n_mr_fail_kind[8];
  /* domain rows (80 B each) resident on the device after the last search: all of them (= n_domains plus segment padding), or, with
   * ITSX_COMPACT_ROWS=1, only the rows that can still win ItsPosition's argmax whatever the dataset-wide domZ turns out to be */
  int64_t n_rows_resident;
  /* the lazy domain stage (itsx_set_rows_mode(ctx, ITSX_ROWS_LAZY)) of the last search: pairs that went through Backward / decoding /
   * envelopes (of n_past_msv), of which round 1 took the best-bound pair of each (representative, class); rows whose reporting
   * depended on the exact domZ and could have changed a result (then the search was repeated in full: n_lazy_reruns);
   * lane-rows and launches of the score-only Forward pass, its time and the selection's */
  int32_t lazy;              int32_t n_bound_launches;
  int64_t n_lazy_pending_profiles;                      /* distinct profiles among the undecided rows that mattered */
  int64_t n_lazy_completed, n_lazy_completed_profiles;  /* itsx_lazy_complete: pairs of the profiles counted exactly, and those profiles */
  int64_t n_mr_overflow;     /* distinct multidomain regions that went through the ensemble stage's overflow path (per-region arrays sized by the region) */
  float   ms_lazy_complete;  float lazy_bound_maxdiff;  /* ITSX_LAZY_CHECK_BOUND=1 (tests): largest |bound kernel - HMMER-order Forward| of the last search, nats */
  int64_t n_lazy_evaluated, n_lazy_round1, n_lazy_pending, n_lazy_reruns, bound_rows;
  float   ms_bound_kernel, ms_lazy_select;
  /* prefix sharing (csrc/k_share.hip) of the last search: rows per block of the prefix tree (0: off); saved row states and chains that
   * start from one; lane-rows the MSV filter and the lazy stage's score-only Forward pass computed (msv_rows, bound_rows) against the
   * rows of their pairs (msv_rows_full, bound_rows_full); pairs that ran in the Forward pass only for a chain below them;
   * ITSX_SHARE_CHECK=1 (tests): results that differ from the unshared kernels' (MSV cells, Forward scores; must be 0) */
  int32_t share_B;           int32_t share_batches;
  int64_t share_nodes, share_chains, msv_rows, msv_rows_full, bound_rows_full, n_share_helpers, share_mismatch;
  float   ms_share_build;    float share_frac;          /* building the tree and the order, ms; rows the chains skip / rows of all uniques */
  /* two-sided sharing (round 6; lazy searches): a Forward chain stops where its SUFFIX is one an earlier representative of its length
   * ends with too, and takes the rest of the sum over paths from the Backward state that representative's chain saved there.
   * n_joined: representatives that join; bwd_chains / gamma_nodes: Backward chains and their saved states; per representative (one
   * profile) two_fwd_rows + two_bwd_rows rows are walked of two_rows_full; bwd_rows: lane-rows of the Backward chains of the last
   * search (bound_rows: the Forward chains'); ITSX_SHARE_CHECK=1 (tests): join_maxdiff = largest |joined score - unshared score|, nats
   * (more than 2e-3 counts into share_mismatch) */
  int32_t two_sided;         int32_t n_bwd_launches;
  int64_t n_joined, bwd_chains, gamma_nodes, bwd_rows, two_fwd_rows, two_bwd_rows, two_rows_full;
  float   join_maxdiff;      float ms_bwd_bound;        /* the Backward chains' kernel time (part of ms_bound_kernel) */
  /* the top-up round of itsx_search_finalize (round 6): pairs it evaluated -- the best-bound unevaluated pairs of the profiles with
   * undecided rows, as many as those rows need for the lower bound on domZ to decide them -- and its time (part of ms_finalize);
   * n_lazy_completed stays 0 when it settles everything.  ms_lazy_topup_stages = the part of ms_lazy_topup spent in the domain pipeline:
   * that part is ALSO accumulated into ms_filters / ms_domains, like the stages itsx_lazy_complete re-runs (it took the place of a
   * padding word: the structure's size and every other offset are unchanged) */
  int64_t n_lazy_topup;      float ms_lazy_topup;       float ms_lazy_topup_stages;
  /* the device inflate (itsx_inflate_device, the loaders of a context that opted in): the two kernels' time and the members of the last
   * call; files the device inflated and files it declined since the context was created (the structure grew at its end: every earlier
   * offset is unchanged) */
  float   ms_inflate;        int32_t n_inflate_members;
  int64_t n_inflate_device, n_inflate_declined;
  /* the device parse (itsx_parse_device, the whole-file loaders of a context that opted in): its kernels' time in the last call, all of
   * the call's texts together; texts the device parsed and texts it declined since the context was created (the structure grew at its
   * end again: every earlier offset is unchanged) */
  float   ms_parse;          int32_t parse_reserved;    /* (padding: 0) */
  int64_t n_parse_device, n_parse_declined;
} itsx_stats;

int         itsx_abi_version(void);
/* itsx_last_error(NULL) returns the message of the last failed itsx_create. */
const char *itsx_last_error(const itsx_ctx *ctx);

/* Replaces: process start-up of the vsearch / hmmsearch subprocesses
 * (itsxpress/SeqSample.py:117,162,210).  device_id = HIP ordinal; flags = 0. */
itsx_ctx   *itsx_create(int device_id, int flags);
void        itsx_destroy(itsx_ctx *ctx);

/* ---- profiles: replaces hmmsearch reading `hmmfile` (itsxpress/SeqSample.py:207), the
 * HMMER3/f text written by create_runtime_hmm (itsxpress/main.py:176-231). */
int itsx_load_profiles_file(itsx_ctx *ctx, const char *hmm_path, int *n_profiles);
int itsx_load_profiles_mem(itsx_ctx *ctx, const char *text, int64_t len, int *n_profiles);
int itsx_profile_name(const itsx_ctx *ctx, int i, char *buf, int buflen);
/* table parity: copy out the configured MSV byte costs [18][M+1], striped odds ratios
 * rfv [18][Q][4] / tfv [8Q][4], and {M, Q, base, bias, tbm, tec}. */
int itsx_profile_tables(const itsx_ctx *ctx, int i, uint8_t *rbv, float *rfv, float *tfv, int32_t *params6);

/* ---- reads: replaces vsearch/hmmsearch reading self.seq_file / rep.fa
 * (itsxpress/SeqSample.py:109,208).  ASCII bases, IUPAC allowed, case-insensitive, U == T.
 * offsets has n+1 entries.  names may be NULL (then the writers emit r%09d).
 * The reads are packed 2 bits/base (+ an exception list for non-ACGT) and are resident in
 * HBM when the call returns. */
int itsx_set_reads(itsx_ctx *ctx, const char *bases, const int64_t *offsets, int64_t n,
                   const char *names, const int64_t *name_offsets);
/* The same without the host-side copy of the bases: the engine keeps the caller's `bases` pointer (itsx_write_rep_fasta
 * reads the representatives from it), so the caller keeps that buffer valid and unchanged until the next reads call on
 * this context or itsx_destroy.  offsets and names are copied as before. */
int itsx_set_reads_view(itsx_ctx *ctx, const char *bases, const int64_t *offsets, int64_t n,
                        const char *names, const int64_t *name_offsets);
/* The same for text that already lives in DEVICE memory (d_bases: a hipMalloc'ed buffer of ASCII bases on this
 * context's GPU, e.g. the output of a device-side parser or of the merge kernel); offsets and names are host arrays.
 * Nothing crosses PCIe but the offsets; the bases are packed where they are.  The caller keeps d_bases valid until the
 * next reads call or itsx_destroy (itsx_write_rep_fasta copies the text back on demand). */
int itsx_set_reads_device(itsx_ctx *ctx, const void *d_bases, const int64_t *offsets, int64_t n,
                          const char *names, const int64_t *name_offsets);
/* FASTA or FASTQ file, plain or gzip (.gz): native parser for the same input. */
int itsx_load_reads_file(itsx_ctx *ctx, const char *path, int64_t *n_reads);
/* One contiguous shard of the same file: records [n shard / n_shards, n (shard + 1) / n_shards) in file order, for a driver that
 * spreads one sample over several GPUs (itsxpress_amd/multi.py); n_total = records in the file, first = index of the shard's first. */
int itsx_load_reads_file_shard(itsx_ctx *ctx, const char *path, int32_t shard, int32_t n_shards, int64_t *n_total, int64_t *first, int64_t *n_reads);
/* the records of a piece of FASTA / FASTQ TEXT already in memory (a slice of itsx_stream_next); replaces the context's reads */
int itsx_load_reads_text(itsx_ctx *ctx, const char *text, int64_t nbytes, int64_t *n_reads);

/* ---- streaming file-to-file runs (host-only, context-free: csrc/stream_host.cpp; driver: itsxpress_amd/stream.py).
 * The reference inflates and parses the whole FASTQ before vsearch starts (itsxpress/main.py:534-554, SeqSample.py:93-131); on one
 * MI355X the inflater is the slower party, so a large .fastq.gz is cut into file-order chunks that are dereplicated and scored while
 * the rest is still being inflated.
 * itsx_stream_open: reads the file and starts inflating in the background (block-parallel for large gzip files; plain, zstd and
 *   small files are ready at once).  itsx_stream_next: BLOCKS until >= min_bytes of new text are final (or the file ends) and returns
 *   the next slice, cut at a FASTQ record start (non-FASTQ text arrives in one slice); *last = 1 on the final slice.  Slices stay
 *   valid until itsx_stream_close; keep_text != 0 leaves the whole text in the process's text cache under the file's path, where
 *   itsx_write_trimmed_fastq finds it.  A corrupt file is an error of the LAST call at the latest (CRC-32 and length of every gzip
 *   member are checked as in itsx_load_reads_file): a driver discards what it computed from earlier slices.
 * itsx_keyset_assign: tuples[n_unique][4] as itsx_unique_keys128 returns them for chunk `chunk`; verdict[n_unique][4] = per local
 *   unique (global index, orientation flag) of the sequence's FIRST occurrence so far and (chunk, local unique) of the holder that
 *   scores it -- the first holder, which in file order is vsearch's representative.  Same rows as the multi-GPU owner verdicts.
 *   gid[n_unique] (may be NULL): the sequence's number in first-seen order = its index in the global unique list.
 * Errors: negative code, text from itsx_stream_last_error(). */
int itsx_stream_open(const char *path, itsx_stream **out);
/* Round 6, for a multi-GPU driver (itsxpress_amd/multi.py; replaces the reference's whole-file read of itsxpress/main.py:295-330 for N
 * worker processes): the text is inflated into a SHARED mapping of `backing` (a new, sparse file the caller unlinks), so that a worker
 * maps the slice it is told about -- offset = slice address - itsx_stream_base(s) -- while later slices are still being inflated; no
 * copy of the pieces.  *plain_input = 1: the input is uncompressed and was not copied: the offsets are offsets into the input file.
 * itsx_stream_progress: text bytes that are final, compressed bytes behind them, the file's size (for an estimate of the whole
 * text's size before it is there: even pieces). */
int itsx_stream_open_threads(const char *path, int32_t threads, itsx_stream **out);     /* itsx_stream_open with a pool of `threads` inflating threads */
int itsx_stream_open_shared(const char *path, const char *backing, itsx_stream **out, int32_t *plain_input);
const char *itsx_stream_base(itsx_stream *s);
int itsx_stream_progress(itsx_stream *s, int64_t *avail, int64_t *consumed, int64_t *raw_size);
int itsx_stream_next(itsx_stream *s, int64_t min_bytes, const char **text, int64_t *nbytes, int32_t *last);
int itsx_stream_close(itsx_stream *s, int32_t keep_text);
/* Round 6, a streamed PAIRED sample (itsxpress/SeqSample.py:266-365, main.py:513-519: the reference merges the whole files first):
 * R1's slice comes from itsx_stream_next, itsx_count_records says how many records it holds, and the mate file's stream hands out
 * exactly that many with itsx_stream_next_records (fewer only at the end of its file: *got). */
int itsx_stream_next_records(itsx_stream *s, int64_t n_records, const char **text, int64_t *nbytes, int64_t *got, int32_t *last);
int64_t itsx_count_records(const char *text, int64_t nbytes);
/* an upper bound of the number of records in the whole file (lines / 4 for FASTQ), or -1 while it is still being inflated */
int64_t itsx_stream_records_bound(itsx_stream *s);
const char *itsx_stream_last_error(void);
/* ---- one file's records in pieces, for the workers of a multi-GPU driver (host-only, context-free: csrc/shard_host.cpp; driver:
 * itsxpress_amd/multi.py).  The reference hands the whole file to one vsearch process (itsxpress/SeqSample.py:93-131, 266-365).
 * itsx_shard_text: the file's text (plain / gzip / zstd, inflated once, kept in the process's text cache) cut into n_parts contiguous
 *   pieces at record starts near equal byte counts; piece p is written as the plain file out_prefix.<p> (use a /dev/shm prefix) and
 *   holds records[p] records (bytes[p] bytes; bytes may be NULL).  match_records != NULL (a mate file, R2 after R1): piece p is cut
 *   to hold exactly match_records[p] records instead; a file that does not hold them is ITSX_E_FORMAT.
 * Errors: negative code, text from itsx_shard_last_error(). */
/* one piece of a text in memory (a slice of itsx_stream_next, while the rest of the file is still being inflated) into a new file, by the
 * I/O pool: a multi-GPU driver's worker loads it with itsx_load_reads_file */
int itsx_write_range(const char *path, const char *text, int64_t nbytes);
int itsx_shard_text(const char *path, int32_t n_parts, const int64_t *match_records, const char *out_prefix, int64_t *records, int64_t *bytes);
/* The owner's step of the cross-shard dereplication for a multi-worker run (itsxpress_amd/multi.py: owner_verdicts states it in numpy):
 * recv[m][5] = (key0, key1, global index of the first occurrence, forward-is-canonical flag, local unique number) of the uniques whose
 * keys this worker owns, src[m] = the worker each row came from; out[m][4] = per row the global index and flag of its group's first
 * occurrence and the worker / local unique number of the holder that scores the sequence.  Host-only. */
int itsx_owner_verdicts(const int64_t *recv, const int64_t *src, int64_t m, int64_t *out);
const char *itsx_shard_last_error(void);
itsx_keyset *itsx_keyset_create(void);
void itsx_keyset_destroy(itsx_keyset *k);
int64_t itsx_keyset_size(const itsx_keyset *k);
int itsx_keyset_assign(itsx_keyset *k, const int64_t *tuples, int64_t n_unique, int32_t chunk, int64_t *verdict, int64_t *gid);

/* ---- f4, per-sample batching: the QIIME 2 plugin runs the whole path once per sample
 * (itsxpress/q2_itsxpress.py:273-333: one SeqSample, one vsearch and one hmmsearch process per manifest row), which
 * starves a GPU when samples are small.  Here many samples share ONE read set and one pass of every kernel while each
 * keeps the results of its own run: reads are dereplicated only within their sample (the first occurrence INSIDE the
 * sample is the representative, so orientation and labels are the sample's own), and hmmsearch's domZ -- the number
 * of reported targets the domain E-value threshold is scaled by -- is counted per (sample, profile).
 * itsx_load_reads_files: the samples' sequence files (FASTA/FASTQ, plain/gzip/zstd) in order; sample index = file index.
 * itsx_set_samples: the same for reads handed over with itsx_set_reads (sample_of_read[n_reads], values in
 * [0, n_samples)); NULL or n_samples <= 1 returns to one sample.  A new read set resets the batch to one sample.
 * With S samples itsx_get_domz / itsx_set_domz move S * n_profiles counters ([sample][profile]).
 * itsx_select_sample: the file writers (itsx_write_uc / _rep_fasta / _domtbl) emit that sample only (cluster numbers
 * and the E-value columns as in a run of that sample alone); -1 = every sample.
 * Greedy clustering at id < 1 is batched by its own call, itsx_cluster_samples (itsx_cluster keeps refusing S > 1).
 * Not batched: itsx_unique_keys (shard whole samples instead). */
int itsx_load_reads_files(itsx_ctx *ctx, const char *const *paths, int32_t n_paths, int64_t *n_reads_per_file);
int itsx_set_samples(itsx_ctx *ctx, const int32_t *sample_of_read, int32_t n_samples);
int itsx_num_samples(const itsx_ctx *ctx);
int itsx_select_sample(itsx_ctx *ctx, int32_t sample);
/* ---- sample sharing (opt-in; off by default, and off changes nothing).  The plugin's loop runs one hmmsearch per manifest row
 * (itsxpress/q2_itsxpress.py:273-333), so a sequence that is a representative in 300 samples of one amplicon is scored 300 times --
 * and a batch that keeps every sample's own representatives does the same.  hmmsearch scores a target from its residues alone (it
 * reseeds its generator per target, -T is a score threshold); the sample enters only where a reported target is counted into domZ and
 * where exp(lnP) * domZ is held against domE.  With the mode on, a search of S > 1 samples groups the uniques of all samples into
 * SCORE CLASSES -- the uniques whose representatives are the same string in the same orientation (csrc/k_derep.hip: keyed by XXH64 of
 * the packed forward words, the exception list and the length, verified word by word; a reverse complement is another target and
 * another class) --, sends one HOLDER per class (its member with the smallest unique index) through the HMM stages, copies the
 * holder's rows to every other member with `rep` rewritten, and counts each member's reported targets into its own sample's domZ.
 * itsx_search_finalize and everything behind it (coordinates, domtbl.txt per sample) run unchanged on those rows: every member gets
 * the rows, dom_reported under its own sample's domZ, coordinates and domtbl.txt lines of a search without the mode, bit for bit
 * (the row table is served in --domtblout order either way).  uc.txt / rep.fa are untouched.  The pair traces
 * (itsx_get_pairtraces) are the unshared search's too: every member gets its holder's traces with `rep` rewritten.  itsx_stats
 * describes the work done: the pairs, cells, rows and times of the holders.
 * Does not apply (accepted, and itsx_sample_sharing_info reports zero classes): one sample; the compact and lazy rows modes, which keep
 * their domZ bounds, top-up round and verdicts per (sample, profile) and have a setting of their own
 * (itsx_set_sample_sharing_lazy, below); a context whose active uniques the caller chose
 * (itsx_set_active_uniques, and with it the itsx_unique_keys-driven sharded runs).  ITSX_SHARE_SAMPLES=1 does the same for every
 * context. */
int itsx_set_sample_sharing(itsx_ctx *ctx, int on);
/* What the last itsx_search shared, in place of one hmmsearch per manifest row (itsxpress/q2_itsxpress.py:273-333): the score
 * classes it built, the uniques that were not scored because their class's holder was (n_unique - n_classes), and the rows copied
 * to them.  All zero when the mode was off or does not apply (the cases above).  Where it applies and the samples have nothing in
 * common, the classes are built all the same: n_classes == n_unique, nothing shared, nothing copied, and the search itself runs as
 * without the mode.  Each pointer may be NULL.  ITSX_E_ARG before a search. */
int itsx_sample_sharing_info(const itsx_ctx *ctx, int64_t *n_classes, int64_t *n_uniques_shared, int64_t *n_rows_expanded);
/* ---- sample sharing in the lazy and compact rows modes (opt-in; a setting of its own: itsx_set_sample_sharing keeps governing the
 * full rows mode alone, and this one has no effect there).  The plugin's loop (itsxpress/q2_itsxpress.py:273-333) is where both of
 * the batch's large savings count -- evaluating only the pairs that can still win, and scoring a shared sequence once -- and with this
 * setting a lazy or compact search of S > 1 samples takes both: the score classes are built as above, the MSV filter, pass A, the
 * lazy rounds and the domain pipeline walk the holders only, and
 *   - every evaluated pair that is a reported target adds one to the domZ counter of EVERY member's sample (csrc/k_derep.hip:
 *     k_member_*, over the chunk's scratch rows before compaction drops them: exact, since the members of a class lie in different
 *     samples and their residues, hence their scores, are the holder's);
 *   - the upper counter of a lazy search adds the HOLDERS past the MSV filter to every sample.  It stays an upper bound: a sample
 *     holds at most one member of a class, so the classes past the filter are at least any one sample's uniques past it;
 *   - the rows the search KEPT are copied to the other members with `rep` rewritten before any finalize (n_rows_expanded counts
 *     them), so finalize, the coordinates, the writers and itsx_align_domains see a member's rows under its own sample's counters.
 * itsx_lazy_complete (and itsx_search_finalize through it) walks the holders again, counts members the same way and copies the rows
 * of the segments it adds; afterwards lower == upper == the exact count for every (sample, completed profile).  The compact re-search
 * that finalize keeps as a safety net is a sharing search itself.  Coordinates, uc.txt, rep.fa and the kept rows' domtbl.txt are
 * those of a search without the setting; the lazy counters are valid bounds on hmmsearch's domZ either way, though not necessarily
 * the same bounds (which pairs the lazy rounds evaluate may depend on the last bits of pass A's scores, and those on the prefix
 * tree of the uniques searched); the compact mode's counters are exact and equal.  itsx_stats describes the holders' work, as in
 * the full mode; the pair traces of a compact search are mapped to the members as there, and itsx_debug_lazy_pairs serves one
 * sample only, so it never follows such a search.  Applies when: the setting is on (or ITSX_SHARE_SAMPLES_LAZY=1), S > 1, the
 * rows mode of the search is compact or lazy, and the caller has not narrowed the active uniques.  Not changed: counters exchanged
 * between ranks (itsx_set_domz / itsx_domz_device) at S > 1 -- a combination nothing uses -- behave as before. */
int itsx_set_sample_sharing_lazy(itsx_ctx *ctx, int on);
/* the mode's own two steps in that search, milliseconds: building the classes, and copying rows and counting (what the saved
 * hmmsearch work of q2_itsxpress.py:273-333 is paid with; scripts/batch_bench.py reports both).  Each is the span between two HIP
 * events on the engine's stream around the whole step, so it holds the step's kernels AND the host synchronisations and small
 * device-to-host copies between them (the collision count and the number of classes; per row segment the number of copies). */
int itsx_sample_sharing_times(const itsx_ctx *ctx, float *ms_classes, float *ms_expand);
/* test hook: class_of[n = n_unique] as the last sharing search left it on the device.  Classes are numbered by their holders in
 * rising unique index; uniques of different manifest rows (q2_itsxpress.py:273-333) share a number exactly when their
 * representatives are one string in one orientation.  ITSX_E_ARG when that search built no classes. */
int itsx_debug_sample_classes(itsx_ctx *ctx, int32_t *class_of, int64_t n);

/* ---- f4: SeqSample.orient_reads (itsxpress/SeqSample.py:48-91) = vsearch --orient IN --db REF --fastqout OUT
 * (12-mer presence counts on both strands, 4x rule; restated in oracle/orc_cluster.c, parity unpinned).
 * itsx_orient_load_db: FASTA (plain/gzip) of reference sequences -> 12-mer bitmap on the device.
 * itsx_orient: per loaded read strand = +1 forward, -1 reverse (to be reverse-complemented), 0 undetermined; counts may be NULL.
 *   Reads of any length the engine loads (up to 65535 bases).
 * itsx_write_oriented_fastq (host, context-free): the FASTQ vsearch would write for those orientations. */
int itsx_orient_load_db(itsx_ctx *ctx, const char *fasta_path, int64_t *n_sequences);
int itsx_orient(itsx_ctx *ctx, int8_t *strand, int32_t *count_fwd, int32_t *count_rev);
int itsx_write_oriented_fastq(const char *seq_path, const char *out_path, const int8_t *strand, int64_t n_records, int64_t *n_written);
/* itsx_orient_apply: orients the context's read set as itsx_orient does (S samples: itsx_load_reads_files, or itsx_set_reads +
 * itsx_set_samples; S = 1 is one sample) and REPLACES it, on the device, by the reads vsearch --orient --fastqout keeps: forward reads as
 * they are, reverse reads reverse-complemented (packed words, exception lists and the host text, whose case is kept), undetermined reads
 * dropped; sample order, then input order.  Afterwards the context is in the state itsx_load_reads_files leaves after loading the S
 * per-sample oriented.fq files that itsx_write_oriented_fastq writes for these strands: S unchanged (a sample that keeps nothing stays, without
 * reads), no dereplication or search results.  strand / count_fwd / count_rev: [reads BEFORE the call], each may be NULL;
 * n_kept_per_sample: [itsx_num_samples], may be NULL.  Reads without labels stay without.
 * On any error (ITSX_E_ARG before itsx_orient_load_db, ITSX_E_NOMEM, ITSX_E_DEVICE) the context KEEPS the read set it had, with whatever
 * results it held: the new read set is built beside it and swapped in only when it is complete. */
int itsx_orient_apply(itsx_ctx *ctx, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, int64_t *n_kept_per_sample);
/* Orientation by the profiles (opt-in; no reference tool does this step: ITSx's own both-strand search is the model).  For a text t,
 * n_fwd(t) = the loaded profiles whose MSV filter passes on t at threshold F1 -- exactly the filter of itsx_search (pass_msv of
 * itsx_pairtrace; the bias filter plays no part) -- and n_rev(t) = n_fwd(reverse complement of t).  strand = +1 if n_fwd > n_rev, -1 if
 * n_rev > n_fwd, 0 otherwise (nothing passes on either strand, or a tie).  Exact integer arithmetic throughout.
 * The call dereplicates the read set itself (strand both, minseqlength 1, per sample) and scans the distinct texts only; a read that
 * is the reverse complement of its cluster's seed gets the seed's strand negated and its counts swapped; a read the dereplication
 * drops (empty) gets 0 / 0 / 0.  strand / count_fwd / count_rev: [reads], each may be NULL.  *ms_kernels (may be NULL): the device
 * time of the scans and of this step's own kernels.  Reads of any length the engine loads (up to 65535 bases).
 * itsx_orient_profiles_apply also reverse-complements the reads of strand -1 where they are, as itsx_orient_apply does (packed words,
 * exception lists, the host text with its case kept, and with itsx_keep_records the records) -- but a read of strand 0 is KEPT AS IT
 * IS: the number of reads, their order and their samples do not change.
 * Afterwards (either call) the context holds no dereplication, clustering or search results.  ITSX_E_ARG before profiles are loaded
 * and before a read set is loaded.  On any error the context keeps the read set it had: the new one is built beside it and swapped
 * in only when it is complete.  The scan obeys ITSX_CHUNK_UNIQUES and the device memory that is free. */
int itsx_orient_profiles(itsx_ctx *ctx, double F1, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, float *ms_kernels);
int itsx_orient_profiles_apply(itsx_ctx *ctx, double F1, int8_t *strand, int32_t *count_fwd, int32_t *count_rev, float *ms_kernels);

/* ---- f2: SeqSample._merge_reads (itsxpress/SeqSample.py:266-365) = vsearch --fastq_mergepairs R1 --reverse R2
 * --fastqout seq.fq --fastq_maxdiffs 40 --fastq_maxee 2 --fastq_qmax 93 [--fastq_allowmergestagger]; restated in
 * oracle/orc_merge.c (parity unpinned: the reference's merged fixture was made by another tool).
 * itsx_merge_buffers: pair i = forward read fseq/fqual[foff[i]..foff[i+1]) and reverse read (as in the file)
 * rseq/rqual[roff[i]..roff[i+1]); the merged read of pair i is written at out_seq/out_qual[foff[i] + roff[i]] with
 * length out_len[i]; reason[i]: 0 merged, 1 no shared 5-mers, 2 several candidate alignments, 3 score < 16,
 * 4 > maxdiffs, 5 overlap < 10, 6 staggered, 7 expected errors > maxee, 8 empty/too long.  score/shift may be NULL.
 * Every merge entry point reads bases in upper case and writes upper-case merged reads: a lower-case base is its upper case.
 * itsx_merge_pairs_files: FASTQ (plain/gzip) in, plain FASTQ out, labels = forward identifier up to the first blank.
 * itsx_merge_tables: the score / quality tables (context-free; tests compare them with the oracle's). */
int itsx_merge_buffers(itsx_ctx *ctx, const char *fseq, const char *fqual, const int64_t *foff, const char *rseq, const char *rqual,
                       const int64_t *roff, int64_t n, int maxdiffs, double maxee, int allow_stagger,
                       char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift);
int itsx_merge_pairs_files(itsx_ctx *ctx, const char *r1_path, const char *r2_path, const char *out_path, int maxdiffs, double maxee,
                           int allow_stagger, int64_t *n_pairs, int64_t *n_merged);
/* the same merge with the merged reads left as the context's read set (labels: R1 identifiers of the merged pairs, input order): no
 * seq.fq is written and nothing is parsed again; the merged bases stay on the device.  What an arrays-mode caller uses in place of
 * itsx_merge_pairs_files + itsx_load_reads_file. */
int itsx_merge_pairs_load(itsx_ctx *ctx, const char *r1_path, const char *r2_path, int maxdiffs, double maxee, int allow_stagger,
                          int64_t *n_pairs, int64_t *n_merged);
/* the same from record-aligned pieces of the two files' text that hold the same number of records (a streaming driver's slices), and,
 * per pair of the last merge-and-load, the index of its merged read in the context's read set (-1: not merged) */
int itsx_merge_pairs_load_text(itsx_ctx *ctx, const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int maxdiffs, double maxee, int allow_stagger,
                               int64_t *n_pairs, int64_t *n_merged);
int itsx_merge_pair_index(const itsx_ctx *ctx, int32_t *index, int64_t n_pairs);
/* f4 batching: the pairs of EVERY sample of a batch (q2_itsxpress.py:72-80 merges once per manifest row) in one call.  Sample s is
 * r1_paths[s] / r2_paths[s] (FASTQ, plain / gzip / zstd, mixed freely; read and parsed side by side); the two must hold the same number
 * of records (else ITSX_E_FORMAT, naming both).  All pairs go through ONE merge; the merged reads, in sample order and then pair order,
 * become the context's read set in the state itsx_load_reads_files leaves: itsx_num_samples = n_samples, each read tied to its sample,
 * labels = R1 identifiers up to the first blank, no dereplication or search results.  A sample may hold no records, or merge none.
 * seq_out_paths: NULL, or per sample NULL (nothing written) or the path of that sample's merged records, byte for byte the file
 * itsx_merge_pairs_files writes for the sample alone; merged bases and qualities leave the device only if at least one is given.
 * n_pairs_per_sample / n_merged_per_sample: [n_samples], may be NULL.
 * Afterwards itsx_merge_pair_index(ctx, index, total pairs) gives, for every pair of the batch in the same order (sample, then pair),
 * the index of its merged read in the batch's read set (-1: not merged).
 * On any error the context is left empty (no reads, one sample) and usable. */
int itsx_merge_pairs_load_files(itsx_ctx *ctx, const char *const *r1_paths, const char *const *r2_paths,
                                const char *const *seq_out_paths /* NULL, or entries NULL: nothing written for that sample */,
                                int32_t n_samples, int maxdiffs, double maxee, int allow_stagger,
                                int64_t *n_pairs_per_sample, int64_t *n_merged_per_sample);
int itsx_merge_tables(double *q2p, double *match, double *mism, uint8_t *qsame, uint8_t *qdiff);
/* ---- joining the pairs that do not overlap (opt-in per context; off by default, and off runs the merge kernel built without it).
 * ITS1 / ITS2 span about 100 to over 600 bases, so a 2x250 or 2x300 run cannot merge the long ones, and a pair the merge rejects is
 * gone from seq.fq, the read set and both trimmed outputs.  While on, a pair rejected with reason 1 (no shared 5-mers), 3 (score < 16)
 * or 5 (overlap < 10) is JOINED instead: its read is R1 (upper case), "NNNNNNNN", then the reverse complement of R2 as the merge reads
 * it (upper case; a symbol outside ACGTU complements to N, U to A); its qualities are R1's, "IIIIIIII", then R2's reversed -- vsearch
 * --fastq_join's padding as its manual gives it (PARITY UNPINNED, like the merge's: no vsearch build was at hand; the join is not part
 * of the reference, which drops these pairs).  Reasons 2, 4, 6, 7 and 8 are not joined; a joined read gets no expected-error filter
 * (--fastq_join has none); reason[i] keeps its code; merged pairs are bit for bit what they are with the setting off.
 * Honoured by itsx_merge_pairs_files (seq.fq holds merged and joined records in pair order), itsx_merge_pairs_load, _load_text and
 * _load_files, on the host and the device parse path: the read set holds merged and joined reads in pair order, labels and
 * itsx_merge_pair_index cover both kinds, itsx_keep_records / itsx_keep_pair_records work unchanged.  *n_merged keeps counting merged
 * pairs only.  A joined read is a read like any other: with tlen = L1 + 8 + L2, start inside R1 and stop inside the R2 part, the paired
 * writers' slices R1[start:stop] and R2[tlen - stop : tlen - start] are R1[start:] and R2[tlen - stop:], each mate cut at its own anchor.
 * itsx_merge_buffers ignores the setting.  Left out: --join_padgap / --join_padgapq, an expected-error or length filter for joined reads.
 * itsx_merge_join_info: per pair of the context's last merge call (after a merge-and-load: the pairs itsx_merge_pair_index speaks of;
 * after itsx_merge_pairs_files: that call's pairs) joined[i] = 1 where its read is a joined one, *n_joined their number; either may be
 * NULL; all 0 with the setting off.
 * itsx_merge_buffers_join: itsx_merge_buffers with the join always on.  Output planes hold foff[n] + roff[n] + 8 n bytes, pair i's read
 * is at foff[i] + roff[i] + 8 i, out_len[i] = fl + 8 + rl and joined[i] = 1 for a joined pair. */
int itsx_set_merge_join(itsx_ctx *ctx, int on);
int itsx_merge_join_info(const itsx_ctx *ctx, int8_t *joined, int64_t n_pairs, int64_t *n_joined);
int itsx_merge_buffers_join(itsx_ctx *ctx, const char *fseq, const char *fqual, const int64_t *foff, const char *rseq, const char *rqual,
                            const int64_t *roff, int64_t n, int maxdiffs, double maxee, int allow_stagger,
                            char *out_seq, char *out_qual, int32_t *out_len, int32_t *reason, double *score, int32_t *shift, int8_t *joined);

/* ---- a read set that keeps its records (opt-in; off by default, and off costs nothing).  While on, every read set made by
 * itsx_load_reads_files (FASTQ only: a FASTA file is ITSX_E_FORMAT, naming it), itsx_merge_pairs_load_files / itsx_merge_pairs_load and
 * itsx_orient_apply also keeps, in device memory, what a FASTQ record needs beyond the packed words: the ASCII bases as in the input
 * (case and IUPAC symbols; a merge's bases are upper case, as seq.fq's), the ASCII qualities (a merge's: the merged ones) and the whole
 * title line ('@', identifier, comment; a merge's: '@' + the R1 identifier up to the first blank, as itsx_merge_pairs_files writes it;
 * no CR).  One owned copy per read set, released with it; +2 bytes per base plus the titles.  itsx_orient_apply turns the records as
 * itsx_write_oriented_fastq writes them (reverse reads: IUPAC-complemented reversed bases, reversed qualities; undetermined reads
 * dropped; titles unchanged), and a failed call keeps the old read set AND its records.  A read set made any other way
 * (itsx_set_reads*, itsx_load_reads_file / _text / _file_shard, itsx_merge_pairs_load_text) has no records. */
int itsx_keep_records(itsx_ctx *ctx, int on);
/* f1 for a batch: Dedup.create_trimmed_seqs (itsxpress/SeqSample.py:886-949) of every sample in one call, from the records the
 * context keeps (itsx_keep_records).  out_paths[s] receives exactly the records itsx_write_trimmed_fastq writes for sample s's
 * own sequence file and its slice of the coordinates (an entry may be NULL: that sample is skipped; a sample that writes nothing
 * still gets its empty file).
 * Coordinates: either left_prefix / right_prefix (the per-read coordinates of the finalized search, taken where they are on the
 * device, as itsx_trim_coords_device gives them), or start / stop [n_reads] from the caller -- exactly one of the two.
 * compression: 0 plain, 1 gzip, 2 zstd, 3 gzip deflated on the device (below).  n_written_per_sample / total_len_per_sample: [n_samples], may be NULL.
 * ITSX_E_ARG: no records (the message names itsx_keep_records), n_samples != itsx_num_samples, both or neither coordinate source,
 * prefixes before itsx_search_finalize.  ITSX_E_IO: a file could not be written whole (it is removed, never left short).
 * The text of the whole batch is made on the device (csrc/k_trim.hip) and fetched in pieces; the context's results are untouched. */
int itsx_write_trimmed_samples(itsx_ctx *ctx, const char *const *out_paths, int32_t n_samples, int compression, int trim_ccs,
                               const char *left_prefix, const char *right_prefix, const int32_t *start, const int32_t *stop,
                               int64_t *n_written_per_sample, int64_t *total_len_per_sample);
/* ---- the feature table of the trimmed regions (a new call after the search; nothing else changes).  What a user of amplicon data
 * does next with the trimmed FASTQ files of all samples: `vsearch --derep_fulllength --sizeout --relabel_sha1` behind QIIME 2's
 * dereplicate-sequences -- a table of distinct trimmed sequences by samples plus one FASTA of representatives, the input of the
 * OTU-clustering workflows.  The reference stops at the trimmed FASTQ: these calls have no reference call site.
 * itsx_trimmed_table builds the table from what the context holds (packed reads, coordinates, samples; csrc/k_ftable.hip):
 *   counted: read i contributes iff the trimmed-FASTQ writer would write it and its slice is not empty: start[i] >= 0, stop[i] >= 0,
 *     start[i] < stop[i] and min(stop[i], len[i]) - start[i] >= min_len (min_len >= 1; the usual value is 1).
 *   bases: the read's own bases [start, min(stop, len)) as the packed read set holds them: upper case, U is T, IUPAC symbols kept
 *     (N and A differ).  No trim_ccs stitching.
 *   feature: two counted reads are one feature iff those sequences are equal symbol for symbol (forward strand only: trimmed regions
 *     are oriented; a sequence that is a prefix of another is another feature).  count[f][s] = counted reads of sample s with
 *     feature f (one column without itsx_set_samples).
 *   order: descending total count, ties by the smaller index of the feature's first read in read-set order; that read is the feature's
 *     representative.  This rule is the project's own (vsearch's order among equal sizes is not pinned against it).
 *   coordinates: either left_prefix / right_prefix (the finalized search's per-read coordinates, taken where they lie on the device, as
 *     itsx_trim_coords_device gives them) or start / stop [n_reads] from the caller -- exactly one of the two.
 *   *n_features, *n_entries (non-zero cells of the table), *n_counted (reads counted), *ms_kernels (device time of the call, by
 *     events; itsx_stats does not grow for it): each may be NULL.
 *   The table stays in the context until the next itsx_trimmed_table or the next call that makes a read set.
 *   ITSX_E_ARG: both, neither or half a coordinate source, prefixes before itsx_search_finalize, min_len < 1, no reads loaded.
 *   Limits: one context (one GPU), a whole-file read set (not a streamed chunk), forward strand only, no trim_ccs stitching. */
int itsx_trimmed_table(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix, const int32_t *start, const int32_t *stop,
                       int32_t min_len, int64_t *n_features, int64_t *n_entries, int64_t *n_counted, float *ms_kernels);
/* the table of the last itsx_trimmed_table, features in table order: feat_len / feat_total / feat_first_read [n_features]; the cells as
 * CSR rows: feature f's entries are [row_off[f], row_off[f + 1]) of entry_sample / entry_count [n_entries], samples ascending;
 * row_off [n_features + 1].  Any pointer may be NULL.  ITSX_E_ARG: no table (none made, or a new read set dropped it). */
int itsx_trimmed_table_get(itsx_ctx *ctx, int32_t *feat_len, int32_t *feat_total, int32_t *feat_first_read, int64_t *row_off,
                           int32_t *entry_sample, int32_t *entry_count);
/* the sizes of the table the context holds now (what the getters' arrays must hold); each may be NULL.  ITSX_E_ARG: no table */
int itsx_trimmed_table_size(itsx_ctx *ctx, int64_t *n_features, int64_t *n_entries, int64_t *n_counted);
/* feature_of_read [n_reads]: every read's feature (its row of the table), -1 for a read that is not counted */
int itsx_trimmed_table_reads(itsx_ctx *ctx, int32_t *feature_of_read);
/* the features' sequences, feature f's at bases[offsets[f], offsets[f + 1]) (no terminators); offsets [n_features + 1].  bases == NULL
 * fills offsets only (offsets[n_features] = the bytes bases needs); offsets may be NULL. */
int itsx_trimmed_table_seqs(itsx_ctx *ctx, char *bases, int64_t *offsets);
/* The two files of a feature table, from the arrays above (host only, no context, like itsx_write_trimmed_fastq; no reference call
 * site).  fasta_path: per feature `>label;size=total` and the sequence on one line (vsearch --sizeout's header).  tsv_path: a first
 * line `#feature`, a TAB and the TAB-joined sample names, then per feature, in table order, its label and its n_samples counts.
 * Either path may be NULL.
 * labels / label_offsets: feature f's label at labels[label_offsets[f], label_offsets[f + 1]); NULL: the id of the feature's first read --
 *   read_names[read_name_offsets[r], ...) up to the first blank or TAB -- or r%09d of that read's index where read_names is NULL.
 * sample_names / sample_name_offsets: likewise; NULL: s%d.
 * ITSX_E_ARG: missing arrays, an entry's sample outside [0, n_samples).  ITSX_E_IO: a file could not be written whole (it is removed,
 * never left short; a FASTA already written stays); itsx_writers_last_error() has the text. */
int itsx_write_feature_files(const char *fasta_path, const char *tsv_path, int64_t n_features, int32_t n_samples, const int32_t *feat_total,
                             const int32_t *feat_first_read, const int64_t *row_off, const int32_t *entry_sample, const int32_t *entry_count,
                             const char *bases, const int64_t *offsets, const char *labels, const int64_t *label_offsets,
                             const char *read_names, const int64_t *read_name_offsets, const char *sample_names,
                             const int64_t *sample_name_offsets);
/* ---- the feature table denoised into ZOTUs (a new call after itsx_trimmed_table; nothing else changes).  What a user does with a
 * table of distinct sequences: `usearch -unoise3` / `vsearch --cluster_unoise` fold every low-abundance sequence into the abundant one
 * it is an error copy of; the survivors are the ZOTUs (ASVs).  The reference stops at the trimmed FASTQ: no reference call site.
 * The rule (the project's own statement, after Edgar's UNOISE2 paper; it does not restate vsearch's k-mer candidate ranking or
 * maxrejects, and parity with usearch / vsearch is not pinned):
 *   inputs: the feature table of the last itsx_trimmed_table -- features 0 .. F-1 in table order, totals a_f, sequences s_f;
 *     max_skew[0 .. D-1], D = n_diffs in 0 .. 31, every value a double in (0, 1), non-increasing: max_skew[d-1] is UNOISE's
 *     beta(d) = 1 / 2^(alpha*d + 1), tabulated by the caller (device and model never evaluate pow); minsize >= 1.
 *   Features are processed in table order; the centroid set starts empty.  For feature q:
 *     d(q, t) is the Levenshtein distance, unit costs, global, of the two sequences as the table holds them: upper case, IUPAC
 *       symbols compared literally, so N != A.
 *     Centroid t takes q iff 1 <= d(q, t) <= D and (double)a_q <= max_skew[d-1] * (double)a_t (one IEEE multiply and one compare,
 *       no FMA).
 *     If some centroid takes q, q joins the one with the smallest d, ties going to the smallest feature index t:
 *       zotu_of_feature[q] is that centroid's ZOTU, dist_of_feature[q] = d.
 *     Else if a_q >= minsize, q becomes a centroid: the next ZOTU, dist 0.
 *     Else q is unassigned: zotu_of_feature[q] = -1, dist -1; its reads leave the denoised table and are counted in n_dropped_reads.
 *   ZOTUs are numbered in the order their centroids appear, which is table order.  A ZOTU's row is the sample-wise sum of its members'
 *   rows, CSR with samples ascending; zotu_total is the sum of the members' totals and need not descend.
 *   n_diffs == 0 is valid: nothing is taken, every feature with a_q >= minsize is a ZOTU.
 *   *n_zotus, *n_entries (non-zero cells of the denoised table), *n_dropped_reads, *n_pairs ((feature, centroid) pairs that reached the
 *   distance kernel), *ms_kernels (device time of the call, by events; itsx_stats does not grow for it): each may be NULL.
 *   The result stays in the context until the next itsx_denoise_table, the next itsx_trimmed_table or the next call that makes a read set.
 *   ITSX_E_ARG: no table, n_diffs outside 0 .. 31, a skew outside (0, 1) or above the one before it, minsize < 1.
 *   Limits: one context (one GPU), whole-file read sets, no chimera step (uchime3_denovo is another step), unassigned reads are dropped,
 *   not mapped back at 97 %.  Cost: three launches per level of the schedule, at most 1 + ln(largest total) / ln(1 / max_skew[0]) levels and
 *   never more than n_features: a max_skew[0] close to 1 is answered correctly, but slowly. */
int itsx_denoise_table(itsx_ctx *ctx, const double *max_skew, int32_t n_diffs, int32_t minsize, int64_t *n_zotus, int64_t *n_entries,
                       int64_t *n_dropped_reads, int64_t *n_pairs, float *ms_kernels);
/* the denoised table of the last itsx_denoise_table: zotu_feature (the centroid's feature) / zotu_total [n_zotus]; ZOTU z's cells are
 * [row_off[z], row_off[z + 1]) of entry_sample / entry_count [n_entries], samples ascending; row_off [n_zotus + 1].  Any pointer may be
 * NULL.  ITSX_E_ARG: no denoised table. */
int itsx_denoise_table_get(itsx_ctx *ctx, int32_t *zotu_feature, int32_t *zotu_total, int64_t *row_off, int32_t *entry_sample,
                           int32_t *entry_count);
/* zotu_of_feature / dist_of_feature [n_features]; either may be NULL */
int itsx_denoise_table_features(itsx_ctx *ctx, int32_t *zotu_of_feature, int32_t *dist_of_feature);
/* how the last call went (for profiles): the levels of its schedule, the (feature, centroid) pairs left out before any distance work
 * by the skew (dmax == 0) and by the length difference (> dmax), and the target symbols the distance kernel stepped over all its pairs
 * (a pair stops at the column where its score passes its cut-off); each may be NULL */
int itsx_denoise_table_info(itsx_ctx *ctx, int64_t *n_levels, int64_t *n_skipped_skew, int64_t *n_skipped_length, int64_t *n_columns);
/* ---- a merged read set that keeps its ORIGINAL pairs (opt-in; off by default; independent of itsx_keep_records).  While on,
 * itsx_merge_pairs_load and itsx_merge_pairs_load_files also keep, in device memory beside the merged read set, every pair's R1 and
 * R2 record: the bases and qualities as the merge kernel read them (its own upload, taken over instead of freed), both whole title lines ('@' and any comment included, no CR), and per pair the merged read whose
 * coordinates it is sliced with -- the read that R1's identifier (the title after '@' up to the first blank or TAB) NAMES among
 * the merged reads of the SAME sample, the first of equal labels, as Dedup looks record1.id up in the sample's dictionary; a pair
 * that did not merge but carries a merged pair's identifier has one.  The merge reads upper-case bases, so pairs whose files hold a
 * lower-case base keep NO pair records (slices of the upload would not be the input's bytes): itsx_write_trimmed_paired_samples
 * then returns ITSX_E_ARG and the caller uses itsx_write_trimmed_paired.  itsx_merge_pairs_load_text keeps none.  Released with the
 * read set (whatever replaces it) and by itsx_orient_apply.  Cost: R1 + R2 bases, qualities and titles stay resident. */
int itsx_keep_pair_records(itsx_ctx *ctx, int on);
/* f1 for a batch of paired samples: Dedup.create_paired_trimmed_seqs (itsxpress/SeqSample.py:564-790) of every sample in one call,
 * from the pair records the context keeps (itsx_keep_pair_records).  out1_paths[s] / out2_paths[s] receive exactly the records
 * itsx_write_trimmed_paired writes for sample s's own R1 / R2 files, its merged reads' labels and its slice of the coordinates:
 * a pair is written (both sides) iff its read has start >= 0, stop >= 0 and start < stop; R1[start:stop] ([start:] where
 * stop > tlen) and R2[tlen - stop : tlen - start], clamped as Python clamps a slice.  Both entries NULL: that sample is skipped;
 * a sample that writes nothing still gets its two empty files (gzip / zstd: a valid empty member).
 * Coordinates: either left_prefix / right_prefix (the finalized search's per-read coordinates, taken where they are on the
 * device), or start / stop / tlen [n_reads] from the caller -- exactly one of the two, and all three arrays.
 * compression: 0 plain, 1 gzip, 2 zstd, 3 gzip deflated on the device (below).  n_written_per_sample: [n_samples] pairs written, may be NULL.
 * ITSX_E_ARG: no pair records (the message names itsx_keep_pair_records), n_samples != itsx_num_samples, one path of a sample's two
 * NULL, both, neither or part of a coordinate source, prefixes before itsx_search_finalize.  ITSX_E_IO: zstd requested but not
 * available, or a file could not be written whole: then every file this call was given is removed (R1's files are written before
 * R2's, so no half of a pair of files is left behind). */
int itsx_write_trimmed_paired_samples(itsx_ctx *ctx, const char *const *out1_paths, const char *const *out2_paths, int32_t n_samples,
                                      int compression, int trim_ccs, const char *left_prefix, const char *right_prefix,
                                      const int32_t *start, const int32_t *stop, const int32_t *tlen, int64_t *n_written_per_sample);
/* ---- gzip output deflated on the device (opt-in).  compression == 3 in the two calls above means "gzip, deflated on the device":
 * the text k_trim.hip leaves in device memory is cut into blocks of at most itsx_deflate_block_bytes() bytes, none across two files,
 * csrc/k_deflate.hip turns every block into one independent gzip member (greedy LZ77 matches from a 4-byte hash, dynamic Huffman
 * codes, stored blocks where those are not larger; CRC-32 and ISIZE per member), and only the members come back to the host, where a
 * file is its members written one after another -- the "concatenated gzip members" the host writers make too.  Same records, other
 * bytes, a ratio like a fast deflate level's; the same input gives the same bytes on every run.  An empty file is one empty member.
 * Everything else about the two calls stays: a NULL path is skipped, a file that could not be written whole is removed, and a failed
 * paired call leaves neither file of a pair.  With ITSX_DEVICE_DEFLATE=1 in the environment, compression == 1 takes this path in these
 * two calls.  The host-only writers (itsx_write_trimmed_fastq, itsx_write_trimmed_paired) have no device text and refuse 3; so does
 * itsx_twriter_open, whose writer takes the device path through itsx_twriter_set_device instead (below).  Device memory: a fixed scratch of about 0.4 GB for any size of batch.  itsx_stats.ms_deflate: the kernel's time. */
int64_t itsx_deflate_block_bytes(void);
/* the most bytes itsx_deflate_device can write for nbytes of text in n_ranges ranges (host only) */
int64_t itsx_deflate_bound(int64_t nbytes, int32_t n_ranges);
/* The coder by itself, for any bytes: ranges [bounds[r], bounds[r + 1]) of text (bounds[0] = 0, bounds[n_ranges] = nbytes, non-decreasing)
 * go to the device and range r's members arrive in out[out_bounds[r], out_bounds[r + 1]) (out_bounds: n_ranges + 1 entries).
 * ITSX_E_ARG: out_cap below itsx_deflate_bound(nbytes, n_ranges), or bounds that do not tile the text. */
int itsx_deflate_device(itsx_ctx *ctx, const char *text, int64_t nbytes, const int64_t *bounds, int32_t n_ranges, char *out, int64_t out_cap,
                        int64_t *out_bounds);
/* ---- gzip input inflated on the device (opt-in).  A gzip file made of independent members -- what this library's writers produce
 * (one member per 4 MiB of text from the host writer, one per itsx_deflate_block_bytes() from the device deflate), what bgzip produces,
 * any cat a.gz b.gz -- is as parallel as it has members: csrc/k_inflate.hip finds the member starts with a strict test of every
 * position, plans the text from the members' ISIZE fields and decodes one member per wave, each verifying its own length, CRC-32
 * and ISIZE.  A general single-stream file is not taken (ITSX_INFLATE_MEMBER_KB, default 8192: the longest compressed member).
 * gzip of independent members -> text, on the device.  The text stays in a buffer of the context.
 * ITSX_OK: the device did the work.  ITSX_E_UNSUPPORTED: it DECLINED (not gzip, byte 0 no member start, a member too long, a member
 * that did not verify, no memory); itsx_last_error names the reason and the member, and nothing half-made is left behind.
 * itsx_stats.ms_inflate: the kernels' time; n_inflate_device / n_inflate_declined count the files of either kind. */
int itsx_inflate_device(itsx_ctx *ctx, const char *gz, int64_t nbytes, int64_t *text_len, int64_t *n_members);
/* the text of the last successful itsx_inflate_device (ITSX_E_ARG: there is none, or out_cap is below its length) */
int itsx_inflate_fetch(itsx_ctx *ctx, char *out, int64_t out_cap);
/* inflate_codes.h on the host, one thread, no device: the same routine member by member (tests, sanitizer program).  *reason: 0 or
 * the refusal's code; text_len / n_members count the members that verified, and out holds their text alone. */
int itsx_debug_inflate_host(const char *gz, int64_t nbytes, char *out, int64_t out_cap, int64_t *text_len, int64_t *n_members, int32_t *reason);
/* the strict member-start test (inflate_codes.h: ic_candidate) at every position, on the host: the number of positions that pass; the
 * first cap of them to positions (tests) */
int64_t itsx_debug_inflate_candidates(const char *gz, int64_t nbytes, int64_t *positions, int64_t cap);
/* after a successful itsx_inflate_device of n members: per member (file order) workgroup << 32 | the number of members that workgroup
 * of k_inflate had decoded before it (tests: which members followed which on one workgroup) */
int itsx_debug_inflate_where(itsx_ctx *ctx, int64_t *where, int64_t n);
/* opt in per context: the context's whole-file loaders (itsx_load_reads_file, itsx_load_reads_files, the merge loaders) try the device
 * first for a gzip file; a file it declines is inflated by the host exactly as without this.  ITSX_DEVICE_INFLATE=1 does the same. */
int itsx_set_device_inflate(itsx_ctx *ctx, int on);
/* ---- FASTQ text parsed on the device (opt-in).  csrc/k_fastq.hip indexes the lines of a text that lies in device memory, checks every
 * record by the rule of csrc/fastq_rec.h and gathers bases, qualities and title lines into planes.  The rule accepts exactly the texts
 * that are 4 lines per record throughout (no blank line anywhere, no FASTA), and for those the records are the host parser's byte for
 * byte; any other text is DECLINED, which is no error: the host parser then decides what the text is.
 * text -> records, on the device (the text goes up through the staging buffers).  keep_qual == 0: no quality plane is made.
 * ITSX_OK: *n_records records lie in the context (itsx_parse_fetch).  ITSX_E_UNSUPPORTED: declined; itsx_last_error names the reason
 * and the record, and nothing is left to fetch.  itsx_stats.ms_parse: the kernels' time; n_parse_device / n_parse_declined count the
 * texts of either kind. */
int itsx_parse_device(itsx_ctx *ctx, const char *text, int64_t nbytes, int keep_qual, int64_t *n_records);
/* a range of one plane of the last successful itsx_parse_device: ITSX_PARSE_OFF / ITSX_PARSE_TOFF elements [lo, hi) of the n + 1
 * offsets of the bases / title lines (out: int64_t), ITSX_PARSE_SEQ / ITSX_PARSE_QUAL / ITSX_PARSE_TITLES bytes [lo, hi) of the
 * bases, the qualities, the title lines ('@' included, no line end).  ITSX_E_ARG: no parse to fetch from, no such plane (qualities that
 * were not kept), a range outside the plane. */
#define ITSX_PARSE_OFF 0
#define ITSX_PARSE_TOFF 1
#define ITSX_PARSE_SEQ 2
#define ITSX_PARSE_QUAL 3
#define ITSX_PARSE_TITLES 4
int itsx_parse_fetch(itsx_ctx *ctx, int32_t plane, int64_t lo, int64_t hi, void *out);
/* csrc/fastq_rec.h on the host, one thread, no device (tests, sanitizer program).  *reason: 0 or the decline's code, *bad_record the
 * record it shows at (-1: the text as a whole).  off / toff: cap_records + 1 entries; seq, qual (may be NULL: not kept): cap_bases
 * bytes; titles: cap_titles bytes.  ITSX_OK, ITSX_E_UNSUPPORTED (declined: nothing written), ITSX_E_ARG (a buffer too small: nothing
 * written, and *n_records, *n_bases, *n_title_bytes say what is needed). */
int itsx_debug_parse_host(const char *text, int64_t nbytes, int64_t *off, int64_t *toff, int64_t cap_records, char *seq, char *qual, int64_t cap_bases,
                          char *titles, int64_t cap_titles, int64_t *n_records, int64_t *n_bases, int64_t *n_title_bytes, int32_t *reason, int64_t *bad_record);
/* ---- a PAIR of texts (R1, R2) parsed on the device: each text into a plane set of its own (side 0: R1, side 1: R2) by the same rule,
 * then one pass over both sides' planes (csrc/k_fastq.hip: k_fastq_pairs) does what the host path does between its parser and the merge
 * kernel: bases 'a'..'z' become upper case in place, every quality byte is held against 33..126, the longest pair is measured.  Nothing
 * is merged.  *flags: bit 0 / 1 = upper-casing changed a base of R1 / R2, bit 2 / 3 = a quality of R1 / R2 lies outside 33..126;
 * *max_total: the largest R1 + R2 length of a pair (no pairs: 0).  ITSX_E_UNSUPPORTED: declined -- a text the rule declines, or texts of
 * unequal record counts; itsx_last_error names the reason, and nothing is left to fetch.  Counters as itsx_parse_device, per text. */
int itsx_parse_pairs_device(itsx_ctx *ctx, const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int64_t *n_pairs, int32_t *flags, int64_t *max_total);
/* itsx_parse_fetch for one side (0: R1, 1: R2) of the last successful itsx_parse_pairs_device; the qualities are always kept */
int itsx_parse_pairs_fetch(itsx_ctx *ctx, int32_t side, int32_t plane, int64_t lo, int64_t hi, void *out);
/* the same result on the host, one thread, no device (tests, sanitizer program): csrc/fastq_rec.h's fq_parse_host per text and the host
 * twin of the pass.  Buffers per side as itsx_debug_parse_host's, the caps hold for either side; sizes[4]: bases and title bytes of R1,
 * then of R2.  *reason: 0, a text's decline code (*bad_side 0 / 1, *bad_record as there) or 7: unequal record counts (*bad_side -1).
 * ITSX_OK, ITSX_E_UNSUPPORTED (declined: nothing written), ITSX_E_ARG (a buffer too small: nothing written, *n_pairs and sizes say what
 * is needed). */
int itsx_debug_parse_pairs_host(const char *text1, int64_t nbytes1, const char *text2, int64_t nbytes2, int64_t *off1, int64_t *toff1, char *seq1, char *qual1, char *titles1,
                                int64_t *off2, int64_t *toff2, char *seq2, char *qual2, char *titles2, int64_t cap_records, int64_t cap_bases, int64_t cap_titles,
                                int64_t *n_pairs, int64_t *sizes, int32_t *flags, int64_t *max_total, int32_t *reason, int32_t *bad_side, int64_t *bad_record);
/* the host twin of the pass alone, over one side's planes of nbytes bytes: seq is upper-cased in place, *flags = bit 0 (a base changed)
 * | bit 2 (a quality outside 33..126) */
int itsx_debug_pair_pass_host(char *seq, const char *qual, int64_t nbytes, int32_t *flags);
/* opt in per context: itsx_load_reads_file, itsx_load_reads_text and itsx_load_reads_files (with or without itsx_keep_records) parse on
 * the device.  A text the device inflate produced (itsx_set_device_inflate) is parsed where it lies and never reaches the host or its
 * text cache -- a host consumer that wants the file later reads it again, as on any cache miss; any other text is uploaded once.
 * Only the offsets and the title lines come back; the bases stay on the device (fetched when rep.fa or the seeds' sequences are asked
 * for).  One declined text makes the whole call start over on the host path: results and errors are that path's.
 * The paired merge loaders (itsx_merge_pairs_load, itsx_merge_pairs_load_files, itsx_merge_pairs_load_text) do the same with both texts
 * of every sample: R1 and R2 go into a plane set each, k_fastq_pairs upper-cases and checks them there, the merge kernel reads them where
 * they lie and itsx_keep_pair_records keeps them; only offsets, R1's title lines and the counts come back.  They start over on the host
 * path also where R1 and R2 of a sample differ in their record counts, a quality lies outside 33..126 or a pair is longer than 12000
 * bases, so those errors are the host path's too.  The streamed loaders, itsx_load_reads_file_shard, itsx_merge_pairs_files and the
 * orient loaders parse on the host.  ITSX_DEVICE_PARSE=1 does the same. */
int itsx_set_device_parse(itsx_ctx *ctx, int on);
/* csrc/deflate_codes.h on the host (no context, no device): the code lengths the kernel gives n <= 288 symbols of these counts (sum
 * below 2^32) under a limit of maxbits (1..15, n <= 2^maxbits).  lengths: [n]. */
int itsx_debug_huffman_lengths(const uint32_t *freq, int32_t n, int32_t maxbits, uint8_t *lengths);

/* ---- a1: SeqSample.deduplicate (itsxpress/SeqSample.py:93-131)
 * = vsearch --fastx_uniques --strand both; vsearch's --minseqlength default is 1 for this command (32 for the clustering
 * commands): SeqSample.deduplicate passes 1, shorter reads are dropped (rep_of -1). */
int itsx_derep(itsx_ctx *ctx, int strand_both, int minseqlength, int64_t *n_unique);
/* ---- a2: SeqSample.cluster (itsxpress/SeqSample.py:133-176) = vsearch --cluster_size --id X --strand both:
 * greedy centroid clustering in label order (8-mer candidate ranking, global alignment, --iddef 2 identity,
 * maxaccepts 1 / maxrejects 32), restated in oracle/orc_cluster.c (parity unpinned: the reference holds no
 * fixture for it).  id == 1.0 is exact dereplication (itsx_derep), which is what the reference runs at 1.0
 * (main.py:534-537).  Fills the same arrays as itsx_derep. */
int itsx_cluster(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique);
/* itsx_cluster with the centroid stream (the quadratic term) spread over `ctx` and n_helpers more contexts, one shard each.
 * Same results as itsx_cluster(ctx, ...) bit for bit, whatever n_helpers and whichever devices the helpers sit on.
 * Helpers need no reads or profiles; they are only borrowed for the call. n_helpers == 0 is itsx_cluster. id == 1.0 is
 * itsx_derep as in itsx_cluster. */
int itsx_cluster_multi(itsx_ctx *ctx, itsx_ctx *const *helpers, int32_t n_helpers, double id, int strand_both, int64_t *n_unique);
/* after itsx_cluster at id < 1: pct_id[n_reads] = identity of each member with its centroid (uc column 4; -1 for
 * centroids and dropped reads), order[n_order] = kept reads in processing order (the order of uc's S/H rows). */
int itsx_get_cluster(const itsx_ctx *ctx, double *pct_id, int64_t *order, int64_t *n_order);
/* a2 for every sample of a batch (itsx_set_samples): SeqSample.cluster (itsxpress/SeqSample.py:133-176), which the QIIME 2
 * plugin runs once per sample at cluster_id < 1 (itsxpress/q2_itsxpress.py:287-290), in one call.  Each sample is clustered
 * exactly as itsx_cluster clusters that sample's reads alone: label order inside the sample, --minseqlength 32, DUST,
 * maxaccepts 1 / maxrejects 32, --iddef 2; a member's centroid, strand and pct_id are those of the solo run.  The samples'
 * windows advance side by side (k_cluster.hip: segmented windows).  Fills the same arrays as itsx_cluster, and the per-unique
 * sample that itsx_search keeps domZ by; itsx_get_cluster's order is the samples' processing orders, sample after sample.
 * id == 1.0 is itsx_derep(ctx, strand_both, 32, ...) on the batch; with S == 1 this is itsx_cluster. */
int itsx_cluster_samples(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique);
/* ---- column 8 of the --uc file of itsxpress/SeqSample.py:147-162 (opt-in; the text form is the USEARCH / vsearch uc format's,
 * parity unpinned as for the rest of a2: DESIGN.md 2).
 * itsx_align_clusters: after itsx_cluster / itsx_cluster_multi / itsx_cluster_samples at id < 1, aligns every member with its
 *   centroid once more and keeps the path (csrc/k_cigar.hip): global, the member on the strand itsx_get_derep reports, the cell
 *   definition of the clustering; among the paths of the optimal (score, matches, -counted columns), walking back from the end:
 *   the diagonal where it reproduces the cell, else the gap that consumes a centroid symbol, else the gap that consumes a member
 *   symbol, and a gap extends in preference to closing.  n_aligned = members that have a text, ms_kernels = device time of the
 *   sweeps and walks; either may be NULL.  ITSX_E_ARG before a clustering, and after itsx_derep or id == 1.0 (exact dereplication
 *   has nothing to align: its file keeps '*', as vsearch's does).  ITSX_CIGAR_MB caps the direction bits of one batch of pairs; a
 *   pair larger than it runs alone.
 * itsx_get_cluster_cigars: read r's text is text[offs[r] .. offs[r + 1]): run-length encoded, M a column with a symbol of each read,
 *   I a centroid symbol opposite a gap in the member, D a member symbol opposite a gap in the centroid, a run of one without its
 *   count; the single character '=' for a member that equals its centroid symbol for symbol on its strand (never aligned); empty
 *   for a centroid or a dropped read.  text == NULL fills offs only (offs[n_reads] = bytes needed).  ITSX_E_ARG when no alignments
 *   exist for the current clustering: a new read set, itsx_derep and every itsx_cluster* drop them.
 * itsx_write_uc prints column 8 of every H row from them while they exist (also under itsx_select_sample), and '*' otherwise;
 *   100 * matches / counted columns of the printed path is itsx_get_cluster's pct_id, the same double. */
int itsx_align_clusters(itsx_ctx *ctx, int64_t *n_aligned, float *ms_kernels);
int itsx_get_cluster_cigars(const itsx_ctx *ctx, int64_t *offs /* [n_reads + 1] */, char *text);
/* Dedup.parse's matchdict (itsxpress/SeqSample.py:542-562) as arrays over reads:
 * rep_of[i] = read index of the cluster seed (first occurrence), -1 if the read was dropped;
 * strand[i] = +1 / -1 (uc column 5); uniq_of[i] = index into the unique list, -1 if dropped. */
int itsx_get_derep(const itsx_ctx *ctx, int64_t *rep_of, int8_t *strand, int64_t *uniq_of);
/* ---- multi-GPU exact dereplication (SURVEY 8e option 2; itsxpress_amd/dist.py:global_derep).
 * itsx_unique_keys: XXH64 (given seed) of each local unique's packed forward strand and of its reverse complement,
 * to be exchanged between ranks.  itsx_set_active_uniques: active[U] != 0 keeps a unique in the set the HMM stages
 * score (a unique whose global first occurrence lives on another rank is scored THERE); inactive uniques get no
 * domains, their coordinates arrive through the exchange.  A later itsx_derep / itsx_cluster resets the set. */
int itsx_unique_keys(itsx_ctx *ctx, uint64_t seed, uint64_t *fwd, uint64_t *rc);
int itsx_set_active_uniques(itsx_ctx *ctx, const uint8_t *active);
/* read index of each unique (rep.fa order = input order of seeds), abundance of its cluster */
int itsx_get_uniques(const itsx_ctx *ctx, int64_t *seed_read, int64_t *abundance);

/* ---- a4: SeqSample._search (itsxpress/SeqSample.py:178-225)
 * = hmmsearch --domtblout -T <T> --F1 --F2 --F3 (domE = 10).  With the reference's flags (F1 == F2) the Viterbi filter never
 * runs; with F2 < F1 (hmmsearch's own defaults: 0.02, 1e-3, 1e-5) it runs between the bias filter and Forward (k_vit).
 * itsx_search runs every stage up to per-sequence reporting and counts, per profile, the
 * reported representatives (hmmsearch's domZ).  itsx_search_finalize applies the
 * domain threshold.  Between the two a multi-GPU driver all-reduces domZ. */
int itsx_search(itsx_ctx *ctx, double T, double F1, double F2, double F3);
/* What itsx_search keeps of hmmsearch's per-domain table (--domtblout, itsxpress/SeqSample.py:190-209).  The reference's only
 * consumer, ItsPosition.parse/_score (SeqSample.py:400-461), keeps per target and side the first row with the strictly greatest
 * %.1f score and drops the rest:
 *   ITSX_ROWS_FULL     every row stays resident (itsx_get_domains / itsx_write_domtbl work): what _search needs with --keeptemp;
 *   ITSX_ROWS_COMPACT  every pair is evaluated, only the rows that can still win that argmax once domZ is known are kept;
 *   ITSX_ROWS_LAZY     pairs that cannot win it are not evaluated past their Forward score (csrc/k_lazy.hip: a rigorous bound of
 *                      a pair's best domain score from its Forward score); coordinates are exactly those of the other modes.
 * In the last two the row table / domtbl.txt are refused -- unless the caller asks for the KEPT rows: itsx_set_kept_rows(ctx, 1)
 * makes itsx_num_domains / itsx_get_domains / itsx_write_domtbl serve, after itsx_search_finalize, the WINNERS among the rows the context
 * holds: per target and 2-character profile prefix the reported row ItsPosition's argmax ends up with -- a row of the full table, field
 * for field, in --domtblout order.  ItsPosition.parse (SeqSample.py:400-461) reads the same dictionary out of that domtbl.txt as out of
 * the full one (itsxpress_amd/SeqSample.py: ITSXPRESS_DOMTBL=winners); the '#' / 'of' columns count the listed rows of the target.
 * mode -1 (the default) reads the environment at every search: ITSX_ROWS=full|compact|lazy, or ITSX_COMPACT_ROWS=1.
 * After a LAZY search hmmsearch's domZ is known by bounds only: itsx_get_domz / itsx_set_domz / itsx_domz_device move
 * itsx_domz_count() = 2 x n_samples x n_profiles counters (lower bounds, then upper bounds; a multi-rank driver sums both).
 * itsx_search_finalize decides every row both bounds decide alike.  itsx_lazy_pending() = rows left undecided that could change
 * a coordinate (itsx_trim_coords refuses while it is positive): see itsx_lazy_complete. */
enum { ITSX_ROWS_FULL = 0, ITSX_ROWS_COMPACT = 1, ITSX_ROWS_LAZY = 2 };
int itsx_set_rows_mode(itsx_ctx *ctx, int mode);
int itsx_set_kept_rows(itsx_ctx *ctx, int on);
int64_t itsx_lazy_pending(const itsx_ctx *ctx);
/* The profiles of the undecided rows (flags[n_profiles], 1 = some row of this profile is pending), and the cure: itsx_lazy_complete
 * sends EVERY pair of the flagged profiles through the domain pipeline, after which their counters are exact (lower == upper) and
 * every row of theirs is decided.  Alone, itsx_search_finalize does this by itself; a multi-rank driver ORs the flags over the
 * ranks, completes on every rank, exchanges the counters again and finalizes again. */
int itsx_lazy_pending_profiles(const itsx_ctx *ctx, int32_t *flags);
/* The representatives of the undecided rows (flags[n_unique]); itsx_set_partial_coords(ctx, 1): itsx_rep_coords / itsx_trim_coords
 * answer although rows are undecided -- the caller promises not to use the flagged representatives' coordinates (a streaming driver
 * finalizes a chunk with provisional bounds, writes what is decided and comes back for the rest: itsxpress_amd/stream.py). */
int itsx_lazy_pending_uniques(itsx_ctx *ctx, uint8_t *flags);
int itsx_set_partial_coords(itsx_ctx *ctx, int on);
int itsx_lazy_complete(itsx_ctx *ctx, const int32_t *flags);
/* The top-up round of itsx_search_finalize runs count-only (ITSX_TOPUP_COUNT_ONLY=0: as a third lazy round): it is there for the lower
 * bounds on domZ, so a pair with a multidomain region is deferred -- unevaluated, on the upper bound's side -- instead of taking the
 * ensemble stage, and no rows are kept.  counters[0] = pairs the last search's round deferred; counters[1] = 1 when rows of its profiles
 * were still undecided and the deferred pairs went through the ordinary pipeline in a second sub-round, else 0.  (Counters of their own
 * and not fields of itsx_stats: that structure's size and last fields are fixed by its readers.) */
int itsx_topup_counters(const itsx_ctx *ctx, int64_t *counters /* [2] */);
int64_t itsx_domz_count(const itsx_ctx *ctx);
int itsx_get_domz(const itsx_ctx *ctx, int64_t *domZ /* [itsx_domz_count]: [n_samples][n_profiles] (x 2 after a lazy search) */);
int itsx_set_domz(itsx_ctx *ctx, const int64_t *domZ /* same */);
int itsx_search_finalize(itsx_ctx *ctx, double domE);
int64_t itsx_num_domains(const itsx_ctx *ctx);
int itsx_get_domains(const itsx_ctx *ctx, itsx_domain *rows /* [itsx_num_domains] */);
/* ---- the hmm / ali / acc columns of the --domtblout file of itsxpress/SeqSample.py:191-209 (opt-in; a restatement of hmmsearch's
 * optimal-accuracy stage, parity unpinned: DESIGN.md 2).
 * itsx_align_domains: after itsx_search_finalize, aligns every resident row with dom_reported == 1 (unihit local mode over its
 *   envelope, the length model at the target's length; the posteriors are the ones the row's null2 correction was summed from).
 *   n_aligned = rows aligned (a pair a lazy search evaluated twice counts twice), ms_kernels = device time of the three sweeps;
 *   either may be NULL.  ITSX_E_ARG before a finalize; where itsx_get_domains refuses, the same code; an envelope whose
 *   posteriors are not finite is ITSX_E_UNSUPPORTED with the row named.  ITSX_ALIGN_SLAB_MB caps the slab of one batch of waves.
 * itsx_get_alignments: out[k] belongs to row k of itsx_get_domains (aligned = 0, all zero, where that row is not reported).
 *   ITSX_E_ARG when no alignments exist for the current finalize: a new read set, itsx_derep / itsx_cluster*, itsx_search,
 *   itsx_search_finalize, itsx_lazy_complete, itsx_set_domz and itsx_debug_set_domains drop them.
 * itsx_write_domtbl prints the real columns for every aligned row while alignments exist, and today's placeholders otherwise. */
int itsx_align_domains(itsx_ctx *ctx, int64_t *n_aligned, float *ms_kernels);
int itsx_get_alignments(const itsx_ctx *ctx, itsx_alignment *out /* [itsx_num_domains] */);
int64_t itsx_num_pairtraces(const itsx_ctx *ctx);
/* row_size = sizeof(itsx_pairtrace) as the CALLER was compiled: a library built from other sources is refused (ITSX_E_ARG) instead of
 * writing rows of another stride */
int itsx_get_pairtraces(const itsx_ctx *ctx, itsx_pairtrace *rows, int64_t row_size);

/* ---- a5/a6/a7: ItsPosition.parse/_score/get_position (itsxpress/SeqSample.py:400-498)
 * composed with Dedup.matchdict: per READ, start = left.env_to, stop = right.env_from - 1,
 * tlen = length of the representative; -1 where the reference returns None; in_ddict[i] = 0
 * where ItsPosition.get_position would raise KeyError (or the read was dropped). */
int itsx_trim_coords(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix,
                     int32_t *start, int32_t *stop, int32_t *tlen, int32_t *in_ddict);
/* same, per unique representative */
int itsx_rep_coords(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix,
                    int32_t *start, int32_t *stop, int32_t *tlen, int32_t *in_ddict);

/* ---- device-resident exchange for multi-GPU drivers (itsxpress_amd/dist.py; RCCL over xGMI): the quantities the ranks
 * exchange stay in the context's device memory, so a collective library reduces / gathers / scatters them where they are.
 * Every pointer is valid until the next call that recomputes the same quantity on this context.
 * itsx_domz_device: after itsx_search, int64[n_samples * n_profiles] reported-target counters; all-reduce them in place, then
 *   call itsx_search_finalize (it uses the device values; itsx_set_domz returns to host values).
 * itsx_trim_coords_device / itsx_rep_coords_device: int32 rows [n][4] = (start, stop, tlen, in_ddict) per read / representative.
 * itsx_derep_device: rep_of / uniq_of (int32[n_reads]), strand (int8[n_reads]), seed_read (int32[n_unique]).
 * itsx_unique_keys128_device: int64 rows [n_unique][4] = (key0, key1, gidx_base + first occurrence, 1 if the forward strand is
 *   the canonical orientation): the orientation-free 128-bit key of each local unique (two XXH64 seeds). */
int itsx_domz_device(itsx_ctx *ctx, int64_t **d_domz, int64_t *n);
int itsx_trim_coords_device(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix, int32_t **d_rows, int64_t *n_rows);
int itsx_rep_coords_device(itsx_ctx *ctx, const char *left_prefix, const char *right_prefix, int32_t **d_rows, int64_t *n_rows);
int itsx_derep_device(itsx_ctx *ctx, const int32_t **d_rep_of, const int32_t **d_uniq_of, const int8_t **d_strand, const int32_t **d_seed_read);
int itsx_unique_keys128_device(itsx_ctx *ctx, uint64_t seed_a, uint64_t seed_b, int64_t gidx_base, int64_t **d_tuples, int64_t *n_unique);
/* the same tuples copied to host memory (tuples[n_unique][4]): for a driver that has no collective library and moves them itself */
int itsx_unique_keys128(itsx_ctx *ctx, uint64_t seed_a, uint64_t seed_b, int64_t gidx_base, int64_t *tuples);

/* ---- file-compatible outputs (users pass --keeptemp; itsxpress/SeqSample.py:104-105,190) */
int itsx_write_uc(const itsx_ctx *ctx, const char *path);
int itsx_write_rep_fasta(const itsx_ctx *ctx, const char *path);
int itsx_write_domtbl(const itsx_ctx *ctx, const char *path);
/* The same three files written from ARRAYS (host-only, context-free: csrc/writers_host.cpp), for a driver that spreads ONE sample
 * over several GPUs and must hand the reference's parsers one uc.txt / rep.fa / domtbl.txt, byte for byte what one GPU writes.
 * itsx_write_derep_arrays: rep_of[i] = read index of the cluster's seed (-1 dropped), strand[i] = +1 / -1 relative to the seed,
 *   len[i], names (NULL: r%09d), the seeds' sequences concatenated in input order of the seeds; either path may be NULL.
 * itsx_write_domtbl_arrays: domain rows from any number of contexts with rep = index into target_names (the global unique list),
 *   Z = targets searched, domz[n_profiles] = the data set's reported targets per profile, per profile NAME / M / Forward tau, lambda.
 * itsx_profile_params / itsx_get_unique_seqs: what a driver needs from its contexts to fill those arrays.
 * Errors: negative code, text from itsx_writers_last_error(). */
int itsx_write_derep_arrays(const char *uc_path, const char *rep_path, int64_t n, const int64_t *rep_of, const int8_t *strand,
                            const int32_t *len, const char *names, const int64_t *name_offsets, const char *seed_bases,
                            const int64_t *seed_offs, int64_t n_seeds);
int itsx_write_domtbl_arrays(const char *path, const itsx_domain *rows, int64_t n_rows, int64_t Z, const int64_t *domz, int32_t n_profiles,
                             const char *prof_names, const int64_t *prof_name_offsets, const int32_t *prof_M, const float *prof_tau,
                             const float *prof_lambda, const char *target_names, const int64_t *target_name_offsets);
/* itsx_write_domtbl_arrays with the hmm / ali / acc columns of the --domtblout file of itsxpress/SeqSample.py:191-209 taken from
 * ali[n_rows], parallel to rows, wherever ali[i].aligned == 1; ali == NULL: the file of itsx_write_domtbl_arrays, byte for byte */
int itsx_write_domtbl_arrays_ali(const char *path, const itsx_domain *rows, int64_t n_rows, int64_t Z, const int64_t *domz, int32_t n_profiles,
                                 const char *prof_names, const int64_t *prof_name_offsets, const int32_t *prof_M, const float *prof_tau,
                                 const float *prof_lambda, const char *target_names, const int64_t *target_name_offsets,
                                 const itsx_alignment *ali);
const char *itsx_writers_last_error(void);
int itsx_profile_params(const itsx_ctx *ctx, int i, int32_t *M, float *evparam6);
int itsx_get_unique_seqs(itsx_ctx *ctx, char *bases, int64_t cap, int64_t *offsets);

/* labels of the loaded reads in input order (what Dedup.matchdict is keyed by, itsxpress/SeqSample.py:542-562; the paired
 * writer looks R1/R2 records up by them): concatenated into names[cap], offsets[n_reads + 1]; names == NULL fills the
 * offsets only (offsets[n_reads] = bytes needed). */
int itsx_get_read_names(const itsx_ctx *ctx, char *names, int64_t cap, int64_t *offsets);

/* out_size = sizeof(itsx_stats) as the caller was compiled (checked, like itsx_get_pairtraces' row_size) */
int itsx_get_stats(const itsx_ctx *ctx, itsx_stats *out, int64_t out_size);
/* The library's environment switches that are set ("NAME=value" lines; the registry with every switch's class -- tuning, mode,
 * diagnostic, test hook -- is csrc/switches.cpp, the table INTEGRATION.md section 7): of ctx's last search (snapshot taken when it
 * started) or, with ctx == NULL, of the environment now.  A test hook (result-changing) is honoured only under ITSX_TEST_HOOKS=1 and
 * says so here otherwise.  The reference has no such surface: it passes fixed flags (itsxpress/SeqSample.py:191-209).
 * Returns the length needed, terminator included. */
/* A context that will not search again soon (a streamed file's chunk, itsxpress_amd/stream.py) hands its largest scratch buffer -- the DP
 * slab, tens of GB -- to the next context of the process on that device; results and everything itsx_search_finalize /
 * itsx_lazy_complete need stay.  The reference has nothing of the kind (one process per tool run, itsxpress/SeqSample.py:117,210). */
int itsx_release_scratch(itsx_ctx *ctx);
int64_t itsx_switches(const itsx_ctx *ctx, char *buf, int64_t cap);
/* the registry: "NAME<tab>class<tab>meaning" lines, class = tuning | mode | diagnostic | hook */
int64_t itsx_switch_registry(char *buf, int64_t cap);

/* ---- f1 ("next"): native FASTQ parse -> slice -> write.  Host-only and context-free.
 * itsx_write_trimmed_fastq replaces Dedup.create_trimmed_seqs (itsxpress/SeqSample.py:886-949): record i of
 * seq_path (plain or .gz) is written as record[start[i]:stop[i]] iff both are >= 0 and start < stop.
 * itsx_write_trimmed_paired replaces Dedup.create_paired_trimmed_seqs (SeqSample.py:713-790): R1/R2 pair k is
 * looked up by the id of its R1 title among `names` (the merged reads the coordinates belong to) and sliced
 * with the reference's r2start = tlen - stop / r2end = tlen - start arithmetic.  trim_ccs stitches the CCS
 * primers with quality 93.  Errors: negative code, text from itsx_trim_last_error().
 * Inputs are plain, gzip or zstd (told apart by their magic bytes; the reference goes by .gz / .zst, main.py:296-330).
 * `compression` of the output: 0 plain, 1 gzip, 2 zstd (the reference's gzipped / zstd_file flags, SeqSample.py:909-925).
 * Compressed output is written as concatenated gzip members / zstd frames produced by a pool of threads
 * (ITSX_IO_THREADS, default min(hardware threads, 32)); any gzip / zstd reader sees one stream. */
int itsx_write_trimmed_fastq(const char *seq_path, const char *out_path, int compression, int trim_ccs,
                             const int32_t *start, const int32_t *stop, int64_t n_records,
                             int64_t *n_written, int64_t *total_len);
/* The same writer as an object that takes the input's TEXT and the COORDINATES piece by piece and slices / deflates on its own
 * threads while more arrive (a streaming run writes the first chunks' reads while the GPU scores the later ones).  The text is cut
 * into units at the first record start at or after every multiple of 8 MB; a unit's output is one gzip member / zstd frame, units are
 * written in order, so the file's bytes do not depend on how text and coordinates arrived: itsx_write_trimmed_fastq IS this object
 * fed once.  itsx_twriter_text: text[0, avail) is final (one address, growing; last = 1 with the final piece; the text must stay
 * valid until close).  itsx_twriter_coords: rows of records first_record .. first_record + n - 1 (record order, no gaps);
 * decided[i] == 0 (NULL: all decided) marks a record whose coordinates may still change -- it holds back its own unit only, until
 * itsx_twriter_update names it.  itsx_twriter_close waits for the pool, fails if a record was left undecided, frees the object.
 * Errors: negative code, text from itsx_trim_last_error(). */
int itsx_twriter_open(const char *out_path, int compression, int trim_ccs, itsx_twriter **w);
/* mode 1 (a paired run's mates, itsxpress/SeqSample.py:587-670): (start, stop) are Python slice bounds as they come -- start may be
 * negative, stop == INT32_MAX = open end, stop == INT32_MIN = the record is not written (ITSX_E_ARG on a writer that has strands) */
int itsx_twriter_set_mode(itsx_twriter *w, int32_t mode);
/* The writer's gzip output made on the device (opt-in): a unit that is ready has its raw text and coordinates uploaded, its lines
 * indexed, its records planned, copied and deflated by the context (csrc/k_trim.hip, csrc/k_deflate.hip: members of at most
 * itsx_deflate_block_bytes() bytes of text, cut from the start of the unit's output), and only compressed bytes come back; the host
 * keeps the count pass.  A unit with a blank line between records (or of 2^31 bytes or more) is sliced on the host and deflated on the
 * device all the same, so the file's bytes depend on the units' output text alone -- not on the arrival of text and coordinates,
 * and they are the same on every run (they differ from the host deflate's; the records do not).  Valid only on a writer opened with
 * compression 1, before any text or coordinates arrive: ITSX_E_ARG otherwise.  The writer BORROWS ctx: it must outlive
 * itsx_twriter_close and serve nothing else meanwhile, except further writers (a paired run's R1 and R2 share one: their use of it is
 * serialised).  The device buffers (a unit of text, its index and output, the deflate scratch of about 0.4 GB) are allocated here.  All
 * device work happens on one thread of the writer's own.  A HIP error marks the writer failed, nothing more is started on the device,
 * itsx_twriter_close returns ITSX_E_DEVICE and itsx_trim_last_error() names the step.  itsx_stats of ctx: ms_deflate = the deflate
 * kernel's time summed over the units so far; n_tw_units_device / n_tw_units_host = units that took the device's index, plan and copy /
 * units the host sliced.  Growth past what was reserved here (a unit of one long record, many short CCS records) allocates in mid-run and
 * can fail with ITSX_E_DEVICE when the chunk contexts have taken the memory. */
int itsx_twriter_set_device(itsx_twriter *w, itsx_ctx *ctx);
int itsx_twriter_text(itsx_twriter *w, const char *text, int64_t avail, int32_t last);
int itsx_twriter_coords(itsx_twriter *w, int64_t first_record, int64_t n, const int32_t *start, const int32_t *stop, const uint8_t *decided);
int itsx_twriter_update(itsx_twriter *w, const int64_t *records, int64_t m, const int32_t *start, const int32_t *stop);
int itsx_twriter_close(itsx_twriter *w, int64_t *n_written, int64_t *total_len);
/* Strands for the writer (a streamed run that orients its reads chunk by chunk): rows of records first_record .. first_record + n - 1,
 * in record order without gaps, BEFORE the coordinates of the same records (rows for records whose coordinates are in: ITSX_E_ARG).
 * A record of strand -1 is written from its reverse complement -- bases reversed and complemented byte by byte with the table
 * itsx_write_oriented_fastq uses (case and IUPAC symbols kept), qualities reversed -- and start / stop are the Python slice of THAT
 * record, trim_ccs stitching around it as ever: the bytes are those of the writer run over oriented.fq.  Strand +1 and 0 are written as
 * they are, and a writer that never gets this call writes what it always wrote.  Mode 0 only (ITSX_E_ARG on a mode-1 writer).  On the
 * device path the unit's strands are uploaded beside its coordinates and the copy kernel reads a flipped record's lines backwards
 * (csrc/k_trim.hip); units the host slices honour the strands there.
 * itsx_write_trimmed_fastq_strands: the object fed once (strand == NULL: itsx_write_trimmed_fastq). */
int itsx_twriter_strands(itsx_twriter *w, int64_t first_record, int64_t n, const int8_t *strand);
int itsx_write_trimmed_fastq_strands(const char *seq_path, const char *out_path, int compression, int trim_ccs,
                                     const int32_t *start, const int32_t *stop, const int8_t *strand, int64_t n_records,
                                     int64_t *n_written, int64_t *total_len);

int itsx_write_trimmed_paired(const char *r1_path, const char *r2_path, const char *out1_path, const char *out2_path,
                              int compression, int trim_ccs, const char *names, const int64_t *name_offsets, int64_t n_names,
                              const int32_t *start, const int32_t *stop, const int32_t *tlen, int64_t *n_written);
const char *itsx_trim_last_error(void);
/* The readers behind every *_file entry point, exposed for the host side (replaces gzip.open / pyzstd.open of
 * main.py:296-330 and SeqSample.py:929-949): the decompressed content of a plain / gzip / zstd file in a buffer the
 * caller releases with itsx_io_free.  itsx_io_codecs: bit 0 = libdeflate in use for gzip, bit 1 = libzstd available.
 * A single-member gzip file of more than a few MB is inflated by a pool of threads (csrc/pinflate.cpp: block starts are
 * found inside the stream, every chunk is decoded with its unknown 32-KB history as markers, the markers are resolved
 * front to back) and accepted only when length and CRC-32 match the trailer; everything else takes the serial inflater.
 * itsx_io_parallel_inflates: files delivered that way since the library was loaded (ITSX_PARALLEL_INFLATE=0 turns it off). */
int  itsx_io_read(const char *path, char **text, int64_t *len);
/* identifiers of a FASTQ file's records (title up to the first blank) through the record parser the trimming writers use:
 * names[offsets[i] .. offsets[i + 1]) is record i's; both buffers are released with itsx_io_free */
int  itsx_fastq_ids(const char *path, char **names, int64_t **offsets, int64_t *n_records);
void itsx_io_free(char *text);
int  itsx_io_codecs(void);
int64_t itsx_io_parallel_inflates(void);
/* drops the process-wide cache of decompressed texts (ITSX_TEXT_CACHE_GB; the loaders leave a file's text there for the writers) */
void itsx_io_cache_clear(void);

/* ---- test hooks (parity tests only) */
/* a hand-made domain table in place of a search's results (tests of the stage that decides every trimmed read: the domain threshold,
 * ItsPosition's argmax, the compact and lazy rows modes).  Needs loaded profiles and a finished itsx_derep / itsx_cluster.  rows[n_rows]
 * lie in n_segs segments of seg_rows[s] rows (a segment = the rows one chunk of a search leaves; empty ones allowed).  A row with
 * dom_idx < 0 is padding and stays as given; every other row must name a representative (rep < n_unique) and a profile (prof <
 * n_profiles): ITSX_E_ARG otherwise, and the context keeps what it had.  mode = ITSX_ROWS_FULL, ITSX_ROWS_COMPACT (each segment goes
 * through the compaction a search's chunk goes through, ITSX_COMPACT_ZMAX / ITSX_COMPACT_DOME_MIN honoured) or ITSX_ROWS_LAZY (the rows
 * are the kept rows).  Afterwards the context is as itsx_search leaves it in that mode, with all [sample][profile] counters zero (twice
 * as many after lazy) and dom_reported still to be set: itsx_set_domz, then itsx_search_finalize and everything behind it.  Nothing
 * can be evaluated again: itsx_search_finalize of a lazy table without itsx_set_domz, and itsx_lazy_complete, are ITSX_E_ARG. */
int itsx_debug_set_domains(itsx_ctx *ctx, const itsx_domain *rows, int64_t n_rows, const int64_t *seg_rows, int32_t n_segs, int mode);
/* the rows the context holds as they lie in its segments (segment after segment, padding included; after ITSX_ROWS_COMPACT the kept
 * rows; dom_reported as the last itsx_search_finalize left it, 2 = undecided after a lazy one): returns their number, and copies them
 * when cap holds them all; negative on error */
int64_t itsx_debug_get_rows(itsx_ctx *ctx, itsx_domain *rows, int64_t cap);
/* XXH64 of each read's packed forward / reverse-complement key, as computed on the device */
int itsx_debug_read_hashes(itsx_ctx *ctx, uint64_t *fwd, uint64_t *rc);
/* the sample of every read of a batch, [n_reads] each (either may be NULL): as the device kernels see it and as the host-side writers see
 * it; all 0 when the context holds one sample */
int itsx_debug_read_samples(itsx_ctx *ctx, int32_t *device_ids, int32_t *host_ids);
/* the length-ordered list of uniques the HMM stages walk, copied from the device (not from the host mirror): out[n_unique]; returns the
 * number of entries written (all uniques after itsx_derep / itsx_cluster, the active ones after itsx_set_active_uniques) or an error */
int itsx_debug_sorted_uniques(itsx_ctx *ctx, int32_t *out);
/* packed representation of read i: words [ceil(len/16)], exception list (pos<<4|code) */
int itsx_debug_packed_read(const itsx_ctx *ctx, int64_t i, uint32_t *words, int32_t *nwords,
                           uint32_t *exc, int32_t *nexc);
/* PMC calibration (scripts/fetch_calib.py): stream `gbytes` GB `iters` times in one of the DP slab's access patterns --
 * 0: read all 6 fields of a [row][6][64] float plane at 4 B per lane, 1: read 5 of the 6 fields (k_decode), 2: write all 6,
 * 3: read 16 B per lane -- and report the bytes one launch touches, so rocprofv3's FETCH_SIZE / WRITE_SIZE can be scaled */
int itsx_debug_calibrate(itsx_ctx *ctx, int pattern, double gbytes, int iters, int64_t *bytes_per_launch, double *ms_per_launch);
/* VALU issue-rate probe behind bench.py's valu_issue_frac (profiles/round5_valu_issue.md): op 0 v_fma_f32, 1 v_pk_fma_f32, 2 v_pk_max_i16,
 * 3 v_pk_add_u16, 4 v_pk_mul_f32, 5 v_pk_add_f32, 6 s_nop 0, 7 v_mul_f32, 8 v_pk_mov_b32, 9 v_max_i16; 10 the scalar-cache probe: two
 * s_load_dwordx8 of a 1-KB table per step, waited for one step later (what k_fwd_bound asks per pair of nodes), 11 the same under 12
 * v_pk_fma_f32 per step (scripts/scalar_probe.py); 12 v_pk_add_i16 ... clamp (the MSV filter's saturating row add); 64 x iters independent
 * instructions (steps) per
 * wave, waves_per_simd (1-4, 6, 8) waves on every SIMD; cycles_per_instr as one wave sees them (shader clock ticks, median over the waves) */
int itsx_debug_issue(itsx_ctx *ctx, int op, int waves_per_simd, int iters, double *cycles_per_instr, double *ms);
/* deterministic log/exp evaluated ON THE DEVICE for n inputs */
int itsx_debug_detmath(itsx_ctx *ctx, const double *x, int64_t n, double *out_log, double *out_exp);
/* the bias filter's table-driven float logarithm (detmath.h: det_logf_fast) ON THE DEVICE: out[i] must equal (float)det_log((double)x[i]) */
int itsx_debug_logf(itsx_ctx *ctx, const float *x, int64_t n, float *out);
/* the DUST soft mask (vsearch --qmask dust) the device computes for the current reads: masked[sum of lengths], 1 = masked */
int itsx_debug_dust(itsx_ctx *ctx, uint8_t *masked);
/* launch_exclusive_scan (k_util.hip) over n int32 values: out[i] = in[0] + ... + in[i - 1]; in_place != 0: the device scans the input
 * buffer onto itself */
int itsx_debug_scan(itsx_ctx *ctx, const int32_t *in, int64_t n, int32_t *out, int in_place);
/* One selection of the lazy stage (k_lazy.hip) over a pair list of the caller's: pairs[NP][4] = (useq, prof, xj, L), prof < 0 = padding;
 * profile p's pairs lie in [seg_start[p], seg_start[p + 1]), every bound a multiple of 64.  mode 0 / 1: round 0 / round 1 of the lazy
 * rounds -- group[n_group] is gtop indexed by useq * ncls + cls[prof] (mode 0), or bestc indexed by sorted_uniq[useq] * ncls + cls[prof]
 * (mode 1); mode 2: the top-up round's marking with slot_of_prof[P] and cutoff[2 n_slots]; mode 3: the top-up round's key list.
 * Modes 0-2: done[NP] is updated, out_seg[P + 1] receives the selected list's segments (padded to 64), *out_n its length and, when
 * out_cap holds it, out_pairs the list itself (padding records are all 0xFF).  Mode 3: *out_n = the marked pairs, out_keys / out_vals
 * (when out_cap holds them) their keys (slot << 32 | ~b10) and indices in list order.  An index that points outside a table is ITSX_E_ARG. */
int itsx_debug_select(itsx_ctx *ctx, int mode, const int32_t *pairs, int64_t NP, const int64_t *seg_start, int32_t P, uint8_t *done, const uint32_t *b10,
                      const int8_t *cls, int32_t ncls, const unsigned long long *group, int64_t n_group, const int32_t *sorted_uniq, int64_t n_sorted,
                      const int32_t *slot_of_prof, const uint32_t *cutoff, int32_t n_slots, int64_t *out_seg, int32_t *out_pairs, int64_t out_cap,
                      unsigned long long *out_keys, int32_t *out_vals, int64_t *out_n);
/* The lazy stage's pair list with pass A's scores and the bounds made from them (k_lazy.hip: k_fwd_bound, k_lazy_bound), as the last
 * itsx_search left them: only after a lazy search that ran as ONE chunk of one sample (what the top-up round of itsx_search_finalize
 * reads, so also after that call unless it had to count a profile in full); any other state is ITSX_E_ARG.  Records come as they lie in
 * the list, padding (prof < 0) and the pairs that ran for their row states only (xj < 0) included.  rep = the representative's index in
 * itsx_get_uniques order (-1 on padding), fb = pass A's Forward score (nats), b10 = the biased %.1f tenths no domain of the pair can
 * exceed (0 on padding and helpers), done = the pair went through the domain stage, nullsc / lazy_c = LenTables[L] as k_lazy_bound read
 * them.  Returns the number of records (out is filled when cap holds them), or a negative ITSX_E_*; *tenths_bias (may be NULL) = the
 * bias of b10. */
typedef struct { int64_t rep; int32_t prof, L, xj; float fb; uint32_t b10; int32_t done; float nullsc, lazy_c; } itsx_lazy_pair;
int64_t itsx_debug_lazy_pairs(itsx_ctx *ctx, itsx_lazy_pair *out, int64_t cap, int32_t *tenths_bias);
/* The envelope memoisation's table (k_derep.hip: k_region_keys, k_region_resolve) over regions of the loaded reads: regions[n][4] =
 * (pair, ienv, jenv, multi), pair < 0 = none; pairs[n_pairs][4] as above with useq = the READ's index.  rep_region[g] = the smallest
 * region with g's profile, L and residues (-1: no region), is_uniq[g] = (rep_region[g] == g).  The table has the size a search gives it. */
int itsx_debug_region_keys(itsx_ctx *ctx, const int32_t *regions, int64_t n_regions, const int32_t *pairs, int64_t n_pairs, int32_t *rep_region, int32_t *is_uniq);

#ifdef __cplusplus
}
#endif
#endif
