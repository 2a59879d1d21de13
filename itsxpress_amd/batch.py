"""Per-sample batching for callers that hold MANY samples.

The QIIME 2 plugin walks its manifest and runs the whole path once per sample
(itsxpress/q2_itsxpress.py:273-333: `_set_fastqs_and_check` -> `sobj.deduplicate` -> `sobj._search` ->
`ItsPosition` / `Dedup` -> writer, inside `for sample in samples.itertuples()`).  Amplicon samples are small
(10^4..10^5 reads), so each of those runs leaves most of an MI355X idle and pays the launch and transfer
latencies again.  `SampleBatch` takes the same `SeqSample` objects and runs the two engine steps ONCE for all of
them -- one read set, one pass of every kernel -- while every sample keeps exactly the results of its own run:

* reads are dereplicated within their sample only (representative = first occurrence inside the sample),
* hmmsearch's domZ (reported targets per profile, the factor in the domain E-value threshold) is counted per
  (sample, profile),
* `uc.txt`, `rep.fa`, `domtbl.txt` are written per sample, byte-identical to the files a run of that sample
  alone writes (tests/test_gpu_batch.py), and each `SeqSample`'s `uc_file` / `rep_file` / `dom_file` point at
  them, so the reference's `ItsPosition(...)` / `Dedup(...)` constructors and writers downstream stay as they are.

Paired samples (the plugin's main case: `_set_fastqs_and_check` -> `sobj._merge_reads` once per manifest row,
q2_itsxpress.py:72-80) join the batch UNMERGED: `merge_reads` sends the pairs of every sample through one merge kernel
(`itsx_merge_pairs_load_files`) and leaves the merged reads of all samples on the device as the batch's read set, so
`deduplicate` / `cluster_per_sample` go on from there without a `seq.fq` round trip; the per-sample `seq.fq` is written
only where a consumer reads it (file-compatible mode, or `write_seq_files=True`).

CCS samples (`trim_ccs`: the plugin calls `sobj.orient_reads()` first, q2_itsxpress.py:284-285) join the batch UNORIENTED:
`orient_reads` orients the reads of every sample in one engine call (`itsx_orient_apply`) and leaves the oriented reads on the
device as the batch's read set; each sample's `oriented.fq` is written by the host writer from its own file and strands.

Nothing here computes: the grouping, the counters and the writers live behind the C ABI
(`itsx_load_reads_files`, `itsx_merge_pairs_load_files`, `itsx_orient_apply`, `itsx_set_samples`, `itsx_select_sample`; include/itsx_hip.h).
"""
import logging
import os
from typing import List, Optional, Sequence, Union

import numpy as np

from .engine import Engine
from ._lib import EngineError
from .SeqSample import _REGION_PREFIX, _domtbl_ali_wanted, _fast_from_env, _keep_undecided, _orient_hmmfile, _uc_cigar_wanted, _winners_from_env
from .definitions import maxmismatches


def write_denoised_files(fasta, tsv, n_samples, totals, zotu_feature, row_off, entry_sample, entry_count, sequences, labels, sample_names):
    """The two files of a denoised table from its arrays, through the host formatter itsx_write_feature_files (no device): the ZOTUs'
    bases and offsets are compacted here, `size=` is the ZOTU's total.  Either path may be None."""
    from . import _lib
    import ctypes as C
    sample_names = [str(x) for x in sample_names]
    if len(sample_names) != n_samples:
        raise ValueError("write_denoised_table: %d sample names for %d sample(s)" % (len(sample_names), n_samples))

    def blob_of(names):
        enc = [x.encode() for x in names]
        return b"".join(enc), np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int64)
    bases, seq_off = blob_of(sequences)
    lab, lab_off = blob_of(labels)
    sn, sn_off = blob_of(sample_names)
    arr = lambda x, dt: np.ascontiguousarray(x, dt)
    totals, zotu_feature, row_off = arr(totals, np.int32), arr(zotu_feature, np.int32), arr(row_off, np.int64)
    entry_sample, entry_count = arr(entry_sample, np.int32), arr(entry_count, np.int32)
    pad = lambda x: x.ctypes.data if x.size else None
    L = _lib.lib()
    rc = L.itsx_write_feature_files(None if fasta is None else os.fsencode(fasta), None if tsv is None else os.fsencode(tsv),
                                    int(totals.shape[0]), int(n_samples), pad(totals), pad(zotu_feature), row_off.ctypes.data,
                                    pad(entry_sample), pad(entry_count), C.c_char_p(bases), seq_off.ctypes.data,
                                    C.c_char_p(lab), lab_off.ctypes.data, None, None, C.c_char_p(sn), sn_off.ctypes.data)
    if rc != 0:
        raise EngineError(rc, L.itsx_writers_last_error().decode())


class SampleBatch:
    """Runs `deduplicate()` and `_search()` of many SeqSample objects as one engine pass.

    samples: objects with `seq_file` and `tempdir` (the mirror's or the reference's SeqSample*), or paired samples that are not
    merged yet (`r1` and `fastq2` set, `seq_file` unset): those are merged by `merge_reads`, all in one engine call.  CCS samples
    (`trim_ccs`) join the batch unoriented and `orient_reads` orients them all in one engine call.  Method names and arguments
    follow SeqSample."""

    def __init__(self, samples: Sequence, engine: Optional[Engine] = None, subdirs: Optional[Sequence[str]] = None,
                 keep_records: Union[bool, str] = False) -> None:
        self.samples = list(samples)
        if not self.samples:
            raise ValueError("SampleBatch needs at least one sample")
        for s in self.samples:
            paired = getattr(s, "r1", None) is not None and getattr(s, "fastq2", None) is not None
            if getattr(s, "seq_file", None) is None and not paired:
                raise ValueError("every sample needs its seq_file, or r1 and fastq2 for merge_reads(), before batching")
        self.engine = engine if engine is not None else Engine()
        # the plugin gives every sample the same tempdir and overwrites uc.txt / rep.fa / domtbl.txt per sample;
        # a batch holds them all at once, so each sample writes into its own sub-directory
        self.subdirs = list(subdirs) if subdirs is not None else ["sample_%04d" % i for i in range(len(self.samples))]
        self.counts: Optional[np.ndarray] = None       # reads per sample
        self.first: Optional[np.ndarray] = None        # index of each sample's first read in the batch
        self.n_pairs: Optional[np.ndarray] = None      # after merge_reads: read pairs per sample
        self.n_joined: Optional[np.ndarray] = None     # after merge_reads: of them joined, not merged, per sample (merge_join; else zeros)
        self._resident = None                          # the seq_files whose reads merge_reads / orient_reads left resident in the engine,
        self._resident_read_set = None                 # and the engine's read-set number at that moment (the engine may be shared)
        self._seq_written = False                      # whether they wrote those files
        self._resident_from = "merge_reads"            # which of the two it was (for the messages)
        # keep_records: the read sets this batch makes keep their FASTQ records on the device (itsx_keep_records) and write_trimmed cuts
        # every sample's output from them in one engine call -- no seq.fq / oriented.fq in between
        # keep_records="pairs": all of that, and merge_reads also keeps the ORIGINAL R1 / R2 records of every pair on the device
        # (itsx_keep_pair_records): write_paired_trimmed cuts every sample's two files from them in one engine call, so the inputs are
        # read once
        if isinstance(keep_records, str) and keep_records != "pairs":
            raise ValueError('keep_records is False, True or "pairs"')
        self.keep_records = bool(keep_records)
        self.keep_pair_records = keep_records == "pairs"
        self._records_read_set = None                  # the engine's read-set number while it holds this batch's reads WITH records
        self._pair_records_read_set = None             # ... and while it holds the pairs those reads were merged from (merge_reads only)

    def _dir(self, i: int) -> str:
        d = os.path.join(self.samples[i].tempdir, self.subdirs[i])
        os.makedirs(d, exist_ok=True)
        return d

    def _set_counts(self, counts) -> None:
        self.counts = np.asarray(counts, np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64)

    def _load_reads(self) -> None:
        """every sample's seq_file as one read set -- unless merge_reads / orient_reads left exactly these reads in the engine
        (SeqSample._reads_loaded_from for a batch)"""
        files = tuple(s.seq_file for s in self.samples)
        if self._resident is not None and self._resident == files:
            if getattr(self.engine, "read_set", None) == self._resident_read_set:
                return
            # something else loaded reads into the shared engine since: the resident reads are gone
            if not all(self._seq_written and os.path.exists(f) for f in files):
                raise EngineError(-1, "the engine no longer holds this batch's %s reads (another read set was loaded into it) and their "
                                      "files were not written: call %s() again"
                                      % ("merged" if self._resident_from == "merge_reads" else "oriented", self._resident_from))
        if any(f is None for f in files):
            raise EngineError(-1, "the batch holds paired samples that were never merged: call merge_reads() before deduplicate() / cluster_per_sample()")
        self._resident = None
        self.engine.keep_records(self.keep_records)
        self._set_counts(self.engine.load_reads_files(list(files)))
        self._records_read_set = self.engine.read_set if self.keep_records else None

    def _left_resident(self, files, written: bool, by: str) -> None:
        """the engine holds exactly the reads of `files` (one per sample) from here on"""
        self._resident = tuple(files)
        self._resident_read_set = getattr(self.engine, "read_set", None)
        self._seq_written = written
        self._resident_from = by
        self._records_read_set = self._resident_read_set if self.keep_records else None

    # -- f4 for all samples ------------------------------------------------------------------
    def orient_reads_by_profiles(self, hmmfile: str, threads: Union[int, str] = 1, write_seq_files: Optional[bool] = None) -> None:
        """`orient_reads` by the profiles of `hmmfile` (the file `_search` will get) instead of the universal database, every sample
        in one engine call (`orient_profiles_apply`).  A read the profiles cannot judge stays as it is, so no sample loses a read;
        every sample's strands (+1 / -1 / 0) are left in its `orient_strand`.  `orient_reads` comes here by itself with
        ITSXPRESS_ORIENT=profiles and every sample's `orient_hmmfile` set to one file."""
        self._orient(write_seq_files, hmmfile)

    def orient_reads(self, threads: Union[int, str] = 1, write_seq_files: Optional[bool] = None) -> None:
        """`orient_reads` of every sample (SeqSample.py:48-91; the plugin calls it per manifest row with trim_ccs, q2_itsxpress.py:284-285)
        in one engine call: every sample's `fastq` loaded as one read set, the orientation database loaded once, one `orient_apply`,
        which leaves the oriented reads of all samples on the device as the batch's read set -- `deduplicate` / `cluster_per_sample` go
        on from there without loading `oriented.fq`.  Every sample's `fastq`, `seq_file` and `r1` become `<its batch subdir>/oriented.fq`;
        the file -- byte for byte what the sample's own `orient_reads` writes -- is written unless write_seq_files is false (the default
        is to write it in both modes: a single-end sample's trimmed output is cut from it -- except in a batch with keep_records, which
        cuts it from the records on the device and so defaults to not writing the file).  `threads` is taken for the sake of
        SeqSample's signature and ignored, as in `merge_reads`: the engine sizes its own I/O pool, and the files are written by
        min(16, samples) writers at a time.
        With ITSXPRESS_ORIENT=profiles and every sample's `orient_hmmfile` set to one file: `orient_reads_by_profiles` of that file."""
        hmms = {_orient_hmmfile(s) for s in self.samples}
        if len(hmms) > 1:
            raise ValueError("a batch is oriented by one profile file: every sample's orient_hmmfile must name the same one")
        self._orient(write_seq_files, hmms.pop())

    def _orient(self, write_seq_files, hmm) -> None:
        try:
            from concurrent.futures import ThreadPoolExecutor
            from .definitions import ROOT_DIR
            from .trim import write_oriented_fastq
            for s in self.samples:
                if getattr(s, "fastq", None) is None:
                    raise ValueError("every sample needs its fastq path to orient its reads")
            eng = self.engine
            write = (not self.keep_records) if write_seq_files is None else bool(write_seq_files)
            inputs = [s.fastq for s in self.samples]
            outs = [os.path.join(self._dir(i), "oriented.fq") for i in range(len(self.samples))]
            self._resident = None
            eng.keep_records(self.keep_records)
            if hmm is not None and not isinstance(eng, Engine):
                eng.orient_profiles_apply()                 # (not streamed, not sharded: EngineError -5 naming the mode)
            before = np.asarray(eng.load_reads_files(inputs), np.int64)
            first = np.concatenate([[0], np.cumsum(before)]).astype(np.int64)
            if hmm is not None:
                eng.load_profiles(hmm)
                strand, _, _ = eng.orient_profiles_apply()
                for i, s in enumerate(self.samples):
                    s.orient_strand = strand[first[i]:first[i + 1]].copy()
                strand, kept = _keep_undecided(strand), before
            else:
                eng.orient_load_db(os.path.join(ROOT_DIR, "universal_orient_ref_clean.fasta.gz"))
                strand, _, _, kept = eng.orient_apply()
            if write:
                # the host writer, per sample, on the sample's own file and its slice of the strands (ctypes releases the GIL)
                def one(i):
                    return write_oriented_fastq(inputs[i], outs[i], strand[first[i]:first[i + 1]])
                with ThreadPoolExecutor(max_workers=max(1, min(16, len(outs)))) as pool:
                    written = list(pool.map(one, range(len(outs))))
                if [int(w) for w in written] != [int(k) for k in kept[:len(outs)]]:
                    raise EngineError(-4, "the oriented reads written and the oriented reads kept by the engine differ")
            for s, f in zip(self.samples, outs):
                s.fastq = f
                s.seq_file = f
                s.r1 = f
            self._set_counts(kept[:len(outs)])
            self._left_resident(outs, write, "orient_reads")
            logging.info("itsx_hip batch orient: %d samples, %d reads, %d kept", len(self.samples), int(before.sum()), int(self.counts.sum()))
        except EngineError as e:
            logging.exception("Could not orient reads with the HIP engine: %s", e)
            raise e
        except FileNotFoundError as f:
            logging.error("The HIP engine, the reads or the orientation reference were not found")
            raise f

    # -- f2 for all samples ------------------------------------------------------------------
    def merge_reads(self, threads: Union[int, str] = 1, stagger: bool = False, write_seq_files: Optional[bool] = None) -> None:
        """`_merge_reads` of every (paired) sample (SeqSample.py:266-365) in one engine call: one merge kernel over the pairs of all
        samples, the merged reads left on the device as the batch's read set.  Every sample's `seq_file` becomes
        `<its batch subdir>/seq.fq`; the file is written when write_seq_files is true (default: yes in file-compatible mode, no
        with ITSXPRESS_ARRAYS=1 or in a batch with keep_records), byte for byte what the sample's own `_merge_reads` writes.
        With parse = "device" R1 and R2 of every sample are parsed on the device and merged where the parser left them (with
        inflate = "device" from text that never left it); a batch the device declines is merged from the host's parse, the same."""
        try:
            for s in self.samples:
                if getattr(s, "r1", None) is None or getattr(s, "fastq2", None) is None:
                    raise ValueError("Both r1 and fastq2 paths must be defined to merge reads.")
            eng = self.engine
            write = (not _fast_from_env() and not self.keep_records) if write_seq_files is None else bool(write_seq_files)
            seq_files = [os.path.join(self._dir(i), "seq.fq") for i in range(len(self.samples))]
            self._resident = None
            eng.keep_records(self.keep_records)
            if self.keep_pair_records:
                eng.keep_pair_records(True)
            try:
                n, m = eng.merge_pairs_load_files([s.r1 for s in self.samples], [s.fastq2 for s in self.samples], seq_files if write else None,
                                                  maxdiffs=maxmismatches, maxee=2.0, allow_stagger=bool(stagger))
            finally:
                if self.keep_pair_records:
                    eng.keep_pair_records(False)           # (the flag is the engine's: a later merge of somebody else's keeps none)
            for s, f in zip(self.samples, seq_files):
                s.seq_file = f
            self.n_pairs = np.asarray(n, np.int64)
            self.n_joined = np.zeros(len(self.samples), np.int64)      # merge_join: the joined pairs per sample, reads of the batch like the merged
            if self.merge_join:
                joined = eng.merge_join_info()[0].astype(np.int64)
                ends = np.cumsum(self.n_pairs)
                csum = np.concatenate(([0], np.cumsum(joined)))
                self.n_joined = csum[ends] - csum[ends - self.n_pairs]
            m = np.asarray(m, np.int64) + self.n_joined
            self._set_counts(m)
            self._left_resident(seq_files, write, "merge_reads")
            self._pair_records_read_set = self._resident_read_set if self.keep_pair_records else None
            logging.info("itsx_hip batch merge: %d samples, %d pairs, %d merged, %d joined", len(self.samples), int(self.n_pairs.sum()),
                         int(self.counts.sum() - self.n_joined.sum()), int(self.n_joined.sum()))
        except EngineError as e:
            logging.exception("Could not perform read merging with the HIP engine: %s", e)
            raise e
        except FileNotFoundError as f:
            logging.error("The HIP engine or its input was not found")
            raise f

    # -- a1 for all samples ------------------------------------------------------------------
    def deduplicate(self, threads: Union[int, str] = 1) -> None:
        """`vsearch --fastx_uniques ... --strand both` of every sample (SeqSample.py:93-131), one device pass."""
        try:
            eng = self.engine
            self._load_reads()
            n = eng.derep(strand_both=True, minseqlength=1)      # SeqSample.deduplicate's value (SeqSample.py:96 passes no --minseqlength; the mirror uses 1): a batch and a solo run must agree on short reads
            for i, s in enumerate(self.samples):
                d = self._dir(i)
                s.uc_file = os.path.join(d, "uc.txt")
                s.rep_file = os.path.join(d, "rep.fa")
                eng.select_sample(i)
                eng.write_uc(s.uc_file)
                eng.write_rep_fasta(s.rep_file)
            eng.select_sample(-1)
            logging.info("itsx_hip batch derep: %d samples, %d reads -> %d unique sequences", len(self.samples), eng.n_reads, n)
        except EngineError as e:
            logging.exception("Could not perform dereplication with the HIP engine: %s", e)
            raise e
        except FileNotFoundError as f:
            logging.error("The HIP engine or its input was not found")
            raise f

    def cluster(self, threads: Union[int, str], cluster_id: float = 0.995) -> None:
        """cluster_id == 1.0 is dereplication (main.py:534-537).  Greedy clustering below 1.0 is not run by this
        method: `cluster_per_sample` clusters every sample of the batch as `sobj.cluster(...)` would."""
        if float(cluster_id) == 1.0:
            return self.deduplicate(threads=threads)
        raise EngineError(-5, "cluster_id < 1 is not batched across samples; call SeqSample.cluster per sample")

    def cluster_per_sample(self, threads: Union[int, str], cluster_id: float = 0.995) -> None:
        """`SeqSample.cluster(threads, cluster_id)` of every sample (SeqSample.py:133-176; the QIIME 2 plugin's per-sample
        loop at cluster_id < 1, q2_itsxpress.py:287-290) in one engine call: each sample's uc.txt / rep.fa are
        byte-identical to those of its own run (itsx_cluster_samples)."""
        try:
            eng = self.engine
            self._load_reads()
            n = eng.cluster_samples(float(cluster_id), strand_both=True)
            if float(cluster_id) < 1.0 and _uc_cigar_wanted(self, eng, False):      # every sample's members in one pass; the writer picks the sample's
                eng.align_clusters()
            for i, s in enumerate(self.samples):
                d = self._dir(i)
                s.uc_file = os.path.join(d, "uc.txt")
                s.rep_file = os.path.join(d, "rep.fa")
                eng.select_sample(i)
                eng.write_uc(s.uc_file)
                eng.write_rep_fasta(s.rep_file)
            eng.select_sample(-1)
            logging.info("itsx_hip batch cluster at %g: %d samples, %d reads -> %d clusters", float(cluster_id), len(self.samples), eng.n_reads, n)
        except EngineError as e:
            logging.exception("Could not perform clustering with the HIP engine: %s", e)
            raise e
        except FileNotFoundError as f:
            logging.error("The HIP engine or its input was not found")
            raise f

    # -- a4 for all samples ------------------------------------------------------------------
    def _search(self, hmmfile: str, threads: Union[int, str] = 1) -> None:
        """`hmmsearch --domtblout ... -T 10 --F1 1e-6 --F2 1e-6 --F3 1e-6` of every sample's rep.fa (SeqSample.py:178-225)."""
        try:
            eng = self.engine
            if self.counts is None:
                raise EngineError(-1, "deduplicate() the batch before _search()")
            eng.load_profiles(path=hmmfile)
            # ITSXPRESS_DOMTBL=winners (SeqSample._search): the lazy search, every sample's domtbl.txt = the rows its ItsPosition ends up with
            winners = _winners_from_env()
            if winners:
                eng.set_rows_mode("lazy")
            try:
                eng.search(T=10.0, F1=1e-6, F2=1e-6, F3=1e-6)
                eng.finalize(domE=10.0)
                eng.set_kept_rows(winners)
                if _domtbl_ali_wanted(self, eng, False):      # every sample's reported rows in one pass; the writer picks the sample's
                    eng.align_domains()
                for i, s in enumerate(self.samples):
                    s.dom_file = os.path.join(self._dir(i), "domtbl.txt")
                    eng.select_sample(i)
                    eng.write_domtbl(s.dom_file)
                eng.select_sample(-1)
            finally:
                if winners:
                    eng.set_kept_rows(False)
                    eng.set_rows_mode(None)
        except EngineError as e:
            logging.exception("Could not perform ITS identification with the HIP engine: %s", e)
            raise e
        except FileNotFoundError as f:
            logging.error("The HIP engine or the HMM file was not found")
            raise f

    # -- array fast path ----------------------------------------------------------------------
    def trim_coordinates(self, region: str) -> List[tuple]:
        """Per sample: (start, stop, tlen, in_ddict) arrays over that sample's reads in file order; -1 = None."""
        left, right = _REGION_PREFIX[region]
        a = self.engine.trim_coords(left, right)
        out = []
        for i in range(len(self.samples)):
            lo, hi = int(self.first[i]), int(self.first[i] + self.counts[i])
            out.append(tuple(x[lo:hi] for x in a))
        return out

    # -- the consumers of the coordinates, per sample -------------------------------------------
    # Where write_trimmed / write_paired_trimmed make the bytes of gzip output when they cut the files from records on the device:
    # the engine's own setting (Engine.deflate, "host" by default), under the batch's name.  The host loops have no device text:
    # with "device" they still write with the host's deflate and say so.
    @property
    def deflate(self) -> str:
        return getattr(self.engine, "deflate", "host")

    @deflate.setter
    def deflate(self, where: str):
        self.engine.deflate = where

    # Whether _search scores each distinct representative once for all the samples it occurs in (score classes): the engine's own
    # setting (Engine.share_samples, off by default), under the batch's name.  Every sample's domtbl.txt and coordinates are those of a
    # batch without it.  A setting like deflate / inflate / parse, not a constructor keyword: the constructor's signature stays
    @property
    def share_samples(self) -> bool:
        return self.engine.share_samples

    @share_samples.setter
    def share_samples(self, on: bool):
        self.engine.share_samples = on

    # The same for the lazy / compact searches (ITSXPRESS_DOMTBL=winners, set_rows_mode): the engine's own setting
    # (Engine.share_samples_lazy, off by default), under the batch's name.  A property, not a constructor keyword
    @property
    def share_samples_lazy(self) -> bool:
        return self.engine.share_samples_lazy

    @share_samples_lazy.setter
    def share_samples_lazy(self, on: bool):
        self.engine.share_samples_lazy = on

    # Where the engine's whole-file loaders inflate gzip input: the engine's own setting (Engine.inflate), under the batch's name
    @property
    def inflate(self) -> str:
        return getattr(self.engine, "inflate", "host")

    @inflate.setter
    def inflate(self, where: str):
        self.engine.inflate = where

    # Where the engine's whole-file loaders and its paired merge loaders (merge_reads) parse FASTQ text: the engine's own setting
    # (Engine.parse), under the batch's name
    @property
    def parse(self) -> str:
        return getattr(self.engine, "parse", "host")

    @parse.setter
    def parse(self, where: str):
        self.engine.parse = where

    # Whether merge_reads keeps the pairs whose mates do not overlap as joined reads: the engine's own setting (Engine.merge_join),
    # under the batch's name.  `counts` then holds merged and joined reads, `n_joined` the joined ones per sample.
    @property
    def merge_join(self) -> bool:
        return bool(getattr(self.engine, "merge_join", False))

    @merge_join.setter
    def merge_join(self, on: bool):
        self.engine.merge_join = on

    def _device_deflate_falls_back(self, who, gzipped, zstd_file):
        if self.deflate == "device":
            from .engine import _batch_compression
            _batch_compression(gzipped, zstd_file, "device", who)           # the same ValueError as on the device path
            logging.info("%s: no records on the device to cut the files from, so the host writes and deflates them (deflate = \"device\" has no device text here)", who)

    def _sample_range(self, i: int):
        return int(self.first[i]), int(self.first[i] + self.counts[i])

    # -- the feature table of the trimmed regions ------------------------------------------------
    def feature_table(self, region: str, min_len: int = 1, ids: str = "sha1"):
        """The batch's trimmed `region` dereplicated over all samples (Engine.trimmed_table with the region's profile prefixes): the
        table `vsearch --derep_fulllength --sizeout --relabel_sha1` makes of the files write_trimmed writes, without writing them.
        Returns the engine's FeatureTable with `labels` added: ids="sha1" names a feature by the SHA-1 of its sequence, ids="first" by
        the id of its first read.  Needs the finalized search (_search); one GPU, whole-file read sets, forward strand, no trim_ccs
        stitching."""
        if ids not in ("sha1", "first"):
            raise ValueError('ids is "sha1" or "first"')
        t = self.engine.trimmed_table(region_prefixes=_REGION_PREFIX[region], min_len=min_len)
        if ids == "sha1":
            import hashlib
            t.labels = [hashlib.sha1(s.encode()).hexdigest() for s in t.sequences]
        else:
            blob, offs = self.engine.read_names_raw()
            t.labels = [blob[int(offs[r]):int(offs[r + 1])].decode().split(None, 1)[0] if offs[r + 1] > offs[r] else "r%09d" % r
                        for r in t.first_read]
        return t

    def write_feature_table(self, fasta: Optional[str], tsv: Optional[str], region: str, min_len: int = 1, ids: str = "sha1",
                            sample_names: Optional[Sequence[str]] = None):
        """feature_table(region) written as two files (either may be None): `fasta` holds `>label;size=total` and the sequence per
        feature, `tsv` a `#feature` header line with the sample names and one line of counts per feature, both in table order.
        sample_names default to the basename of each sample's input file.  Returns the table."""
        from . import _lib
        import ctypes as C
        t = self.feature_table(region, min_len=min_len, ids=ids)
        if sample_names is None:
            sample_names = [os.path.basename(getattr(s, "fastq", None) or getattr(s, "r1", None) or s.seq_file) for s in self.samples]
        sample_names = [str(x) for x in sample_names]
        if len(sample_names) != t.n_samples:
            raise ValueError("write_feature_table: %d sample names for %d sample(s)" % (len(sample_names), t.n_samples))

        def blob_of(names):
            enc = [x.encode() for x in names]
            return b"".join(enc), np.concatenate([[0], np.cumsum([len(x) for x in enc])]).astype(np.int64)
        lab, lab_off = blob_of(t.labels)
        sn, sn_off = blob_of(sample_names)
        pad = lambda x: x.ctypes.data if x.size else None
        L = _lib.lib()
        rc = L.itsx_write_feature_files(None if fasta is None else os.fsencode(fasta), None if tsv is None else os.fsencode(tsv),
                                        t.n_features, t.n_samples, pad(t.totals), pad(t.first_read), t.row_off.ctypes.data,
                                        pad(t.entry_sample), pad(t.entry_count), C.c_char_p(t.bases), t.seq_off.ctypes.data,
                                        C.c_char_p(lab), lab_off.ctypes.data, None, None, C.c_char_p(sn), sn_off.ctypes.data)
        if rc != 0:
            raise EngineError(rc, L.itsx_writers_last_error().decode())
        return t

    # -- the feature table denoised into ZOTUs ---------------------------------------------------
    def denoise_features(self, region: str, alpha: float = 2.0, minsize: int = 8, min_len: int = 1, ids: str = "sha1"):
        """feature_table(region) denoised by the UNOISE rule (Engine.denoise_table): what `usearch -unoise3` / `vsearch --cluster_unoise`
        make of the dereplicated trimmed regions, as the project states the rule (parity with either is not pinned; no chimera step;
        unassigned reads are dropped, not mapped back).  Returns the engine's DenoisedTable with `sequences` and `labels` of the
        centroids added (ids as in feature_table) and `features`, the table it was made of."""
        ft = self.feature_table(region, min_len=min_len, ids=ids)
        t = self.engine.denoise_table(alpha=alpha, minsize=minsize)
        t.features = ft
        t.sequences = [ft.sequences[int(f)] for f in t.zotu_feature]
        t.labels = [ft.labels[int(f)] for f in t.zotu_feature]
        return t

    def write_denoised_table(self, fasta: Optional[str], tsv: Optional[str], region: str, alpha: float = 2.0, minsize: int = 8,
                             min_len: int = 1, ids: str = "sha1", sample_names: Optional[Sequence[str]] = None):
        """denoise_features(region) written as the two files write_feature_table writes, one record per ZOTU: `>label;size=total` with
        the ZOTU's total and the centroid's sequence, and the TSV of the ZOTUs' counts.  Returns the table."""
        t = self.denoise_features(region, alpha=alpha, minsize=minsize, min_len=min_len, ids=ids)
        if sample_names is None:
            sample_names = [os.path.basename(getattr(s, "fastq", None) or getattr(s, "r1", None) or s.seq_file) for s in self.samples]
        write_denoised_files(fasta, tsv, t.n_samples, t.totals, t.zotu_feature, t.row_off, t.entry_sample, t.entry_count, t.sequences, t.labels,
                             sample_names)
        return t

    def write_paired_trimmed(self, outfiles1: Sequence[str], outfiles2: Sequence[str], region: str, gzipped: bool = False,
                             zstd_file: bool = False, trim_ccs: bool = False) -> List[int]:
        """`Dedup.create_paired_trimmed_seqs` of every sample from the batch's arrays: the ORIGINAL r1 / fastq2 records of sample i,
        sliced with its merged reads' coordinates, into outfiles1[i] / outfiles2[i].  Returns the pairs written per sample.
        The host writer reads and parses every sample's two files again -- unless the batch keeps the pair records
        (keep_records="pairs") and the engine still holds its read set: then every sample's two files are cut from the records on the
        device in one engine call (itsx_write_trimmed_paired_samples), the same bytes.  (Inputs with lower-case bases keep no pair records
        -- the merge reads them in upper case -- and take the host loop.)
        With self.deflate = "device" the engine call makes the gzip bytes (gzipped=True) on the device."""
        from .trim import write_trimmed_paired
        left, right = _REGION_PREFIX[region]
        if self.keep_pair_records and self._pair_records_read_set is not None and getattr(self.engine, "read_set", None) == self._pair_records_read_set:
            try:
                return self.engine.write_trimmed_paired_samples(list(outfiles1), list(outfiles2), region_prefixes=(left, right), gzipped=gzipped,
                                                                zstd_file=zstd_file, trim_ccs=trim_ccs)
            except EngineError as e:
                # the merge kept no pair records after all: the inputs hold lower-case bases, which the merge's upper-case upload cannot
                # give back.  The host writer copies the input's bytes.
                # (The C ABI has no query for it; the engine's message for exactly this case names the switch -- engine.hip says so there.)
                if e.code != -1 or "itsx_keep_pair_records" not in str(e):
                    raise
                self._pair_records_read_set = None
        self._device_deflate_falls_back("write_paired_trimmed", gzipped, zstd_file)
        start, stop, tlen, _ = self.engine.trim_coords(left, right)
        blob, offs = self.engine.read_names_raw()
        out = []
        for i, s in enumerate(self.samples):
            if getattr(s, "r1", None) is None or getattr(s, "fastq2", None) is None:
                raise ValueError("Both fastq and fastq2 paths must be defined to create paired trimmed sequences.")
            lo, hi = self._sample_range(i)
            names = (blob[int(offs[lo]):int(offs[hi])], offs[lo:hi + 1] - offs[lo])
            out.append(write_trimmed_paired(s.r1, s.fastq2, outfiles1[i], outfiles2[i], names, start[lo:hi], stop[lo:hi], tlen[lo:hi],
                                            gzipped=gzipped, trim_ccs=trim_ccs, zstd_file=zstd_file))
        return out

    def write_trimmed(self, outfiles: Sequence[str], region: str, gzipped: bool = False, zstd_file: bool = False,
                      trim_ccs: bool = False) -> List[tuple]:
        """`Dedup.create_trimmed_seqs` of every sample from the batch's arrays: record k of sample i's seq_file trimmed to its
        coordinates, into outfiles[i].  A paired sample's seq_file is its merged reads: merge_reads must have written it -- unless the
        batch keeps records (keep_records=True) and the engine still holds its read set: then every sample's output is cut from the
        records on the device in one engine call (itsx_write_trimmed_samples), the same bytes.
        With self.deflate = "device" that call makes the gzip bytes (gzipped=True) on the device: the same records in other bytes."""
        from .trim import write_trimmed_fastq
        left, right = _REGION_PREFIX[region]
        if self.keep_records and self._records_read_set is not None and getattr(self.engine, "read_set", None) == self._records_read_set:
            return self.engine.write_trimmed_samples(list(outfiles), region_prefixes=(left, right), gzipped=gzipped, zstd_file=zstd_file,
                                                     trim_ccs=trim_ccs)
        self._device_deflate_falls_back("write_trimmed", gzipped, zstd_file)
        for s in self.samples:
            if self._resident is not None and s.seq_file in self._resident and not (self._seq_written and os.path.exists(s.seq_file)):
                raise EngineError(-1, "write_trimmed: the %s reads of this batch were never written (%s); call %s(write_seq_files=True)"
                                      % ("merged" if self._resident_from == "merge_reads" else "oriented", s.seq_file, self._resident_from))
        start, stop, _, _ = self.engine.trim_coords(left, right)
        out = []
        for i, s in enumerate(self.samples):
            lo, hi = self._sample_range(i)
            out.append(write_trimmed_fastq(s.seq_file, outfiles[i], start[lo:hi], stop[lo:hi], gzipped=gzipped, trim_ccs=trim_ccs, zstd_file=zstd_file))
        return out
