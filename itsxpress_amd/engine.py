"""Engine: a thin object wrapper over the C ABI (one context = one GPU).

Nothing here computes: every method forwards to libitsx_hip.so and copies results into numpy
arrays the caller owns.  See include/itsx_hip.h for the reference interface each call replaces.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import ALIGNMENT_DTYPE, DOMAIN_DTYPE, LAZY_PAIR_DTYPE, STATS_DTYPE_ALL, TRACE_DTYPE, EngineError


def _device_from_env():
    for k in ("ITSXPRESS_GPU", "LOCAL_RANK"):
        v = os.environ.get(k)
        if v is not None and v.strip() != "":
            return int(v)
    return 0


class _DevArray:
    """a raw device pointer dressed up for torch.as_tensor (zero-copy): the engine keeps owning the memory"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3,
                                         "strides": None}


def _devtensor(ptr, shape, typestr, device):
    import torch
    dt = {"<i8": torch.int64, "<i4": torch.int32, "|i1": torch.int8}[typestr]
    if not ptr or int(np.prod(shape)) == 0:
        return torch.empty(tuple(shape), dtype=dt, device=device)
    return torch.as_tensor(_DevArray(ptr, shape, typestr), device=device)


def _batch_compression(gzipped, zstd_file, deflate, who):
    """The batch writers' compression kind: the reference's two flags, and 3 (gzip members made on the device) where deflate is
    "device" -- which goes with gzip output only."""
    from .trim import _compression
    if deflate == "device":
        if zstd_file or not gzipped:
            raise ValueError('%s: deflate = "device" makes gzip output: it goes with gzipped=True and without zstd_file' % who)
        return 3
    return _compression(gzipped, zstd_file)


class FeatureTable:
    """What Engine.trimmed_table returns: the distinct trimmed sequences of a read set by its samples, in table order.
    sequences (list[str], made on first use from bases / seq_off), lengths, totals, first_read: per feature; the cells as CSR rows --
    feature f's are [row_off[f], row_off[f + 1]) of entry_sample / entry_count, samples ascending; feature_of_read: per read, -1 = not
    counted; n_counted; ms_kernels: the device time of the call."""
    n_samples = 1
    n_counted = 0
    ms_kernels = 0.0
    _seqs = None

    @property
    def n_features(self):
        return int(self.totals.shape[0])

    @property
    def sequences(self):
        if self._seqs is None:
            text = self.bases.decode("ascii")
            self._seqs = [text[int(self.seq_off[f]):int(self.seq_off[f + 1])] for f in range(self.n_features)]
        return self._seqs

    def dense(self):
        """the table as an [n_features, n_samples] int64 array"""
        out = np.zeros((self.n_features, self.n_samples), np.int64)
        rows = np.repeat(np.arange(self.n_features), np.diff(self.row_off))
        out[rows, self.entry_sample] = self.entry_count
        return out


class DenoisedTable:
    """What Engine.denoise_table returns: the feature table denoised into ZOTUs by the UNOISE rule, ZOTUs in the order of their
    centroids (table order).  zotu_feature (the centroid's feature), totals: per ZOTU; the cells as CSR rows -- ZOTU z's are
    [row_off[z], row_off[z + 1]) of entry_sample / entry_count, samples ascending; zotu_of_feature (-1: unassigned) and dist_of_feature
    (0: a centroid, -1: unassigned): per feature; n_dropped_reads: the unassigned features' reads; n_pairs: the (feature, centroid) pairs
    that reached the distance kernel; n_levels, n_skipped_skew, n_skipped_length: the schedule's levels and the pairs left out before
    any distance work; n_columns: the target symbols the kernel stepped; max_skew: the skew table used; ms_kernels: the device time of the call."""
    n_samples = 1
    n_dropped_reads = 0
    n_pairs = 0
    ms_kernels = 0.0

    @property
    def n_zotus(self):
        return int(self.totals.shape[0])

    def dense(self):
        """the denoised table as an [n_zotus, n_samples] int64 array"""
        out = np.zeros((self.n_zotus, self.n_samples), np.int64)
        rows = np.repeat(np.arange(self.n_zotus), np.diff(self.row_off))
        out[rows, self.entry_sample] = self.entry_count
        return out


def unoise_skews(alpha=2.0, max_total=None, max_diffs=None):
    """UNOISE's skew limits as the table itsx_denoise_table takes: max_skew[d - 1] = 2.0 ** -(alpha * d + 1) for d = 1, 2, ...  The
    table stops at the smaller of max_diffs (default 31) and the last d with max_skew * max_total >= 1 (max_total: the largest feature
    total; None: no such stop): no later d can accept anything, since every feature holds at least one read."""
    alpha = float(alpha)
    if not alpha > 0:
        raise ValueError("unoise_skews: alpha must be above 0")
    top = 31 if max_diffs is None else int(max_diffs)
    if not 0 <= top <= 31:
        raise ValueError("unoise_skews: max_diffs is 0 .. 31")
    out = []
    for d in range(1, top + 1):
        v = 2.0 ** -(alpha * d + 1)
        if v <= 0.0 or (max_total is not None and not v * float(max_total) >= 1.0):
            break
        out.append(v)
    return np.asarray(out, np.float64)


class Engine:
    def __init__(self, device=None):
        self.L = _lib.lib()
        if device is None:
            device = _device_from_env()
        self.h = self.L.itsx_create(int(device), 0)
        if not self.h:
            msg = self.L.itsx_last_error(None).decode()
            raise EngineError(-4, msg)
        self.device = int(device)
        self.read_set = 0            # bumped whenever the context is given (or loses) a read set: see n_reads
        self.n_reads = 0
        self.n_unique = 0
        self.n_profiles = 0
        self.n_samples = 1
        self.rows_mode = -1
        self.n_joined = 0            # the joined pairs of the last merge call (merge_join; 0 with it off)

    # Where the batch writers (write_trimmed_samples, write_trimmed_paired_samples) make the bytes of gzip output: "host" (the
    # default: the text comes back and the host's deflate writes it, byte for byte what it always wrote) or "device" (the gzip
    # members are made on the device, csrc/k_deflate.hip, and only they come back: the same records in other bytes, at a fast
    # level's ratio).  Stays until set again; "device" asks for gzipped=True without zstd_file and is a ValueError otherwise.
    @property
    def deflate(self):
        return getattr(self, "_deflate", "host")

    @deflate.setter
    def deflate(self, where):
        if where not in ("host", "device"):
            raise ValueError('Engine.deflate is "host" or "device", not %r' % (where,))
        self._deflate = where

    # Where the context's whole-file loaders (load_reads_file, load_reads_files, the merge loaders) inflate a gzip input: "host" (the
    # default: libdeflate / zlib / the block-parallel inflater on the I/O threads, as ever) or "device" (a file made of independent
    # gzip members -- this package's writers', bgzip's -- is inflated by csrc/k_inflate.hip first; a file the device declines goes the
    # host's way).  The same text either way.  Stays until set again.
    @property
    def inflate(self):
        return getattr(self, "_inflate", "host")

    @inflate.setter
    def inflate(self, where):
        if where not in ("host", "device"):
            raise ValueError('Engine.inflate is "host" or "device", not %r' % (where,))
        if getattr(self, "h", None):
            self._chk(self.L.itsx_set_device_inflate(self.h, int(where == "device")))
        self._inflate = where

    # Where the context's whole-file loaders (load_reads_file, load_reads_text, load_reads_files) and its paired merge loaders
    # (merge_pairs_load, merge_pairs_load_text, merge_pairs_load_files) parse FASTQ text: "host" (the default: the I/O threads, as ever)
    # or "device" (csrc/k_fastq.hip: the text is parsed where the device inflate left it, or uploaded once; only offsets and title
    # lines come back, and the bases stay on the device until rep.fa asks for them; a text the device declines -- FASTA, blank lines, a
    # malformed record -- makes the call start over on the host).  The merge loaders parse R1 and R2 into a plane set each, upper-case
    # and check them there, and the merge kernel and keep_pair_records take the planes where they lie; unequal record counts, a quality
    # outside 33..126 and a pair above 12000 bases also start over on the host, whose errors they then are.  merge_pairs_files and the
    # orient, shard and streamed loaders parse on the host.  The same reads either way.  A file the device both inflated and parsed
    # never enters the host's text cache: a writer that wants its text later reads the file again.
    @property
    def parse(self):
        return getattr(self, "_parse", "host")

    @parse.setter
    def parse(self, where):
        if where not in ("host", "device"):
            raise ValueError('Engine.parse is "host" or "device", not %r' % (where,))
        if getattr(self, "h", None):
            self._chk(self.L.itsx_set_device_parse(self.h, int(where == "device")))
        self._parse = where

    # Whether a search of a sample batch (S > 1, full rows mode) scores each distinct representative ONCE for all the samples it occurs
    # in (itsx_set_sample_sharing): the uniques of all samples whose representatives are the same string in the same orientation form a
    # score class, one holder per class goes through the HMM stages, and every member gets the holder's rows -- the rows, counters,
    # coordinates and domtbl.txt of a search without it, bit for bit.  False (the default) or True; no effect on one sample, in the
    # compact / lazy rows modes (share_samples_lazy, below, is theirs) and after set_active_uniques (sample_sharing_info() then reports no classes).  Stays until set again.
    @property
    def share_samples(self):
        return getattr(self, "_share_samples", False)

    @share_samples.setter
    def share_samples(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("Engine.share_samples is False or True, not %r" % (on,))
        if getattr(self, "h", None):
            self._chk(self.L.itsx_set_sample_sharing(self.h, int(bool(on))))
        self._share_samples = bool(on)

    # The same for the compact and lazy rows modes (itsx_set_sample_sharing_lazy), a setting of its own: share_samples governs the full
    # rows mode alone, this one the searches behind set_rows_mode("lazy") / ("compact") and ITSXPRESS_DOMTBL=winners.  One holder per
    # score class goes through the MSV filter, pass A, the lazy rounds and the domain pipeline; every evaluated, reported pair counts
    # for each member's sample, the holders past the filter bound every sample's domZ from above, and the kept rows are copied to the
    # members before finalize().  Coordinates, uc.txt / rep.fa and the kept rows' domtbl.txt are those of a search without it; the lazy
    # counters are valid bounds (exact after a completion), the compact ones exact.  False (the default) or True; no effect on one
    # sample, in the full rows mode and after set_active_uniques.  Stays until set again.
    @property
    def share_samples_lazy(self):
        return getattr(self, "_share_samples_lazy", False)

    @share_samples_lazy.setter
    def share_samples_lazy(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("Engine.share_samples_lazy is False or True, not %r" % (on,))
        if getattr(self, "h", None):
            self._chk(self.L.itsx_set_sample_sharing_lazy(self.h, int(bool(on))))
        self._share_samples_lazy = bool(on)

    # Whether the merge entry points keep a pair whose mates do not overlap (itsx_set_merge_join).  ITS1 / ITS2 run from about 100 to
    # over 600 bases, so a 2x250 or 2x300 run cannot merge the long ones, and a pair the merge rejects is gone from seq.fq, the read
    # set and both trimmed outputs.  While on, a pair rejected with reason 1, 3 or 5 (no shared 5-mers, score < 16, overlap < 10) is
    # joined: R1 + "NNNNNNNN" + revcomp(R2), qualities Q1 + "IIIIIIII" + reversed Q2 (vsearch --fastq_join's padding; parity unpinned,
    # like the merge's), with no expected-error filter.  merge_pairs_files, merge_pairs_load, merge_pairs_load_text and
    # merge_pairs_load_files honour it; the counts they return stay those of the MERGED pairs, n_reads and merge_pair_index cover both
    # kinds, merge_join_info() tells them apart.  The paired trimmed output is what the mode is for: each mate is cut at its own anchor.
    # A single merged output then holds joined reads with the N gap inside.  False (the default) or True; stays until set again.
    @property
    def merge_join(self):
        return getattr(self, "_merge_join", False)

    @merge_join.setter
    def merge_join(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("Engine.merge_join is False or True, not %r" % (on,))
        if getattr(self, "h", None):
            self._chk(self.L.itsx_set_merge_join(self.h, int(bool(on))))
        self._merge_join = bool(on)

    def merge_join_info(self):
        """After a merge (merge_pairs_load / _load_text / _load_files: the pairs merge_pair_index speaks of; merge_pairs_files: that
        call's pairs): (joined int8[n_pairs], n_joined) -- 1 where the pair's read is a joined one.  All 0 with merge_join off."""
        n = int(getattr(self, "_n_pairs_join", getattr(self, "_n_pairs", 0)))
        j = np.zeros(max(1, n), np.int8)
        c = C.c_int64(0)
        self._chk(self.L.itsx_merge_join_info(self.h, j.ctypes.data, n, C.byref(c)))
        return j[:n], int(c.value)

    def _n_joined(self, n_pairs):
        """the joined pairs of the merge call just made (0 without a call to the engine when merge_join is off)"""
        self._n_pairs_join = int(n_pairs)
        self.n_joined = 0
        if self.merge_join:
            c = C.c_int64(0)
            self._chk(self.L.itsx_merge_join_info(self.h, None, int(n_pairs), C.byref(c)))
            self.n_joined = int(c.value)
        return self.n_joined

    def sample_sharing_info(self):
        """What the last search() shared across samples: dict(n_classes, n_uniques_shared, n_rows_expanded, ms_classes, ms_expand) --
        the score classes it built, the uniques it did not score because their class's holder was, the rows copied to them, and the
        time of the two steps (event spans: their kernels and the host synchronisations between them).  All zero when share_samples was
        off or does not apply; where it applies and nothing is common, n_classes == n_unique and nothing is shared or copied."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.itsx_sample_sharing_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        x, y = C.c_float(0), C.c_float(0)
        self._chk(self.L.itsx_sample_sharing_times(self.h, C.byref(x), C.byref(y)))
        return dict(n_classes=int(a.value), n_uniques_shared=int(b.value), n_rows_expanded=int(c.value), ms_classes=float(x.value), ms_expand=float(y.value))

    def debug_sample_classes(self):
        """test hook: class_of[n_unique] of the last sharing search, from the device (classes numbered by their first member)"""
        out = np.zeros(max(int(self.n_unique), 1), np.int32)
        self._chk(self.L.itsx_debug_sample_classes(self.h, out.ctypes.data, int(self.n_unique)))
        return out[:int(self.n_unique)]

    # Every call that changes the context's read set records the new count here, so the setter is where the read set's serial number
    # advances: a caller that left reads resident (SampleBatch.merge_reads) keeps the number and can tell later whether the
    # engine -- which may be shared -- still holds them
    @property
    def n_reads(self):
        return self._n_reads

    @n_reads.setter
    def n_reads(self, v):
        self._n_reads = v
        self.read_set += 1

    def close(self):
        if getattr(self, "h", None):
            self.L.itsx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise EngineError(rc, self.L.itsx_last_error(self.h).decode())

    # ---- profiles
    def load_profiles(self, path=None, text=None):
        n = C.c_int(0)
        if path is not None:
            if not os.path.exists(path):
                raise FileNotFoundError(path)
            self._chk(self.L.itsx_load_profiles_file(self.h, os.fsencode(path), C.byref(n)))
        else:
            if isinstance(text, str):
                text = text.encode()
            self._chk(self.L.itsx_load_profiles_mem(self.h, text, len(text), C.byref(n)))
        self.n_profiles = n.value
        return n.value

    def profile_names(self):
        buf = C.create_string_buffer(256)
        out = []
        for i in range(self.n_profiles):
            self._chk(self.L.itsx_profile_name(self.h, i, buf, 256))
            out.append(buf.value.decode())
        return out

    def profile_tables(self, i):
        p = np.zeros(6, np.int32)
        self._chk(self.L.itsx_profile_tables(self.h, i, None, None, None, p.ctypes.data))
        M, Q = int(p[0]), int(p[1])
        rbv = np.zeros((18, M + 1), np.uint8)
        rfv = np.zeros((18, Q, 4), np.float32)
        tfv = np.zeros((8 * Q, 4), np.float32)
        self._chk(self.L.itsx_profile_tables(self.h, i, rbv.ctypes.data, rfv.ctypes.data, tfv.ctypes.data, p.ctypes.data))
        return dict(M=M, Q=Q, base=int(p[2]), bias=int(p[3]), tbm=int(p[4]), tec=int(p[5]), rbv=rbv, rfv=rfv, tfv=tfv)

    # ---- reads
    def set_reads(self, seqs, names=None):
        """seqs: list[str] (or list[bytes]); names: optional list[str]."""
        n = len(seqs)
        lens = np.fromiter((len(s) for s in seqs), np.int64, n)
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        blob = ("".join(seqs)).encode() if (n and isinstance(seqs[0], str)) else b"".join(seqs)
        return self.set_reads_buffer(blob, offs, names)

    def set_reads_buffer(self, blob, offsets, names=None):
        """blob: bytes-like of ASCII bases (bytes, bytearray, numpy uint8 array); the engine keeps a pointer into it
        (itsx_set_reads_view), and this object keeps the buffer alive until the next read set."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        nb = no = None
        if names is not None:
            nl = np.fromiter((len(s) for s in names), np.int64, n)
            no = np.zeros(n + 1, np.int64)
            np.cumsum(nl, out=no[1:])
            nb = "".join(names).encode()
        if isinstance(blob, np.ndarray):
            blob = np.ascontiguousarray(blob, np.uint8)
            cptr = C.c_void_p(blob.ctypes.data)
        else:
            if not isinstance(blob, bytes):
                blob = bytes(blob)
            cptr = C.cast(C.c_char_p(blob), C.c_void_p)
        self._keep = (blob, offsets, nb, no)
        self._chk(self.L.itsx_set_reads_view(self.h, cptr, offsets.ctypes.data, n,
                                        C.cast(C.c_char_p(nb), C.c_void_p) if nb is not None else None,
                                        no.ctypes.data if no is not None else None))
        self.n_reads = n
        self.n_samples = 1
        return n

    def set_reads_device(self, dev_ptr, offsets, keep=None):
        """ASCII bases already in device memory on this engine's GPU (dev_ptr: integer address); offsets int64[n+1] on the
        host.  `keep`: any object that owns the device buffer (kept referenced until the next read set)."""
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        self._keep = (keep, offsets)
        self._chk(self.L.itsx_set_reads_device(self.h, C.c_void_p(int(dev_ptr)), offsets.ctypes.data, n, None, None))
        self.n_reads = n
        self.n_samples = 1
        return n

    def load_reads_file(self, path):
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        n = C.c_int64(0)
        self._chk(self.L.itsx_load_reads_file(self.h, os.fsencode(path), C.byref(n)))
        self.n_reads = n.value
        self.n_samples = 1
        return n.value

    def load_reads_text(self, ptr, nbytes):
        """the records of FASTA / FASTQ text already in memory (address + length: a slice of itsxpress_amd.stream's text stream)"""
        n = C.c_int64(0)
        self._chk(self.L.itsx_load_reads_text(self.h, C.c_void_p(ptr), int(nbytes), C.byref(n)))
        self.n_reads = n.value
        self.n_samples = 1
        return n.value

    # ---- f4: per-sample batching (many samples, one pass of every kernel, per-sample results)
    def load_reads_files(self, paths):
        """One sequence file per sample, in order: sample index = position in `paths`.
        Returns the read count of each file (reads of sample s are the s-th contiguous block)."""
        for p in paths:
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        counts = np.zeros(max(1, len(paths)), np.int64)
        self._chk(self.L.itsx_load_reads_files(self.h, arr, len(paths), counts.ctypes.data))
        self.n_reads = int(counts[:len(paths)].sum())
        self.n_samples = max(1, self.L.itsx_num_samples(self.h))
        return counts[:len(paths)]

    def set_samples(self, sample_of_read, n_samples):
        """sample_of_read int32[n_reads] in [0, n_samples); None returns to one sample."""
        if sample_of_read is None:
            self._chk(self.L.itsx_set_samples(self.h, None, 1))
        else:
            a = np.ascontiguousarray(sample_of_read, np.int32)
            assert a.shape[0] == self.n_reads
            self._chk(self.L.itsx_set_samples(self.h, a.ctypes.data if a.size else None, int(n_samples)))
        self.n_samples = max(1, self.L.itsx_num_samples(self.h))

    def select_sample(self, sample):
        """Restrict write_uc / write_rep_fasta / write_domtbl to one sample of the batch (-1 = all)."""
        self._chk(self.L.itsx_select_sample(self.h, int(sample)))

    # ---- derep
    def derep(self, strand_both=True, minseqlength=1):
        n = C.c_int64(0)
        self._chk(self.L.itsx_derep(self.h, int(strand_both), int(minseqlength), C.byref(n)))
        self.n_unique = n.value
        return n.value

    def cluster(self, cluster_id, strand_both=True, helpers=None):
        """Greedy clustering (itsx_cluster).  helpers: other Engines (no reads needed, any devices) that each take a shard of the
        centroid stream for this call (itsx_cluster_multi); the result is the same bit for bit.  None or empty: itsx_cluster."""
        n = C.c_int64(0)
        if helpers:
            hs = list(helpers)
            arr = (C.c_void_p * len(hs))(*[h.h for h in hs])
            self._chk(self.L.itsx_cluster_multi(self.h, arr, len(hs), float(cluster_id), int(strand_both), C.byref(n)))
        else:
            self._chk(self.L.itsx_cluster(self.h, float(cluster_id), int(strand_both), C.byref(n)))
        self.n_unique = n.value
        return n.value

    def cluster_samples(self, cluster_id, strand_both=True):
        """cluster(cluster_id) of every sample of the batch (set_samples) in one call: each sample's clusters are those of
        a run of that sample alone.  With one sample this is cluster()."""
        n = C.c_int64(0)
        self._chk(self.L.itsx_cluster_samples(self.h, float(cluster_id), int(strand_both), C.byref(n)))
        self.n_unique = n.value
        return n.value

    # ---- f4: read orientation
    def orient_load_db(self, fasta_path):
        if not os.path.exists(fasta_path):
            raise FileNotFoundError(fasta_path)
        n = C.c_int64(0)
        self._chk(self.L.itsx_orient_load_db(self.h, os.fsencode(fasta_path), C.byref(n)))
        return n.value

    def orient(self):
        """strand int8[n_reads] (+1 forward, -1 reverse, 0 undetermined), count_fwd, count_rev of the loaded reads"""
        strand = np.zeros(max(1, self.n_reads), np.int8)
        cf = np.zeros(max(1, self.n_reads), np.int32)
        cr = np.zeros(max(1, self.n_reads), np.int32)
        self._chk(self.L.itsx_orient(self.h, strand.ctypes.data, cf.ctypes.data, cr.ctypes.data))
        return strand[:self.n_reads], cf[:self.n_reads], cr[:self.n_reads]

    def orient_apply(self):
        """orient the loaded reads (every sample of a batch) and make the reads `vsearch --orient --fastqout` keeps this engine's read
        set, on the device: forward reads as they are, reverse ones reverse-complemented, undetermined ones dropped -- the state
        load_reads_files leaves after loading the samples' oriented.fq files.  Returns (strand, count_fwd, count_rev) of the reads
        BEFORE the call and the reads kept per sample."""
        n = self.n_reads
        strand = np.zeros(max(1, n), np.int8)
        cf = np.zeros(max(1, n), np.int32)
        cr = np.zeros(max(1, n), np.int32)
        kept = np.zeros(max(1, self.n_samples), np.int64)
        self._chk(self.L.itsx_orient_apply(self.h, strand.ctypes.data, cf.ctypes.data, cr.ctypes.data, kept.ctypes.data))
        kept = kept[:max(1, self.n_samples)]
        self.n_reads, self.n_unique = int(kept.sum()), 0
        return strand[:n], cf[:n], cr[:n], kept

    def _orient_profiles(self, fn, F1):
        n = self.n_reads
        strand = np.zeros(max(1, n), np.int8)
        cf = np.zeros(max(1, n), np.int32)
        cr = np.zeros(max(1, n), np.int32)
        ms = C.c_float(0)
        self._chk(fn(self.h, float(F1), strand.ctypes.data, cf.ctypes.data, cr.ctypes.data, C.byref(ms)))
        self.last_orient_ms = float(ms.value)
        self.n_unique = 0
        return strand[:n], cf[:n], cr[:n]

    def orient_profiles(self, F1=1e-6):
        """Orientation by the loaded profiles (itsx_orient_profiles): per read strand int8 (+1 if more profiles pass the MSV filter at
        F1 on the read than on its reverse complement, -1 if fewer, 0 if equally many -- none, or a tie), count_fwd, count_rev.  The
        call dereplicates the reads itself and leaves no dereplication behind; last_orient_ms is the device time of its kernels."""
        return self._orient_profiles(self.L.itsx_orient_profiles, F1)

    def orient_profiles_apply(self, F1=1e-6):
        """orient_profiles(), and the reads of strand -1 reverse-complemented where they are (packed words, exceptions, the host text,
        with keep_records the records).  Unlike orient_apply() a read of strand 0 is kept as it is: the number of reads, their order
        and their samples do not change.  Returns (strand, count_fwd, count_rev) of the reads before the call."""
        out = self._orient_profiles(self.L.itsx_orient_profiles_apply, F1)
        self.read_set += 1
        return out

    def orient_file(self, fastq):
        """load a FASTQ file and orient its reads (what SeqSample.orient_reads needs in one call)"""
        self.load_reads_file(fastq)
        return self.orient()

    # ---- f2: paired-end merge
    def merge_pairs(self, fwd, fqual, rev, rqual, maxdiffs=40, maxee=2.0, allow_stagger=False, join=False):
        """Lists of equal length (str): forward reads / qualities, reverse reads / qualities as they are in the file.
        Returns (reason int32[n], merged list[(seq, qual) or None], score float64[n], shift int32[n]).
        join=True (itsx_merge_buffers_join; the merge_join setting is not consulted): a pair rejected with reason 1, 3 or 5 is joined,
        its (bases, quals) stand in the list, and a fifth array joined int8[n] marks it."""
        n = len(fwd)
        enc = lambda xs: ("".join(xs)).encode()
        fo = np.zeros(n + 1, np.int64); np.cumsum([len(x) for x in fwd], out=fo[1:])
        ro = np.zeros(n + 1, np.int64); np.cumsum([len(x) for x in rev], out=ro[1:])
        fs, fq, rs, rq = enc(fwd), enc(fqual), enc(rev), enc(rqual)
        assert len(fs) == len(fq) and len(rs) == len(rq)
        pad = 8 if join else 0                               # a slot holds 8 bytes more than the mates
        cap = int(fo[-1] + ro[-1]) + pad * n + 1
        oseq = C.create_string_buffer(cap)
        oqual = C.create_string_buffer(cap)
        olen = np.zeros(max(1, n), np.int32)
        reason = np.zeros(max(1, n), np.int32)
        score = np.zeros(max(1, n), np.float64)
        shift = np.zeros(max(1, n), np.int32)
        joined = np.zeros(max(1, n), np.int8)
        if join:
            self._chk(self.L.itsx_merge_buffers_join(self.h, fs, fq, fo.ctypes.data, rs, rq, ro.ctypes.data, n, int(maxdiffs), float(maxee),
                                                     int(allow_stagger), oseq, oqual, olen.ctypes.data, reason.ctypes.data,
                                                     score.ctypes.data, shift.ctypes.data, joined.ctypes.data))
        else:
            self._chk(self.L.itsx_merge_buffers(self.h, fs, fq, fo.ctypes.data, rs, rq, ro.ctypes.data, n, int(maxdiffs), float(maxee),
                                                int(allow_stagger), oseq, oqual, olen.ctypes.data, reason.ctypes.data,
                                                score.ctypes.data, shift.ctypes.data))
        merged = []
        sraw, qraw = oseq.raw, oqual.raw
        for i in range(n):
            o = int(fo[i] + ro[i]) + pad * i
            merged.append((sraw[o:o + olen[i]].decode(), qraw[o:o + olen[i]].decode()) if (reason[i] == 0 or joined[i]) else None)
        if join:
            return reason[:n], merged, score[:n], shift[:n], joined[:n]
        return reason[:n], merged, score[:n], shift[:n]

    def merge_pairs_files(self, r1, r2, out, maxdiffs=40, maxee=2.0, allow_stagger=False):
        for p in (r1, r2):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        n = C.c_int64(0)
        m = C.c_int64(0)
        self._chk(self.L.itsx_merge_pairs_files(self.h, os.fsencode(r1), os.fsencode(r2), os.fsencode(out), int(maxdiffs),
                                                float(maxee), int(allow_stagger), C.byref(n), C.byref(m)))
        self._n_joined_files = self._n_joined(n.value)       # (merge_join: the joined records the file holds beside the m merged ones)
        return n.value, m.value

    def merge_pairs_load(self, r1, r2, maxdiffs=40, maxee=2.0, allow_stagger=False):
        """merge R1 / R2 and leave the merged reads as this engine's read set (nothing written): (pairs, merged)"""
        for p in (r1, r2):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        n = C.c_int64(0)
        m = C.c_int64(0)
        self._chk(self.L.itsx_merge_pairs_load(self.h, os.fsencode(r1), os.fsencode(r2), int(maxdiffs), float(maxee), int(allow_stagger),
                                               C.byref(n), C.byref(m)))
        self.n_reads, self.n_samples, self.n_unique = m.value + self._n_joined(n.value), 1, 0      # (the reads: merged and joined)
        self._n_pairs = n.value
        self._last_merge = dict(r1=r1, r2=r2, maxdiffs=int(maxdiffs), maxee=float(maxee), allow_stagger=bool(allow_stagger), join=self.merge_join)
        return n.value, m.value

    def merge_pairs_load_text(self, ptr1, nb1, ptr2, nb2, maxdiffs=40, maxee=2.0, allow_stagger=False):
        """the same from record-aligned pieces of R1's and R2's text in memory that hold the same number of records (addresses + lengths:
        slices of itsxpress_amd.stream's two text streams): (pairs, merged, per pair the index of its merged read or -1)"""
        n = C.c_int64(0)
        m = C.c_int64(0)
        self._chk(self.L.itsx_merge_pairs_load_text(self.h, C.c_void_p(ptr1), int(nb1), C.c_void_p(ptr2), int(nb2), int(maxdiffs), float(maxee),
                                                    int(allow_stagger), C.byref(n), C.byref(m)))
        self.n_reads, self.n_samples, self.n_unique = m.value + self._n_joined(n.value), 1, 0
        self._n_pairs = n.value
        idx = np.zeros(max(1, n.value), np.int32)
        self._chk(self.L.itsx_merge_pair_index(self.h, idx.ctypes.data, n.value))
        return n.value, m.value, idx[:n.value]

    def merge_pairs_load_files(self, r1s, r2s, seq_outs=None, maxdiffs=40, maxee=2.0, allow_stagger=False):
        """The pairs of every sample of a batch (sample s = r1s[s] / r2s[s]) through one merge; the merged reads of all samples, in sample
        order, become this engine's read set with one sample per file pair (as load_reads_files leaves it).  seq_outs: None, or per
        sample None or the path its merged records are written to (what merge_pairs_files writes for it alone).
        Returns (n_pairs[S], n_merged[S])."""
        S = len(r1s)
        if S < 1 or len(r2s) != S or (seq_outs is not None and len(seq_outs) != S):
            raise ValueError("merge_pairs_load_files: one R1, one R2 (and one output or None) per sample, at least one sample")
        for p in list(r1s) + list(r2s):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        a1 = (C.c_char_p * S)(*[os.fsencode(p) for p in r1s])
        a2 = (C.c_char_p * S)(*[os.fsencode(p) for p in r2s])
        ao = None
        if seq_outs is not None and any(p is not None for p in seq_outs):
            ao = (C.c_char_p * S)(*[None if p is None else os.fsencode(p) for p in seq_outs])
        n = np.zeros(S, np.int64)
        m = np.zeros(S, np.int64)
        self._last_merge = None
        try:
            self._chk(self.L.itsx_merge_pairs_load_files(self.h, a1, a2, ao, S, int(maxdiffs), float(maxee), int(allow_stagger),
                                                         n.ctypes.data, m.ctypes.data))
        except EngineError:
            self.n_reads, self.n_samples, self.n_unique, self._n_pairs = 0, 1, 0, 0      # the context is left empty
            raise
        self.n_reads, self.n_unique = int(m.sum()) + self._n_joined(int(n.sum())), 0
        self.n_samples = max(1, self.L.itsx_num_samples(self.h))
        self._n_pairs = int(n.sum())
        return n, m

    def merge_pair_index(self):
        """After merge_pairs_load_files: per pair of the batch (sample order, then pair order) the index of its merged read in the
        batch's read set, -1 = not merged.  After merge_pairs_load: the same for that one sample's pairs."""
        n = int(getattr(self, "_n_pairs", 0))
        idx = np.zeros(max(1, n), np.int32)
        self._chk(self.L.itsx_merge_pair_index(self.h, idx.ctypes.data, n))
        return idx[:n]

    def write_merged_fastq(self, path):
        """After merge_pairs_load (which writes nothing): the merged records as a FASTQ file after all -- the same merge once more, in a
        context of its own (this engine's read set and results stay as they are); record i of the file is read i of this engine.  For
        the consumer that wants the MERGED reads trimmed (Dedup.create_trimmed_seqs on a paired sample, itsxpress/main.py:596-624)."""
        lm = getattr(self, "_last_merge", None)
        if lm is None:
            raise EngineError(-1, "write_merged_fastq: this engine's reads do not come from merge_pairs_load")
        tmp = Engine(self.device)
        try:
            tmp.merge_join = bool(lm.get("join", False))      # the same merge: joined records too, where the reads hold them
            n, m = tmp.merge_pairs_files(lm["r1"], lm["r2"], path, maxdiffs=lm["maxdiffs"], maxee=lm["maxee"], allow_stagger=lm["allow_stagger"])
            m += tmp._n_joined_files
        finally:
            tmp.close()
        if m != self.n_reads:
            raise EngineError(-1, "write_merged_fastq: %d merged records written, the engine holds %d" % (m, self.n_reads))
        return m

    def get_cluster(self):
        """After cluster(id < 1): (pct_id float64[n_reads] (-1 for centroids / dropped), order int64[kept])."""
        pct = np.zeros(self.n_reads, np.float64)
        order = np.zeros(max(1, self.n_reads), np.int64)
        n = C.c_int64(0)
        self._chk(self.L.itsx_get_cluster(self.h, pct.ctypes.data, order.ctypes.data, C.byref(n)))
        return pct, order[:n.value]

    def align_clusters(self):
        """After cluster(id < 1) / cluster_samples: the alignment of every member with its centroid (csrc/k_cigar.hip), what fills
        column 8 of write_uc's H rows ('*' without it).  Dropped by whatever changes the clustering.
        Returns {"n_aligned": members that have a text, "ms_kernels": device time of the stage}."""
        n, ms = C.c_int64(0), C.c_float(0.0)
        self._chk(self.L.itsx_align_clusters(self.h, C.byref(n), C.byref(ms)))
        return {"n_aligned": int(n.value), "ms_kernels": float(ms.value)}

    def get_cluster_cigars(self):
        """list of str over the reads, after align_clusters(): a member's run-length alignment with its centroid (M / I / D, a run
        of one without its count; '=' for a member that equals its centroid on its strand), '' for centroids and dropped reads"""
        offs = np.zeros(self.n_reads + 1, np.int64)
        self._chk(self.L.itsx_get_cluster_cigars(self.h, offs.ctypes.data, None))
        text = C.create_string_buffer(max(1, int(offs[-1])))
        self._chk(self.L.itsx_get_cluster_cigars(self.h, offs.ctypes.data, text))
        raw = text.raw
        return [raw[offs[r]:offs[r + 1]].decode("ascii") for r in range(self.n_reads)]

    def get_derep(self):
        rep_of = np.zeros(self.n_reads, np.int64)
        strand = np.zeros(self.n_reads, np.int8)
        uniq_of = np.zeros(self.n_reads, np.int64)
        self._chk(self.L.itsx_get_derep(self.h, rep_of.ctypes.data, strand.ctypes.data, uniq_of.ctypes.data))
        return rep_of, strand, uniq_of

    def unique_keys(self, seed=0):
        """XXH64(seed) of every local unique's forward strand and reverse complement (uint64[U] each)."""
        kf = np.zeros(max(1, self.n_unique), np.uint64)
        kr = np.zeros(max(1, self.n_unique), np.uint64)
        self._chk(self.L.itsx_unique_keys(self.h, C.c_uint64(seed), kf.ctypes.data, kr.ctypes.data))
        return kf[:self.n_unique], kr[:self.n_unique]

    def set_active_uniques(self, active):
        a = np.ascontiguousarray(active, np.uint8)
        assert a.shape[0] == self.n_unique
        self._chk(self.L.itsx_set_active_uniques(self.h, a.ctypes.data if a.size else None))

    def read_names_raw(self):
        """labels of the loaded reads, in input order: (bytes blob, int64 offsets[n_reads + 1]) -- the form the paired
        writer takes without a detour through a million Python strings"""
        offs = np.zeros(self.n_reads + 1, np.int64)
        self._chk(self.L.itsx_get_read_names(self.h, None, 0, offs.ctypes.data))
        buf = C.create_string_buffer(int(offs[-1]) + 1)
        self._chk(self.L.itsx_get_read_names(self.h, buf, int(offs[-1]), offs.ctypes.data))
        return buf.raw[:int(offs[-1])], offs

    def read_names(self):
        """labels of the loaded reads, in input order (list[str])"""
        blob, offs = self.read_names_raw()
        blob = blob.decode()
        return [blob[offs[i]:offs[i + 1]] for i in range(self.n_reads)]

    def get_uniques(self):
        seed = np.zeros(self.n_unique, np.int64)
        ab = np.zeros(self.n_unique, np.int64)
        self._chk(self.L.itsx_get_uniques(self.h, seed.ctypes.data, ab.ctypes.data))
        return seed, ab

    # ---- search
    def search(self, T=10.0, F1=1e-6, F2=1e-6, F3=1e-6):
        self._chk(self.L.itsx_search(self.h, T, F1, F2, F3))

    ROWS_FULL, ROWS_COMPACT, ROWS_LAZY = 0, 1, 2

    def set_rows_mode(self, mode):
        """What search() keeps of the domain table: "full" (every row: domtbl.txt), "compact" (every pair evaluated, only the rows
        that can still win ItsPosition's argmax kept), "lazy" (pairs that cannot win it are not evaluated past their Forward score;
        same coordinates), None = from the environment (ITSX_ROWS / ITSX_COMPACT_ROWS)."""
        m = {None: -1, "env": -1, "full": 0, "compact": 1, "lazy": 2}.get(mode, mode)
        self._chk(self.L.itsx_set_rows_mode(self.h, int(m)))
        self.rows_mode = int(m)

    def set_kept_rows(self, on=True):
        """After a "compact" / "lazy" search: domains() / write_domtbl() serve the WINNERS among the rows the context kept (per target and
        2-character profile prefix the reported row ItsPosition's argmax ends up with -- a row of the full table) instead of refusing."""
        self._chk(self.L.itsx_set_kept_rows(self.h, 1 if on else 0))

    def lazy_pending(self):
        """after finalize() of a lazy search whose counters were exchanged: rows that still depend on the exact domZ (> 0: search
        again in "compact" mode on every rank)"""
        return int(self.L.itsx_lazy_pending(self.h))

    def lazy_pending_profiles(self):
        """int32[n_profiles]: 1 where a pending row belongs to the profile"""
        f = np.zeros(max(1, self.n_profiles), np.int32)
        self._chk(self.L.itsx_lazy_pending_profiles(self.h, f.ctypes.data))
        return f[:self.n_profiles]

    def lazy_pending_uniques(self):
        """uint8[n_unique]: 1 where an undecided row could still change the representative's coordinates"""
        f = np.zeros(max(1, self.n_unique), np.uint8)
        self._chk(self.L.itsx_lazy_pending_uniques(self.h, f.ctypes.data))
        return f[:self.n_unique]

    def set_partial_coords(self, on=True):
        """rep_coords / trim_coords answer although rows are undecided (the caller skips the flagged representatives)"""
        self._chk(self.L.itsx_set_partial_coords(self.h, 1 if on else 0))

    def lazy_complete(self, flags):
        """count the flagged profiles' reported targets exactly (every pair of theirs is evaluated); then exchange / finalize again"""
        f = np.ascontiguousarray(flags, np.int32)
        assert f.size == self.n_profiles
        self._chk(self.L.itsx_lazy_complete(self.h, f.ctypes.data))

    def get_domz(self):
        z = np.zeros(max(1, int(self.L.itsx_domz_count(self.h))), np.int64)      # [sample][profile] (x 2 after a lazy search: lower, upper bounds)
        self._chk(self.L.itsx_get_domz(self.h, z.ctypes.data))
        return z[:int(self.L.itsx_domz_count(self.h))]

    def set_domz(self, z):
        z = np.ascontiguousarray(z, np.int64)
        assert z.size == int(self.L.itsx_domz_count(self.h))
        self._chk(self.L.itsx_set_domz(self.h, z.ctypes.data))

    # ---- device-resident exchange (multi-GPU drivers): torch tensors over the engine's own device memory, no copies
    def _torch_device(self, device=None):
        import torch
        return device if device is not None else torch.device("cuda", self.device)

    def domz_device(self, device=None):
        """int64[n_samples * n_profiles] reported-target counters ON THE DEVICE: all-reduce in place, then finalize()."""
        p, n = C.c_void_p(0), C.c_int64(0)
        self._chk(self.L.itsx_domz_device(self.h, C.byref(p), C.byref(n)))
        return _devtensor(p.value, (n.value,), "<i8", self._torch_device(device))

    def _coords_device(self, fn, left, right, device):
        p, n = C.c_void_p(0), C.c_int64(0)
        self._chk(fn(self.h, left.encode(), right.encode(), C.byref(p), C.byref(n)))
        return _devtensor(p.value, (n.value, 4), "<i4", self._torch_device(device))

    def trim_coords_device(self, left, right, device=None):
        """int32 [n_reads, 4] rows (start, stop, tlen, in_ddict) on the device."""
        return self._coords_device(self.L.itsx_trim_coords_device, left, right, device)

    def rep_coords_device(self, left, right, device=None):
        return self._coords_device(self.L.itsx_rep_coords_device, left, right, device)

    def derep_device(self, device=None):
        """dict of device tensors: rep_of, uniq_of (int32[n_reads]), strand (int8[n_reads]), seed_read (int32[n_unique])."""
        a, b, c, d = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
        self._chk(self.L.itsx_derep_device(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        dev = self._torch_device(device)
        return dict(rep_of=_devtensor(a.value, (self.n_reads,), "<i4", dev), uniq_of=_devtensor(b.value, (self.n_reads,), "<i4", dev),
                    strand=_devtensor(c.value, (self.n_reads,), "|i1", dev), seed_read=_devtensor(d.value, (self.n_unique,), "<i4", dev))

    def unique_tuples(self, gidx_base, device=None, seeds=(0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179)):
        """int64 [n_unique, 4] rows on the device: the orientation-free 128-bit key of each local unique (two XXH64 seeds),
        gidx_base + index of its first occurrence, 1 if the forward strand is the canonical orientation."""
        p, n = C.c_void_p(0), C.c_int64(0)
        self._chk(self.L.itsx_unique_keys128_device(self.h, C.c_uint64(seeds[0]), C.c_uint64(seeds[1]), int(gidx_base), C.byref(p), C.byref(n)))
        return _devtensor(p.value, (n.value, 4), "<i8", self._torch_device(device))

    def finalize(self, domE=10.0):
        self._chk(self.L.itsx_search_finalize(self.h, domE))

    def domains(self):
        n = self.L.itsx_num_domains(self.h)
        if n < 0:
            raise EngineError(-1, self.L.itsx_last_error(self.h).decode())
        out = np.zeros(n, DOMAIN_DTYPE)
        if n:
            self._chk(self.L.itsx_get_domains(self.h, out.ctypes.data))
        return out

    def align_domains(self):
        """The optimal-accuracy alignment of every reported domain row, after finalize(): what fills the hmm / ali / acc columns of
        write_domtbl (placeholders without it).  Dropped by whatever changes the rows or their reporting.
        Returns {"n_aligned": rows aligned, "ms_kernels": device time of the stage}."""
        n, ms = C.c_int64(0), C.c_float(0.0)
        self._chk(self.L.itsx_align_domains(self.h, C.byref(n), C.byref(ms)))
        return {"n_aligned": int(n.value), "ms_kernels": float(ms.value)}

    def alignments(self):
        """ALIGNMENT_DTYPE rows parallel to domains(): aligned == 1 where the row is reported, all zero elsewhere"""
        n = self.L.itsx_num_domains(self.h)
        if n < 0:
            raise EngineError(-1, self.L.itsx_last_error(self.h).decode())
        out = np.zeros(max(n, 1), ALIGNMENT_DTYPE)
        self._chk(self.L.itsx_get_alignments(self.h, out.ctypes.data))
        return out[:n]

    def pairtraces(self):
        n = self.L.itsx_num_pairtraces(self.h)
        if n < 0:
            raise EngineError(-1, self.L.itsx_last_error(self.h).decode())
        out = np.zeros(n, TRACE_DTYPE)
        if n:
            self._chk(self.L.itsx_get_pairtraces(self.h, out.ctypes.data, TRACE_DTYPE.itemsize))
        return out

    def _coords(self, fn, n, left, right):
        a = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        self._chk(fn(self.h, left.encode(), right.encode(), *[x.ctypes.data for x in a]))
        return tuple(x[:n] for x in a)

    def trim_coords(self, left, right):
        """per READ: start, stop, tlen (-1 = None), in_ddict."""
        return self._coords(self.L.itsx_trim_coords, self.n_reads, left, right)

    def rep_coords(self, left, right):
        return self._coords(self.L.itsx_rep_coords, self.n_unique, left, right)

    # ---- f1 for a batch: trimmed FASTQ from the records the context keeps
    def keep_records(self, on=True):
        """From now on the read sets that load_reads_files / merge_pairs_load(_files) / orient_apply leave also keep their FASTQ
        records (bases as in the input, qualities, title lines) on the device: what write_trimmed_samples cuts from."""
        self._chk(self.L.itsx_keep_records(self.h, int(bool(on))))

    def write_trimmed_samples(self, paths, region_prefixes=None, start=None, stop=None, gzipped=False, zstd_file=False, trim_ccs=False):
        """The trimmed FASTQ of every sample of the batch (paths[s]; None skips a sample) in one call, from the records the context
        keeps.  Coordinates: region_prefixes = (left, right) of the finalized search, or start / stop arrays over the reads --
        exactly one of the two.  Returns the per-sample (n_written, total_len) pairs.
        With self.deflate = "device" the gzip bytes (gzipped=True) are made on the device."""
        kind = _batch_compression(gzipped, zstd_file, self.deflate, "write_trimmed_samples")
        S = len(paths)
        arr = (C.c_char_p * max(1, S))(*[None if p is None else os.fsencode(p) for p in paths])
        left = right = None
        if region_prefixes is not None:
            left, right = (x.encode() for x in region_prefixes)
        keep = []
        for a in (start, stop):
            if a is None:
                keep.append(None)
                continue
            a = np.ascontiguousarray(a, np.int32)
            if a.shape[0] != self.n_reads:
                raise ValueError("write_trimmed_samples: start / stop hold one entry per read")
            keep.append(a if a.size else np.zeros(1, np.int32))
        nw = np.zeros(max(1, S), np.int64)
        tot = np.zeros(max(1, S), np.int64)
        self._chk(self.L.itsx_write_trimmed_samples(self.h, arr, S, kind, int(bool(trim_ccs)), left, right,
                                                    None if keep[0] is None else keep[0].ctypes.data,
                                                    None if keep[1] is None else keep[1].ctypes.data, nw.ctypes.data, tot.ctypes.data))
        return [(int(nw[s]), int(tot[s])) for s in range(S)]

    # ---- the feature table of the trimmed regions (distinct trimmed sequences by samples)
    def trimmed_table(self, region_prefixes=None, start=None, stop=None, min_len=1):
        """The trimmed regions of the read set dereplicated over all its samples (itsx_trimmed_table): a FeatureTable.
        Read i is counted iff the trimmed-FASTQ writer would write it and min(stop, len) - start >= min_len; two counted reads are one
        feature iff their slices are equal symbol for symbol (upper case, U is T, IUPAC symbols kept; forward strand; no trim_ccs
        stitching).  Features are ordered by descending total, ties by the smaller index of the first read, which is the representative.
        Coordinates: region_prefixes = (left, right) of the finalized search, or start / stop arrays over the reads -- exactly one of
        the two.  One GPU, a whole-file read set."""
        left = right = None
        if region_prefixes is not None:
            left, right = (x.encode() for x in region_prefixes)
        keep = []
        for a in (start, stop):
            if a is None:
                keep.append(None)
                continue
            a = np.ascontiguousarray(a, np.int32)
            if a.shape[0] != self.n_reads:
                raise ValueError("trimmed_table: start / stop hold one entry per read")
            keep.append(a if a.size else np.zeros(1, np.int32))
        nf, ne, nc, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        self._chk(self.L.itsx_trimmed_table(self.h, left, right, None if keep[0] is None else keep[0].ctypes.data,
                                            None if keep[1] is None else keep[1].ctypes.data, int(min_len),
                                            C.byref(nf), C.byref(ne), C.byref(nc), C.byref(ms)))
        F, E = int(nf.value), int(ne.value)
        t = FeatureTable()
        t.n_samples = int(self.L.itsx_num_samples(self.h))
        t.n_counted = int(nc.value)
        t.ms_kernels = float(ms.value)
        t.lengths, t.totals, t.first_read = (np.zeros(F, np.int32) for _ in range(3))
        t.row_off = np.zeros(F + 1, np.int64)
        t.entry_sample, t.entry_count = np.zeros(E, np.int32), np.zeros(E, np.int32)
        pad = lambda x: x.ctypes.data if x.size else None
        self._chk(self.L.itsx_trimmed_table_get(self.h, pad(t.lengths), pad(t.totals), pad(t.first_read), t.row_off.ctypes.data,
                                                pad(t.entry_sample), pad(t.entry_count)))
        t.feature_of_read = np.zeros(max(self.n_reads, 1), np.int32)
        self._chk(self.L.itsx_trimmed_table_reads(self.h, t.feature_of_read.ctypes.data))
        t.feature_of_read = t.feature_of_read[:self.n_reads]
        t.seq_off = np.zeros(F + 1, np.int64)
        self._chk(self.L.itsx_trimmed_table_seqs(self.h, None, t.seq_off.ctypes.data))
        buf = C.create_string_buffer(int(t.seq_off[-1]) + 1)
        self._chk(self.L.itsx_trimmed_table_seqs(self.h, buf, None))
        t.bases = buf.raw[:int(t.seq_off[-1])]
        return t

    # ---- the feature table denoised into ZOTUs (the UNOISE rule)
    def denoise_table(self, alpha=2.0, minsize=8, max_diffs=None, max_skew=None):
        """The table of the last trimmed_table denoised (itsx_denoise_table): a DenoisedTable.  Features in table order; centroid t
        takes feature q iff 1 <= d <= D (Levenshtein, symbols compared literally) and a_q <= max_skew[d - 1] * a_t; q joins the taker
        with the smallest d, then the smallest t; an untaken q with a_q >= minsize is the next ZOTU, any other is unassigned and its
        reads are dropped.  max_skew: unoise_skews(alpha, largest total, max_diffs) unless given (non-increasing values inside (0, 1),
        at most 31).  The project's own statement of the rule: parity with usearch / vsearch is not pinned; no chimera step; one GPU,
        whole-file read sets."""
        nf = C.c_int64(0)
        self._chk(self.L.itsx_trimmed_table_size(self.h, C.byref(nf), None, None))      # (the context's own F sizes the arrays below)
        F = int(nf.value)
        totals = np.zeros(max(F, 1), np.int32)
        self._chk(self.L.itsx_trimmed_table_get(self.h, None, totals.ctypes.data if F else None, None, None, None, None))
        if max_skew is None:
            max_skew = unoise_skews(alpha, int(totals[0]) if F else 0, max_diffs)
        skew = np.ascontiguousarray(max_skew, np.float64)
        buf = skew if skew.size else np.zeros(1, np.float64)
        nz, ne, nd, npairs, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_float(0)
        self._chk(self.L.itsx_denoise_table(self.h, buf.ctypes.data, int(skew.size), int(minsize), C.byref(nz), C.byref(ne), C.byref(nd),
                                            C.byref(npairs), C.byref(ms)))
        Z, E = int(nz.value), int(ne.value)
        t = DenoisedTable()
        t.n_samples = int(self.L.itsx_num_samples(self.h))
        t.n_dropped_reads, t.n_pairs, t.ms_kernels, t.max_skew = int(nd.value), int(npairs.value), float(ms.value), skew
        t.zotu_feature, t.totals = np.zeros(Z, np.int32), np.zeros(Z, np.int32)
        t.row_off = np.zeros(Z + 1, np.int64)
        t.entry_sample, t.entry_count = np.zeros(E, np.int32), np.zeros(E, np.int32)
        t.zotu_of_feature, t.dist_of_feature = np.zeros(F, np.int32), np.zeros(F, np.int32)
        pad = lambda x: x.ctypes.data if x.size else None
        self._chk(self.L.itsx_denoise_table_get(self.h, pad(t.zotu_feature), pad(t.totals), t.row_off.ctypes.data, pad(t.entry_sample),
                                                pad(t.entry_count)))
        self._chk(self.L.itsx_denoise_table_features(self.h, pad(t.zotu_of_feature), pad(t.dist_of_feature)))
        nl, sk, sl, co = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self.L.itsx_denoise_table_info(self.h, C.byref(nl), C.byref(sk), C.byref(sl), C.byref(co)))
        t.n_levels, t.n_skipped_skew, t.n_skipped_length, t.n_columns = int(nl.value), int(sk.value), int(sl.value), int(co.value)
        return t

    # ---- f1 for a batch of paired samples: trimmed R1 / R2 FASTQ from the pair records the context keeps
    def keep_pair_records(self, on=True):
        """From now on merge_pairs_load(_files) also keeps the ORIGINAL pairs on the device beside the merged read set (R1's and R2's
        bases, qualities and title lines, and which read each pair is sliced with): what write_trimmed_paired_samples cuts from.
        Independent of keep_records."""
        self._chk(self.L.itsx_keep_pair_records(self.h, int(bool(on))))

    def write_trimmed_paired_samples(self, paths1, paths2, region_prefixes=None, start=None, stop=None, tlen=None, gzipped=False,
                                     zstd_file=False, trim_ccs=False):
        """The trimmed R1 / R2 FASTQ of every paired sample of the batch (paths1[s], paths2[s]; None for both skips a sample) in one
        call, from the pair records the context keeps.  Coordinates: region_prefixes = (left, right) of the finalized search, or
        start / stop / tlen arrays over the merged reads -- exactly one of the two.  Returns the pairs written per sample.
        The given paths belong to the call: if any file cannot be written, EVERY path it was given is removed, also one that held a
        file before the call and had not been opened yet, so that no half of a pair of files is left behind.
        With self.deflate = "device" the gzip bytes (gzipped=True) are made on the device."""
        kind = _batch_compression(gzipped, zstd_file, self.deflate, "write_trimmed_paired_samples")
        S = len(paths1)
        if len(paths2) != S:
            raise ValueError("write_trimmed_paired_samples: one R1 and one R2 path per sample")
        arr1 = (C.c_char_p * max(1, S))(*[None if p is None else os.fsencode(p) for p in paths1])
        arr2 = (C.c_char_p * max(1, S))(*[None if p is None else os.fsencode(p) for p in paths2])
        left = right = None
        if region_prefixes is not None:
            left, right = (x.encode() for x in region_prefixes)
        keep = []
        for a in (start, stop, tlen):
            if a is None:
                keep.append(None)
                continue
            a = np.ascontiguousarray(a, np.int32)
            if a.shape[0] != self.n_reads:
                raise ValueError("write_trimmed_paired_samples: start / stop / tlen hold one entry per merged read")
            keep.append(a if a.size else np.zeros(1, np.int32))
        nw = np.zeros(max(1, S), np.int64)
        self._chk(self.L.itsx_write_trimmed_paired_samples(self.h, arr1, arr2, S, kind, int(bool(trim_ccs)), left, right,
                                                           *[None if k is None else k.ctypes.data for k in keep], nw.ctypes.data))
        return [int(nw[s]) for s in range(S)]

    # ---- the device deflate by itself
    def deflate_device(self, data, bounds):
        """Ranges [bounds[r], bounds[r + 1]) of data (bounds[0] = 0, bounds[-1] = len(data)) as gzip files made on the device: one
        bytes object per range, each the concatenated gzip members of that range's blocks (an empty range: one empty member)."""
        data = bytes(data)
        b = np.ascontiguousarray(bounds, np.int64)
        if b.ndim != 1 or b.size < 1:
            raise ValueError("deflate_device: bounds holds at least one entry")
        R = int(b.size) - 1
        cap = int(self.L.itsx_deflate_bound(len(data), R))
        out = np.empty(max(cap, 1), np.uint8)
        ob = np.zeros(R + 1, np.int64)
        self._chk(self.L.itsx_deflate_device(self.h, data, len(data), b.ctypes.data, R, out.ctypes.data, cap, ob.ctypes.data))
        return [out[int(ob[r]):int(ob[r + 1])].tobytes() for r in range(R)]

    # ---- the device inflate by itself
    def inflate_device(self, data):
        """The text of a gzip file made of independent members, inflated on the device.  EngineError with code -5 when the device
        declined (not such a file, a member too long, a member that did not verify); the message names the reason and the member."""
        data = bytes(data)
        n, m = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.itsx_inflate_device(self.h, data, len(data), C.byref(n), C.byref(m)))
        out = np.empty(max(n.value, 1), np.uint8)
        self._chk(self.L.itsx_inflate_fetch(self.h, out.ctypes.data, n.value))
        self.inflate_members = int(m.value)
        return out[:n.value].tobytes()

    # ---- the device parse by itself
    PARSE_PLANES = {"off": 0, "toff": 1, "seq": 2, "qual": 3, "titles": 4}

    def parse_fetch(self, plane, lo, hi):
        """Elements [lo, hi) of "off" / "toff" (int64 array) or bytes [lo, hi) of "seq" / "qual" / "titles" of the last parse_device."""
        k = self.PARSE_PLANES[plane]
        n = max(int(hi) - int(lo), 0)
        out = np.empty(max(n, 1), np.int64 if k < 2 else np.uint8)
        self._chk(self.L.itsx_parse_fetch(self.h, k, int(lo), int(hi), out.ctypes.data))
        return out[:n].copy() if k < 2 else out[:n].tobytes()

    def parse_device(self, text, keep_qual=True):
        """FASTQ text taken apart on the device: a dict of n, off, toff (int64 arrays of n + 1), seq, qual (None unless kept) and titles
        (bytes).  EngineError with code -5 when the device declined the text (not 4 lines per record throughout, a malformed record);
        the message names the reason and the record."""
        text = bytes(text)
        n = C.c_int64(0)
        self._chk(self.L.itsx_parse_device(self.h, text, len(text), int(bool(keep_qual)), C.byref(n)))
        n = int(n.value)
        off, toff = self.parse_fetch("off", 0, n + 1), self.parse_fetch("toff", 0, n + 1)
        return dict(n=n, off=off, toff=toff, seq=self.parse_fetch("seq", 0, int(off[-1])),
                    qual=self.parse_fetch("qual", 0, int(off[-1])) if keep_qual else None, titles=self.parse_fetch("titles", 0, int(toff[-1])))

    # ---- a pair of texts through the device parse
    def parse_pairs_fetch(self, side, plane, lo, hi):
        """parse_fetch for one side (0: R1, 1: R2) of the last parse_pairs_device."""
        k = self.PARSE_PLANES[plane]
        n = max(int(hi) - int(lo), 0)
        out = np.empty(max(n, 1), np.int64 if k < 2 else np.uint8)
        self._chk(self.L.itsx_parse_pairs_fetch(self.h, int(side), k, int(lo), int(hi), out.ctypes.data))
        return out[:n].copy() if k < 2 else out[:n].tobytes()

    def parse_pairs_device(self, text1, text2):
        """R1's and R2's FASTQ text taken apart on the device as the paired merge loaders do under parse = "device", nothing merged: a
        dict of n, flags (bit 0 / 1: upper-casing changed a base of R1 / R2, bit 2 / 3: a quality of R1 / R2 outside 33..126),
        max_total (the longest pair) and sides, two dicts of off, toff, seq (upper case), qual and titles.  EngineError with code -5
        when the device declined a text or the two hold different numbers of records."""
        text1, text2 = bytes(text1), bytes(text2)
        n, flags, mx = C.c_int64(0), C.c_int32(0), C.c_int64(0)
        self._chk(self.L.itsx_parse_pairs_device(self.h, text1, len(text1), text2, len(text2), C.byref(n), C.byref(flags), C.byref(mx)))
        n = int(n.value)
        sides = []
        for s in (0, 1):
            off, toff = self.parse_pairs_fetch(s, "off", 0, n + 1), self.parse_pairs_fetch(s, "toff", 0, n + 1)
            sides.append(dict(off=off, toff=toff, seq=self.parse_pairs_fetch(s, "seq", 0, int(off[-1])), qual=self.parse_pairs_fetch(s, "qual", 0, int(off[-1])),
                              titles=self.parse_pairs_fetch(s, "titles", 0, int(toff[-1]))))
        return dict(n=n, flags=int(flags.value), max_total=int(mx.value), sides=sides)

    # ---- writers
    def write_uc(self, path):
        self._chk(self.L.itsx_write_uc(self.h, os.fsencode(path)))

    def write_rep_fasta(self, path):
        self._chk(self.L.itsx_write_rep_fasta(self.h, os.fsencode(path)))

    def write_domtbl(self, path):
        self._chk(self.L.itsx_write_domtbl(self.h, os.fsencode(path)))

    def stats(self):
        s = np.zeros(1, STATS_DTYPE_ALL)
        self._chk(self.L.itsx_get_stats(self.h, s.ctypes.data, STATS_DTYPE_ALL.itemsize))
        out = {k: (s[0][k].item() if s[0][k].ndim == 0 else s[0][k].tolist()) for k in STATS_DTYPE_ALL.names}
        # the count-only top-up round's counters (itsx_topup_counters: itsx_stats itself keeps its size)
        t = np.zeros(2, np.int64)
        self._chk(self.L.itsx_topup_counters(self.h, t.ctypes.data))
        out["n_topup_deferred"], out["n_topup_ensemble"] = int(t[0]), int(t[1])
        return out

    def release_scratch(self):
        """hand the context's DP slab (tens of GB) to the next context of this process on the device: a streamed file's chunk after
        its search (results and what finalize / complete need stay)"""
        self._chk(self.L.itsx_release_scratch(self.h))

    def switches(self, now=False):
        """the library's environment switches that were set when the last search started (now=True: that are set now), as a dict
        NAME -> value; a test hook that is not honoured (no ITSX_TEST_HOOKS=1) carries the note "(ignored: ...)" """
        h = None if now else self.h
        n = self.L.itsx_switches(h, None, 0)
        buf = C.create_string_buffer(int(n))
        self.L.itsx_switches(h, buf, n)
        return dict(line.split("=", 1) for line in buf.value.decode().split("\n") if "=" in line)

    # ---- test hooks
    def debug_set_domains(self, rows, seg_rows=None, mode="full"):
        """a hand-made domain table (DOMAIN_DTYPE rows, in segments of seg_rows rows; None: one segment) in place of a search's
        results, in rows mode "full" / "compact" / "lazy": then set_domz(), finalize() and everything behind them"""
        rows = np.ascontiguousarray(rows, DOMAIN_DTYPE)
        seg = np.ascontiguousarray([len(rows)] if seg_rows is None else seg_rows, np.int64)
        m = {"full": 0, "compact": 1, "lazy": 2}.get(mode, mode)
        self._chk(self.L.itsx_debug_set_domains(self.h, rows.ctypes.data if rows.size else None, len(rows),
                                                seg.ctypes.data if seg.size else None, len(seg), int(m)))

    def debug_get_rows(self):
        """the rows the context holds as they lie in its segments (padding included; the kept rows after "compact"; dom_reported as the
        last finalize() left it, 2 = undecided after a lazy one)"""
        n = int(self.L.itsx_debug_get_rows(self.h, None, 0))
        if n < 0:
            raise EngineError(n, self.L.itsx_last_error(self.h).decode())
        out = np.zeros(max(n, 1), DOMAIN_DTYPE)
        got = int(self.L.itsx_debug_get_rows(self.h, out.ctypes.data, n))
        if got != n:
            raise EngineError(min(got, -1), self.L.itsx_last_error(self.h).decode())
        return out[:n]

    def debug_lazy_pairs(self):
        """(records, bias): the lazy stage's pair list after a lazy search that ran as one chunk -- LAZY_PAIR_DTYPE records as they lie
        (padding: prof < 0; row-state helpers: xj < 0), rep in get_uniques() order, pass A's score fb, the bound b10 = biased %.1f
        tenths, done, and the nullsc / lazy_c k_lazy_bound read for the pair's L; bias = LAZY_TENTHS_BIAS.  EngineError in any other state."""
        bias = C.c_int32(0)
        n = int(self.L.itsx_debug_lazy_pairs(self.h, None, 0, C.byref(bias)))
        if n < 0:
            raise EngineError(n, self.L.itsx_last_error(self.h).decode())
        out = np.zeros(max(n, 1), LAZY_PAIR_DTYPE)
        got = int(self.L.itsx_debug_lazy_pairs(self.h, out.ctypes.data, n, C.byref(bias)))
        if got != n:
            raise EngineError(min(got, -1), self.L.itsx_last_error(self.h).decode())
        return out[:n], int(bias.value)

    def debug_read_hashes(self):
        f = np.zeros(self.n_reads, np.uint64)
        r = np.zeros(self.n_reads, np.uint64)
        self._chk(self.L.itsx_debug_read_hashes(self.h, f.ctypes.data, r.ctypes.data))
        return f, r

    def debug_read_samples(self):
        """(device, host): the sample of every read as the kernels and as the writers see it"""
        d = np.zeros(max(1, self.n_reads), np.int32)
        h = np.zeros(max(1, self.n_reads), np.int32)
        self._chk(self.L.itsx_debug_read_samples(self.h, d.ctypes.data, h.ctypes.data))
        return d[:self.n_reads], h[:self.n_reads]

    def debug_sorted_uniques(self):
        """the length-ordered list of (active) uniques the HMM stages walk, as it lies on the device: get_uniques() numbers"""
        out = np.zeros(max(1, self.n_unique), np.int32)
        m = int(self.L.itsx_debug_sorted_uniques(self.h, out.ctypes.data))
        if m < 0:
            raise EngineError(m, self.L.itsx_last_error(self.h).decode())
        return out[:m]

    def debug_packed_read(self, i):
        nw, ne = C.c_int32(0), C.c_int32(0)
        self._chk(self.L.itsx_debug_packed_read(self.h, i, None, C.byref(nw), None, C.byref(ne)))
        w = np.zeros(max(nw.value, 1), np.uint32)
        e = np.zeros(max(ne.value, 1), np.uint32)
        self._chk(self.L.itsx_debug_packed_read(self.h, i, w.ctypes.data, C.byref(nw), e.ctypes.data, C.byref(ne)))
        return w[:nw.value], e[:ne.value]

    def debug_dust(self, lengths):
        """the device's DUST soft mask of the current reads: a list of bool arrays"""
        tot = int(sum(lengths))
        out = np.zeros(max(tot, 1), np.uint8)
        self._chk(self.L.itsx_debug_dust(self.h, out.ctypes.data))
        o = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        return [out[o[i]:o[i + 1]].astype(bool) for i in range(len(lengths))]

    def debug_logf(self, x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros_like(x)
        self._chk(self.L.itsx_debug_logf(self.h, x.ctypes.data, len(x), out.ctypes.data))
        return out

    def debug_detmath(self, x):
        x = np.ascontiguousarray(x, np.float64)
        a = np.zeros_like(x)
        b = np.zeros_like(x)
        self._chk(self.L.itsx_debug_detmath(self.h, x.ctypes.data, len(x), a.ctypes.data, b.ctypes.data))
        return a, b


def read_fastx(path):
    """Minimal FASTA/FASTQ reader (plain, .gz or .zst, through the engine's file reader) used by the host side,
    tests and the bench: returns (names, seqs)."""
    from .trim import read_text
    lines = read_text(path).decode().split("\n")
    names, seqs = [], []
    if not lines or not lines[0]:
        return names, seqs
    if lines[0][0] == "@":
        i = 0
        while i < len(lines) and lines[i]:
            names.append(lines[i][1:].split()[0])
            seqs.append(lines[i + 1].rstrip("\r") if i + 1 < len(lines) else "")
            i += 4
    else:
        cur = []
        for line in lines:
            if line[:1] == ">":
                if names:
                    seqs.append("".join(cur))
                cur = []
                names.append(line[1:].split()[0])
            else:
                cur.append(line.strip())
        seqs.append("".join(cur))
    return names, seqs
