"""ITSXPRESS_GPUS=N: ONE sample spread over the N GPUs of a node, behind the mirror's own methods.

The reference's callers reach the hot path only through `sobj.deduplicate / cluster / _search` (itsxpress/main.py:534-554,
q2_itsxpress.py:287-309).  With ITSXPRESS_GPUS > 1 those methods drive a `MultiEngine` instead of an `Engine`: N worker processes
(started fresh with multiprocessing "spawn", BEFORE this process has touched a GPU -- it never does), one HIP context each, reads
sharded by contiguous index range.  The results are those of one GPU on the whole input, read for read and file for file:

  * exact global dereplication (SURVEY 8e option 2): every worker dereplicates its shard on its GPU; only the UNIQUES meet, by an
    orientation-free 128-bit key; per distinct sequence the global first occurrence is the representative and ONE holder of the
    sequence in the representative's orientation scores it (`owner_verdicts`, the numpy twin of dist.owner_verdicts);
  * hmmsearch's domZ is summed over the workers between search and finalize (after a lazy search: its bounds; undecided rows are
    settled by counting their profiles on every worker, csrc/k_lazy.hip);
  * per-read coordinates are composed here from the scorers' per-representative rows;
  * uc.txt / rep.fa / domtbl.txt are written from the gathered arrays by the library's context-free writers
    (csrc/writers_host.cpp), byte-identical to the files one GPU writes.

No torch, no collective library.  Round 5: the parent no longer touches anything of the size of the data (it used to sort every
worker's uniques on ONE core -- 8-46 s for 6 M uniques -- and to compose the coordinates per read).  The exchanges go worker to worker
through files under /dev/shm (memory), the pipes carry commands and counts only:
  * the owner step is hash-partitioned like dist.global_derep: key mod N owns, every worker sorts its Nth (`owner_verdicts` on a share);
  * per-read coordinates are composed IN the workers (each reads the scorers' per-representative rows) into one shared array;
  * the input file is inflated once by the parent and cut into record-aligned pieces (csrc/shard_host.cpp), R2 at R1's record counts;
    merging and orientation run on every worker's piece.
The global unique list (numbers in input order of the first occurrences) is only built when a file-compatible writer or get_derep
asks for it.  bench.py's torch.distributed / RCCL path (itsxpress_amd/dist.py) is the device-resident alternative for a driver that
already runs one process per GPU.
"""
import ctypes as C
import glob
import multiprocessing as mp
import os
import shutil
import tempfile
import time

import numpy as np

from ._lib import DOMAIN_DTYPE, EngineError

KEY_SEEDS = (0x1F83D9ABFB41BD6B, 0x5BE0CD19137E2179)


def owner_verdicts(recv, src):
    """recv [m, 5] int64 = (key0, key1, global index of the first occurrence, forward-is-canonical flag, local unique number) of
    every worker's uniques, src [m] = the worker each row came from.  Returns [m, 4] int64 per row: global index and orientation flag
    of the group's first occurrence (the representative), worker and local unique number of the holder that scores the sequence --
    one of the holders in the representative's orientation, picked by the key so that the scoring spreads evenly."""
    m = recv.shape[0]
    if m == 0:
        return np.zeros((0, 4), np.int64)
    order = np.lexsort((recv[:, 2], recv[:, 1], recv[:, 0]))
    s, ssrc = recv[order], src[order]
    first = np.ones(m, bool)
    first[1:] = (s[1:, 0] != s[:-1, 0]) | (s[1:, 1] != s[:-1, 1])
    grp = np.cumsum(first) - 1
    head = np.nonzero(first)[0]
    seed_gidx, seed_fwd = s[head, 2][grp], s[head, 3][grp]
    cand = (s[:, 3] == seed_fwd).astype(np.int64)
    run = np.cumsum(cand) - cand
    pos = run - run[head][grp]
    cnt = np.zeros(head.shape[0], np.int64)
    np.add.at(cnt, grp, cand)
    pick = np.remainder(s[head, 1], cnt)[grp]
    chosen = (cand == 1) & (pos == pick)
    sr = np.zeros(head.shape[0], np.int64)
    su = np.zeros(head.shape[0], np.int64)
    sr[grp[chosen]] = ssrc[chosen]
    su[grp[chosen]] = s[chosen, 4]
    ans = np.stack([seed_gidx, seed_fwd, sr[grp], su[grp]], axis=1)
    out = np.empty_like(ans)
    out[order] = ans
    return out


def owner_verdicts_native(recv, src):
    """owner_verdicts through the library (csrc/shard_host.cpp: buckets by the key's top byte, sorted by a pool of threads): what a
    worker runs on its share of the keys -- numpy's three-key sort of 3 M rows was a second of every exchange"""
    from . import _lib
    recv = np.ascontiguousarray(recv, np.int64)
    src = np.ascontiguousarray(src, np.int64)
    m = int(recv.shape[0])
    out = np.zeros((m, 4), np.int64)
    if m:
        L = _lib.lib()
        rc = L.itsx_owner_verdicts(recv.ctypes.data, src.ctypes.data, m, out.ctypes.data)
        if rc != 0:
            raise EngineError(rc, L.itsx_shard_last_error().decode())
    return out


# ---------------------------------------------------------------------------------------------------- the worker process
def _worker_main(conn, device, rank, world):
    os.environ["ITSXPRESS_GPU"] = str(device)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.pop("ITSXPRESS_GPUS", None)             # a worker drives one GPU
    try:
        from .engine import Engine                     # the first GPU call of this process happens in here
        eng = Engine(device)
    except BaseException as e:                         # noqa: report, do not hang the parent
        conn.send(("err", (type(e).__name__, getattr(e, "code", -1), str(e))))
        return
    conn.send(("ok", None))
    st = {"rank": rank, "world": world, "base": 0}
    while True:
        try:
            cmd, args = conn.recv()
        except EOFError:
            break
        if cmd == "close":
            break
        try:
            conn.send(("ok", _HANDLERS[cmd](eng, st, *args)))
        except BaseException as e:                     # noqa
            conn.send(("err", (type(e).__name__, getattr(e, "code", -1), getattr(e, "message", str(e)))))
    try:
        eng.close()
    finally:
        conn.close()


def _h_load_shard(eng, st, path):
    tot, first, n = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    eng._chk(eng.L.itsx_load_reads_file_shard(eng.h, os.fsencode(path), st["rank"], st["world"], C.byref(tot), C.byref(first), C.byref(n)))
    eng.n_reads, eng.n_samples = n.value, 1
    st["base"] = first.value
    return tot.value, first.value, n.value


def _xpath(st, tag, src, dst):
    return "%s_%s_%d_%d.npy" % (st["xprefix"], tag, src, dst)


def _h_job(eng, st, xprefix):
    st["xprefix"] = xprefix
    return None


def _h_load_piece(eng, st, piece, base, n_expect):
    """this worker's piece of the input (cut by the parent: itsx_shard_text); the piece is memory (/dev/shm) and goes once loaded"""
    n = eng.load_reads_file(piece)
    try:
        os.unlink(piece)
    except OSError:
        pass
    if n_expect >= 0 and n != n_expect:                # (-1: dealt while the file was still being inflated; the base follows with set_base)
        raise RuntimeError("piece %s: %d records parsed, %d counted" % (piece, n, n_expect))
    st["base"] = int(base)
    return n


def _h_load_range(eng, st, path, off, nb):
    """this worker's part of the input as a byte range of a file it maps itself: the shared text the parent is still inflating
    behind this range (itsx_stream_open_shared), or the uncompressed input.  No copy of the piece; the base follows (set_base)"""
    import mmap
    if nb <= 0:
        eng.set_reads([], None)
        return 0
    gran = mmap.ALLOCATIONGRANULARITY
    a = (off // gran) * gran
    with open(path, "rb") as f:
        mm = mmap.mmap(f.fileno(), nb + (off - a), access=mmap.ACCESS_READ, offset=a)
    try:
        arr = np.frombuffer(mm, np.uint8)
        n = eng.load_reads_text(arr.ctypes.data + (off - a), nb)
        del arr
    finally:
        mm.close()
    return n


def _h_merge_piece(eng, st, p1, p2, out, maxdiffs, maxee, allow_stagger, join=False):
    """merge this worker's pieces of R1 / R2: into the engine's read set (out None) or into a piece of seq.fq; join: the parent's
    merge_join setting.  Returns (pairs, merged, joined)."""
    try:
        if bool(join) != eng.merge_join:
            eng.merge_join = bool(join)
        if out is None:
            n, m = eng.merge_pairs_load(p1, p2, maxdiffs=maxdiffs, maxee=maxee, allow_stagger=allow_stagger)
        else:
            n, m = eng.merge_pairs_files(p1, p2, out, maxdiffs=maxdiffs, maxee=maxee, allow_stagger=allow_stagger)
    finally:
        for p in (p1, p2):
            try:
                os.unlink(p)
            except OSError:
                pass
    return n, m, int(getattr(eng, "n_joined", 0))


def _h_set_base(eng, st, base):
    st["base"] = int(base)
    return None


def _h_orient_piece(eng, st, piece, db):
    eng.orient_load_db(db)
    try:
        strand, cf, cr = eng.orient_file(piece)
    finally:
        try:
            os.unlink(piece)
        except OSError:
            pass
    return strand, cf, cr


def _h_derep_x(eng, st, strand_both, minlen):
    """phase A of the exchange: dereplicate the shard, send every unique's tuple to the key's owner (key mod N)"""
    U = eng.derep(strand_both=strand_both, minseqlength=minlen)
    tup = np.zeros((max(U, 1), 4), np.int64)
    eng._chk(eng.L.itsx_unique_keys128(eng.h, C.c_uint64(KEY_SEEDS[0]), C.c_uint64(KEY_SEEDS[1]), int(st["base"]), tup.ctypes.data))
    tup = tup[:U]
    st["tup"] = tup
    N, r = st["world"], st["rank"]
    owner = (tup[:, 1].view(np.uint64) % np.uint64(N)).astype(np.int64) if U else np.zeros(0, np.int64)
    st["sent"] = []
    for d in range(N):
        idx = np.nonzero(owner == d)[0]
        st["sent"].append(idx)
        np.save(_xpath(st, "t", r, d), np.concatenate([tup[idx], idx[:, None]], axis=1))
    return U


def _h_own_x(eng, st):
    """phase B: the owner's step on this worker's share of the keys; the answers go back in the order the rows came"""
    N, d = st["world"], st["rank"]
    parts = []
    for r in range(N):
        p = _xpath(st, "t", r, d)
        parts.append(np.load(p))
        os.unlink(p)
    src = np.concatenate([np.full(a.shape[0], r, np.int64) for r, a in enumerate(parts)]) if parts else np.zeros(0, np.int64)
    recv = np.concatenate(parts) if parts else np.zeros((0, 5), np.int64)
    ans = owner_verdicts_native(recv, src)
    at = 0
    for r, a in enumerate(parts):
        np.save(_xpath(st, "v", d, r), ans[at:at + a.shape[0]])
        at += a.shape[0]
    return int(recv.shape[0])


def _h_verdict_x(eng, st):
    """phase C: the verdicts of this worker's uniques, collected from the owners; it scores what it was chosen for"""
    N, r = st["world"], st["rank"]
    U = eng.n_unique
    verdict = np.zeros((U, 4), np.int64)
    for d in range(N):
        p = _xpath(st, "v", d, r)
        verdict[st["sent"][d]] = np.load(p)
        os.unlink(p)
    st["sent"] = None
    n_act = _h_verdict(eng, st, verdict)
    seed, _ = eng.get_uniques()
    n_seeds = int((verdict[:, 0] == seed + st["base"]).sum()) if U else 0       # global first occurrences this shard holds
    return n_act, n_seeds


def _h_get_verdict(eng, st):
    return st["verdict"]


def _h_rows_pub(eng, st, left, right):
    """coordinates, step 1: the per-representative rows of this worker, where every worker can read them"""
    np.save(_xpath(st, "r", st["rank"], 0), np.stack(eng.rep_coords(left, right), axis=1).astype(np.int32))
    return None


def _h_rows_compose(eng, st, out_path, n_total):
    """coordinates, step 2: this shard's reads -> their local unique -> the scorer's row, written into the sample's shared array"""
    N = st["world"]
    v = st["verdict"]
    U = v.shape[0]
    urows = np.full((U + 1, 4), -1, np.int32)
    urows[:, 3] = 0                                       # row U: a read that belongs to no cluster
    for w in range(N):
        mine = np.nonzero(v[:, 2] == w)[0]
        if mine.shape[0]:
            rw = np.load(_xpath(st, "r", w, 0), mmap_mode="r")
            urows[mine] = rw[v[mine, 3]]
    uq = eng.get_derep()[2]
    g = np.where(uq >= 0, uq, U)
    for k in range(4):                                    # one file per column: the parent maps them as they are
        out = np.lib.format.open_memmap("%s.%d.npy" % (out_path, k), mode="r+")
        out[st["base"]:st["base"] + uq.shape[0]] = urows[g, k]
        out.flush()
        del out
    return int(uq.shape[0])


def _h_rows_done(eng, st):
    try:
        os.unlink(_xpath(st, "r", st["rank"], 0))
    except OSError:
        pass
    return None


def _h_names_pub(eng, st, path):
    blob, offs = eng.read_names_raw()
    np.save(path + ".b.npy", np.frombuffer(blob, np.uint8))
    np.save(path + ".o.npy", offs)
    return int(offs[-1])


def _h_set_reads(eng, st, blob, offs, names, base):
    eng.set_reads_buffer(blob, offs, names)
    st["base"] = int(base)
    return eng.n_reads


def _h_derep(eng, st, strand_both, minlen):
    U = eng.derep(strand_both=strand_both, minseqlength=minlen)
    tup = np.zeros((max(U, 1), 4), np.int64)
    eng._chk(eng.L.itsx_unique_keys128(eng.h, C.c_uint64(KEY_SEEDS[0]), C.c_uint64(KEY_SEEDS[1]), int(st["base"]), tup.ctypes.data))
    st["tup"] = tup[:U]
    return st["tup"]


def _h_verdict(eng, st, verdict):
    U = eng.n_unique
    lu = np.arange(U, dtype=np.int64)
    st["verdict"] = verdict
    active = (verdict[:, 2] == st["rank"]) & (verdict[:, 3] == lu)
    eng.set_active_uniques(active)
    return int(active.sum())


def _h_derep_arrays(eng, st, want_names, want_seqs):
    """per read: local unique number, orientation relative to the GLOBAL representative, length (+ labels); per local unique: its
    first occurrence (global index) and, when asked, its sequence"""
    rep_of, strand, uniq_of = eng.get_derep()
    v, tup = st["verdict"], st["tup"]
    flip = v[:, 1] != tup[:, 3]                          # this shard's seed is the reverse complement of the representative
    gstrand = strand.copy()
    ok = uniq_of >= 0
    gstrand[ok] = np.where(flip[uniq_of[ok]], -strand[ok], strand[ok])
    lens = np.zeros(eng.n_reads, np.int32)
    offs = np.zeros(eng.n_reads + 1, np.int64)
    eng._chk(eng.L.itsx_get_read_names(eng.h, None, 0, offs.ctypes.data))
    out = {"uniq_of": uniq_of.astype(np.int32), "strand": gstrand.astype(np.int8)}
    seed, _ = eng.get_uniques()
    out["seed_gidx_local"] = seed + st["base"]
    if want_names:
        out["names"] = eng.read_names_raw()
    # read lengths from the packed set: the derep arrays do not carry them, the unique sequences do; ask the library for all reads' lengths
    uo = np.zeros(eng.n_unique + 1, np.int64)
    eng._chk(eng.L.itsx_get_unique_seqs(eng.h, None, 0, uo.ctypes.data))
    ulen = np.diff(uo).astype(np.int32)
    lens[ok] = ulen[uniq_of[ok]]                         # a read has its unique's length (exact dereplication)
    out["len"] = lens
    if want_seqs:
        buf = C.create_string_buffer(int(uo[-1]) + 1)
        eng._chk(eng.L.itsx_get_unique_seqs(eng.h, buf, int(uo[-1]), uo.ctypes.data))
        out["useqs"] = (buf.raw[:int(uo[-1])], uo)
    return out


def _h_profiles(eng, st, path, text):
    n = eng.load_profiles(path=path, text=text)
    if st["rank"] != 0:
        return n, None
    names = eng.profile_names()
    M = np.zeros(n, np.int32)
    ev = np.zeros((n, 6), np.float32)
    for i in range(n):
        m = C.c_int32(0)
        eng._chk(eng.L.itsx_profile_params(eng.h, i, C.byref(m), ev[i].ctypes.data))
        M[i] = m.value
    return n, (names, M, ev)


def _h_search(eng, st, mode, T, F1, F2, F3):
    eng.set_rows_mode(mode)
    eng.search(T=T, F1=F1, F2=F2, F3=F3)
    return eng.get_domz()


def _h_finalize(eng, st, z, domE):
    eng.set_domz(z)
    eng.finalize(domE=domE)
    return eng.lazy_pending(), eng.lazy_pending_profiles()


def _h_complete(eng, st, flags):
    eng.lazy_complete(flags)
    return eng.get_domz()


def _h_rep_coords(eng, st, left, right):
    return np.stack(eng.rep_coords(left, right), axis=1).astype(np.int32)


def _h_uniq_of(eng, st):
    return eng.get_derep()[2].astype(np.int32, copy=False)


def _h_domains(eng, st):
    return eng.domains()


def _h_call(eng, st, name, args, kwargs):
    return getattr(eng, name)(*args, **kwargs)


def _h_stats(eng, st):
    return eng.stats()


_HANDLERS = {"job": _h_job, "load_piece": _h_load_piece, "load_range": _h_load_range, "merge_piece": _h_merge_piece, "set_base": _h_set_base, "orient_piece": _h_orient_piece,
             "derep_x": _h_derep_x, "own_x": _h_own_x, "verdict_x": _h_verdict_x, "get_verdict": _h_get_verdict,
             "rows_pub": _h_rows_pub, "rows_compose": _h_rows_compose, "rows_done": _h_rows_done, "names_pub": _h_names_pub,
             "load_shard": _h_load_shard, "set_reads": _h_set_reads, "derep": _h_derep, "verdict": _h_verdict,
             "derep_arrays": _h_derep_arrays, "profiles": _h_profiles, "search": _h_search, "finalize": _h_finalize,
             "complete": _h_complete, "rep_coords": _h_rep_coords, "uniq_of": _h_uniq_of, "domains": _h_domains, "call": _h_call, "stats": _h_stats}


# ---------------------------------------------------------------------------------------------------- the driver
class ShardedOps:
    """What a sample spread over several contexts has in common, whoever holds the contexts (MultiEngine: one worker process per
    GPU; itsxpress_amd.stream.StreamEngine: file-order chunks on one GPU): the global unique list, domZ summed before the
    thresholds, per-read coordinates and the file-compatible outputs composed from the contexts' arrays.  A subclass supplies
    `_each(cmd, args_per_shard)` -> one handler result per shard, `world`, `_verdicts`, `_bases`, `_nloc`."""

    def _all(self, cmd, *args):
        return self._each(cmd, [args] * self.world)

    def _index_uniques(self):
        """after the verdicts: the global unique list = distinct sequences in input order of their first occurrences"""
        verdict = np.concatenate(self._verdicts) if self._verdicts else np.zeros((0, 4), np.int64)
        self._seeds = np.unique(verdict[:, 0]) if verdict.shape[0] else np.zeros(0, np.int64)
        self._gmap = [np.searchsorted(self._seeds, v[:, 0]) for v in self._verdicts]        # local unique -> global unique
        self.n_unique = int(self._seeds.shape[0])
        self._derep = None
        self._final = False

    def _derep_arrays(self, names=True, seqs=False):
        if self._derep is None or (names and "names" not in self._derep[0]) or (seqs and "useqs" not in self._derep[0]):
            self._derep = self._all("derep_arrays", bool(names), bool(seqs))
        return self._derep

    def get_derep(self):
        """(rep_of, strand, uniq_of) per read of the WHOLE sample, as one Engine on the whole input reports them"""
        parts = self._derep_arrays(names=False)
        rep_of, strand, uniq_of = [], [], []
        for r, d in enumerate(parts):
            uq = d["uniq_of"].astype(np.int64)
            ok = uq >= 0
            g = np.where(ok, self._gmap[r][np.maximum(uq, 0)], -1) if self._gmap[r].shape[0] else np.full(uq.shape, -1, np.int64)
            uniq_of.append(g)
            rep_of.append(np.where(ok, self._seeds[np.maximum(g, 0)], -1) if self._seeds.shape[0] else np.full(uq.shape, -1, np.int64))
            strand.append(d["strand"])
        return np.concatenate(rep_of), np.concatenate(strand), np.concatenate(uniq_of)

    def read_names_raw(self):
        parts = self._derep_arrays(names=True)
        blobs = [d["names"][0] for d in parts]
        offs = [np.zeros(1, np.int64)]
        base = 0
        for d in parts:
            o = d["names"][1]
            offs.append(o[1:] + base)
            base += int(o[-1])
        return b"".join(blobs), np.concatenate(offs)

    def read_names(self):
        blob, offs = self.read_names_raw()
        blob = blob.decode()
        return [blob[offs[i]:offs[i + 1]] for i in range(self.n_reads)]

    def write_uc(self, path):
        self._write_derep(path, None)

    def write_rep_fasta(self, path):
        self._write_derep(None, path)

    def _write_derep(self, uc_path, rep_path):
        from . import _lib
        L = _lib.lib()
        parts = self._derep_arrays(names=True, seqs=rep_path is not None)
        rep_of, strand, _ = self.get_derep()
        lens = np.concatenate([d["len"] for d in parts]).astype(np.int32)
        nblob, noffs = self.read_names_raw()
        sb = so = None
        if rep_path is not None:                         # the representatives' sequences, in input order of the seeds
            chunks = [None] * self.n_unique
            for r, d in enumerate(parts):
                blob, uo = d["useqs"]
                is_seed = self._verdicts[r][:, 0] == d["seed_gidx_local"]      # this shard holds the global first occurrence
                for u in np.nonzero(is_seed)[0]:
                    chunks[int(self._gmap[r][u])] = blob[int(uo[u]):int(uo[u + 1])]
            so = np.zeros(self.n_unique + 1, np.int64)
            np.cumsum([len(c) for c in chunks], out=so[1:])
            sb = b"".join(chunks)
        rep_of = np.ascontiguousarray(rep_of, np.int64)
        strand = np.ascontiguousarray(strand, np.int8)
        rc = L.itsx_write_derep_arrays(os.fsencode(uc_path) if uc_path else None, os.fsencode(rep_path) if rep_path else None,
                                       self.n_reads, rep_of.ctypes.data, strand.ctypes.data, lens.ctypes.data,
                                       nblob, noffs.ctypes.data, sb, so.ctypes.data if so is not None else None, self.n_unique)
        if rc != 0:
            raise EngineError(rc, L.itsx_writers_last_error().decode())

    def profile_names(self):
        return list(self._pmeta[0])

    def set_rows_mode(self, mode):
        self._mode = mode
        self.rows_mode = {None: -1, "env": -1, "full": 0, "compact": 1, "lazy": 2}.get(mode, mode)

    def set_kept_rows(self, on=True):
        """after a "lazy" / "compact" search: domains() / write_domtbl() compose the rows the shards kept (Engine.set_kept_rows)"""
        self._all("call", "set_kept_rows", (bool(on),), {})

    def finalize(self, domE=10.0):
        import time
        t0 = time.perf_counter()
        z = np.sum(self._z, axis=0)
        res = self._all("finalize", z, float(domE))
        pend = max(int(r[0]) for r in res)
        self.finalize_s = {"thresholds": round(time.perf_counter() - t0, 3)}       # (where an exact finalize's time goes: scripts/file_run.py prints it)
        if pend > 0:                                     # rows that depend on the exact domZ: their profiles are counted on every shard
            flags = np.max([r[1] for r in res], axis=0).astype(np.int32)
            t1 = time.perf_counter()
            self._z = self._all("complete", flags)
            t2 = time.perf_counter()
            z = np.sum(self._z, axis=0)
            res = self._all("finalize", z, float(domE))
            self.finalize_s.update({"profiles_counted": int((flags != 0).sum()), "counting": round(t2 - t1, 3), "thresholds_again": round(time.perf_counter() - t2, 3)})
            if max(int(r[0]) for r in res) > 0:          # (a counted profile leaves nothing undecided; the safety net: everything in full)
                self._z = self._all("search", "compact", *self._search_args)
                z = np.sum(self._z, axis=0)
                self._all("finalize", z, float(domE))
        self._domz = z
        self._final = True

    def _rep_rows(self, left, right):
        rows = self._all("rep_coords", left, right)      # [U_i, 4] per shard, local uniques (meaningful where the shard scored)
        out = np.full((self.n_unique, 4), -1, np.int32)
        out[:, 3] = 0
        for r, v in enumerate(self._verdicts):
            mine = (v[:, 2] == r) & (v[:, 3] == np.arange(v.shape[0]))
            out[self._gmap[r][mine]] = rows[r][mine]
        return out

    def rep_coords(self, left, right):
        rows = self._rep_rows(left, right)
        return tuple(np.ascontiguousarray(rows[:, k]) for k in range(4))

    def trim_coords(self, left, right):
        """per READ of the whole sample: start, stop, tlen (-1 = None), in_ddict"""
        rows = self._rep_rows(left, right)
        nothing = np.array([[-1, -1, -1, 0]], np.int32)
        rows = np.concatenate([rows, nothing])            # row n_unique: a read that belongs to no cluster
        cols = [np.ascontiguousarray(rows[:, k]) for k in range(4)]
        out = [np.empty(self.n_reads, np.int32) for _ in range(4)]
        at = 0
        for r, uq in enumerate(self._all("uniq_of")):     # per shard: local unique of every read -> global unique -> its row
            g = np.where(uq >= 0, self._gmap[r][np.maximum(uq, 0)], self.n_unique) if self._gmap[r].shape[0] else np.full(uq.shape, self.n_unique, np.int64)
            for k in range(4):
                np.take(cols[k], g, out=out[k][at:at + uq.shape[0]])
            at += uq.shape[0]
        return tuple(out)

    def domains(self):
        """every shard's domain rows with `rep` = index into the GLOBAL unique list, in domtblout order"""
        parts = self._all("domains")
        rows = []
        for r, d in enumerate(parts):
            d = d.copy()
            d["rep"] = self._gmap[r][d["rep"]]
            rows.append(d)
        allr = np.concatenate(rows) if rows else np.zeros(0, DOMAIN_DTYPE)
        order = np.lexsort((allr["dom_idx"], allr["rep"], allr["prof"]))
        return allr[order]

    def write_domtbl(self, path):
        from . import _lib
        L = _lib.lib()
        rows = np.ascontiguousarray(self.domains())
        names, M, ev = self._pmeta
        pn = "".join(names).encode()
        po = np.zeros(len(names) + 1, np.int64)
        np.cumsum([len(x) for x in names], out=po[1:])
        tau = np.ascontiguousarray(ev[:, 4], np.float32)
        lam = np.ascontiguousarray(ev[:, 5], np.float32)
        M = np.ascontiguousarray(M, np.int32)
        # labels of the representatives = labels of the global first occurrences
        nblob, noffs = self.read_names_raw()
        tn = [nblob[int(noffs[g]):int(noffs[g + 1])] for g in self._seeds]
        to = np.zeros(len(tn) + 1, np.int64)
        np.cumsum([len(x) for x in tn], out=to[1:])
        tb = b"".join(tn)
        z = np.ascontiguousarray(self._domz[:self.n_profiles], np.int64)
        rc = L.itsx_write_domtbl_arrays(os.fsencode(path), rows.ctypes.data, rows.shape[0], self.n_unique, z.ctypes.data, self.n_profiles,
                                        pn, po.ctypes.data, M.ctypes.data, tau.ctypes.data, lam.ctypes.data, tb, to.ctypes.data)
        if rc != 0:
            raise EngineError(rc, L.itsx_writers_last_error().decode())

    def stats(self):
        return self._all("stats")


class MultiEngine(ShardedOps):
    """The part of Engine's interface the mirror classes use, over N single-GPU workers."""

    def __init__(self, n_gpus, devices=None):
        self.world = int(n_gpus)
        if self.world < 1:
            raise ValueError("ITSXPRESS_GPUS must be >= 1")
        self.devices = list(devices) if devices is not None else _devices_from_env(self.world)
        ctx = mp.get_context("spawn")                   # fresh interpreters: nothing of this process's state, no forked GPU context
        self.conns, self.procs = [], []
        for r in range(self.world):
            a, b = ctx.Pipe()
            p = ctx.Process(target=_worker_main, args=(b, self.devices[r], r, self.world), daemon=True)
            p.start()
            b.close()
            self.conns.append(a)
            self.procs.append(p)
        try:
            self._collect()
        except BaseException:
            self.close()
            raise
        self.n_reads = self.n_unique = self.n_profiles = 0
        self.n_samples = 1
        self.rows_mode = -1
        self._mode = None
        self._search_args = None
        self._final = False
        self._lazy_index = False
        self._verdicts_ = []
        self._seeds_ = np.zeros(0, np.int64)
        self._gmap_ = []
        self._last_merge = None
        self.parent_s, self.parent_own_s = {}, {}         # seconds inside each call / of them this process's own work (scripts/multi_run.py)
        # worker-to-worker exchanges: files named by this driver -- in memory (/dev/shm) while it has room for them, else in the temp
        # directory; ITSXPRESS_XDIR names another place (a container's /dev/shm is often 64 MB)
        self._xdir = None
        self._new_xdir(self._xbase(1 << 26))

    @staticmethod
    def _free_bytes(d):
        try:
            v = os.statvfs(d)
            return v.f_bavail * v.f_frsize
        except OSError:
            return 0

    def _xbase(self, need):
        """where the exchange files go: ITSXPRESS_XDIR if given, /dev/shm if it holds `need` bytes, else the temp directory"""
        env = os.environ.get("ITSXPRESS_XDIR")
        if env:
            if not (os.path.isdir(env) and os.access(env, os.W_OK)):
                raise EngineError(-2, "ITSXPRESS_XDIR=%s is not a writable directory" % env)
            return env
        if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) and self._free_bytes("/dev/shm") >= need:
            return "/dev/shm"
        return tempfile.gettempdir()

    def _new_xdir(self, base):
        old = self._xdir
        self._xdir = tempfile.mkdtemp(prefix="itsx_multi_%d_" % os.getpid(), dir=base)
        self._xprefix = os.path.join(self._xdir, "x")
        self._all("job", self._xprefix)
        if old:
            shutil.rmtree(old, ignore_errors=True)

    def _ensure_room(self, need):
        """the exchange directory must hold `need` more bytes: move it (memory -> temp directory) or say so, instead of a worker dying of
        SIGBUS on a full tmpfs"""
        if self._free_bytes(self._xdir) >= need:
            return
        base = self._xbase(need)
        if os.path.dirname(self._xdir) != base and self._free_bytes(base) >= need:
            self._new_xdir(base)
            return
        raise EngineError(-2, "the multi-GPU exchange directory %s has %.1f GB free, this sample needs %.1f GB: point ITSXPRESS_XDIR at a "
                              "directory with room (or enlarge /dev/shm)" % (self._xdir, self._free_bytes(self._xdir) / 1e9, need / 1e9))

    def _sweep(self):
        """a failed exchange leaves its files behind: remove what the current job wrote"""
        for f in glob.glob(self._xprefix + "_*"):
            try:
                os.unlink(f)
            except OSError:
                pass

    def _tic(self):
        return (time.perf_counter(), getattr(self, "wait_s", 0.0))

    def _timed(self, name, t0):
        """wall time of a call, and the part of it that was this process's OWN work (the rest: waiting for the workers)"""
        dt = time.perf_counter() - t0[0]
        w = getattr(self, "wait_s", 0.0) - t0[1]
        self.parent_s[name] = self.parent_s.get(name, 0.0) + dt
        self.parent_own_s[name] = self.parent_own_s.get(name, 0.0) + max(0.0, dt - w)

    # -- the global unique list: built when a file-compatible writer / get_derep asks, never on the coordinates-only path
    def _build_index(self):
        if not self._lazy_index:
            return
        self._lazy_index = False
        t0 = self._tic()
        self._verdicts_ = self._all("get_verdict")
        keep = (self._derep, self._final, self.n_unique)
        ShardedOps._index_uniques(self)
        assert self.n_unique == keep[2], (self.n_unique, keep[2])
        self._derep, self._final = keep[0], keep[1]
        self._timed("index_uniques", t0)

    @property
    def _verdicts(self):
        self._build_index()
        return self._verdicts_

    @_verdicts.setter
    def _verdicts(self, v):
        self._verdicts_ = v

    @property
    def _seeds(self):
        self._build_index()
        return self._seeds_

    @_seeds.setter
    def _seeds(self, v):
        self._seeds_ = v

    @property
    def _gmap(self):
        self._build_index()
        return self._gmap_

    @_gmap.setter
    def _gmap(self, v):
        self._gmap_ = v

    # -- plumbing
    def _send(self, cmd, args_per_worker):
        for c, a in zip(self.conns, args_per_worker):
            c.send((cmd, a))

    def _collect(self):
        out, err = [], None
        for r, c in enumerate(self.conns):
            try:
                tag, val = c.recv()
            except EOFError:
                tag, val = "err", ("EOFError", -4, "worker %d (GPU %s) died" % (r, self.devices[r]))
            if tag == "err" and err is None:
                err = val
            out.append(val)
        if err is not None:                              # every worker has answered: nobody is left waiting in a half-done exchange
            name, code, msg = err
            if name == "FileNotFoundError":
                raise FileNotFoundError(msg)
            raise EngineError(code, msg)
        return out

    def _each(self, cmd, args_per_worker):
        t0 = time.perf_counter()
        self._send(cmd, args_per_worker)
        try:
            return self._collect()
        finally:                                          # time this process spent waiting for its workers (not its own work)
            self.wait_s = getattr(self, "wait_s", 0.0) + (time.perf_counter() - t0)

    def _w0(self, name, *args, **kwargs):
        self.conns[0].send(("call", (name, args, kwargs)))
        tag, val = self.conns[0].recv()
        if tag == "err":
            if val[0] == "FileNotFoundError":
                raise FileNotFoundError(val[2])
            raise EngineError(val[1], val[2])
        return val

    def close(self):
        for c in getattr(self, "conns", []):
            try:
                c.send(("close", None))
            except Exception:
                pass
        for p in getattr(self, "procs", []):
            p.join(timeout=20)
            if p.is_alive():
                p.kill()                                  # this exact child, nothing else
        self.conns, self.procs = [], []
        xd = getattr(self, "_xdir", None)
        if xd and os.path.isdir(xd):
            import shutil
            shutil.rmtree(xd, ignore_errors=True)
            self._xdir = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reads
    def _shard(self, path, tag, match=None):
        """the file's text in one piece per worker (csrc/shard_host.cpp): piece paths, records per piece"""
        from . import _lib
        L = _lib.lib()
        rec = np.zeros(self.world, np.int64)
        # the pieces are the inflated text: a .gz / .zst file is taken at eight times its size (FASTQ deflates ~4-5 x), anything else at its own
        size = os.path.getsize(path)
        self._ensure_room(int(size * (8 if path.endswith((".gz", ".zst")) else 1.05)) + (1 << 20))
        pre = os.path.join(self._xdir, tag)
        m = None if match is None else np.ascontiguousarray(match, np.int64)
        rc = L.itsx_shard_text(os.fsencode(path), self.world, None if m is None else m.ctypes.data, os.fsencode(pre), rec.ctypes.data, None)
        L.itsx_io_cache_clear()                              # (the parent keeps no copy of the text: the pieces are it)
        if rc != 0:
            self._sweep()
            raise EngineError(rc, L.itsx_shard_last_error().decode())
        return ["%s.%d" % (pre, r) for r in range(self.world)], rec

    def load_reads_file(self, path):
        """The reference reads the whole file before anything else starts (itsxpress/main.py:295-330).  Here the parent inflates it ONCE
        and hands every worker its piece as soon as that part of the text is final: worker 0 parses, uploads and packs while the pieces
        of workers 1 .. N - 1 are still being inflated (round 5 cut the pieces after the last byte: 1.6-2.8 s in which no worker had
        anything to do).  The pieces are files in the exchange directory, written by the I/O pool (itsx_write_range); a shared MAPPING of
        one file for all workers (itsx_stream_open_shared) was measured first and is slower -- 2.3 M page faults of 4 KB under the
        inflater's threads: 4.7 s instead of 1.5 for 9 GB."""
        if not os.path.exists(path):
            raise FileNotFoundError(path)
        if os.environ.get("ITSX_MULTI_LOAD", "stream") != "pieces":
            return self._load_streamed(path)
        t0 = self._tic()
        pieces, rec = self._shard(path, "reads")
        base = np.concatenate([[0], np.cumsum(rec)])
        self._timed("load: inflate + cut", t0)
        self._each("load_piece", [(pieces[r], int(base[r]), int(rec[r])) for r in range(self.world)])
        self.n_reads = int(base[-1])
        self._bases = [int(b) for b in base[:-1]]
        self._nloc = [int(x) for x in rec]
        self._derep = None
        self._final = False
        self._last_merge = None
        return self.n_reads

    def _load_streamed(self, path):
        from . import _lib
        L = _lib.lib()
        t0 = self._tic()
        size = os.path.getsize(path)
        self._ensure_room(int(size * (8 if path.endswith((".gz", ".zst")) else 1.05)) + (1 << 20))
        h = C.c_void_p()
        rc = L.itsx_stream_open(os.fsencode(path), C.byref(h))
        if rc != 0:
            raise EngineError(rc, L.itsx_stream_last_error().decode())
        N = self.world
        sent, t_first = 0, None
        try:
            ptr, nb, lst = C.c_void_p(), C.c_int64(0), C.c_int32(0)
            last = False

            def nxt(min_bytes):
                rc = L.itsx_stream_next(h, int(max(1, min_bytes)), C.byref(ptr), C.byref(nb), C.byref(lst))
                if rc != 0:
                    raise EngineError(rc, L.itsx_stream_last_error().decode())
                return (ptr.value or 0), nb.value, bool(lst.value)

            def estimate():
                a, c, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
                L.itsx_stream_progress(h, C.byref(a), C.byref(c), C.byref(r))
                return int(a.value * (r.value / c.value)) if c.value > 0 else 0

            done_bytes = 0
            for r in range(N):
                p0, got = 0, 0                               # the piece: [p0, p0 + got) of the text (slices are consecutive)
                if not last:
                    if r == N - 1:
                        while not last:                      # the rest of the file
                            q, n1, last = nxt(1 << 40)
                            p0 = p0 or q
                            got += n1
                    else:
                        if done_bytes == 0:                  # a first, small slice: after it the text's final size can be estimated
                            q, n1, last = nxt(16 << 20)
                            p0 = p0 or q
                            got += n1
                        while not last:
                            total = estimate()
                            want = (total - done_bytes) // (N - r) if total > 0 else (64 << 20)
                            if got >= want - (want >> 3):
                                break
                            q, n1, last = nxt(max(1 << 20, min(want - got, 256 << 20)))   # (next() hands out up to 1.5 x what is asked for)
                            p0 = p0 or q
                            got += n1
                    done_bytes += got
                piece = os.path.join(self._xdir, "reads.%d" % r)
                rc = L.itsx_write_range(os.fsencode(piece), C.c_void_p(p0), int(got))
                if rc != 0:
                    raise EngineError(rc, L.itsx_shard_last_error().decode())
                if t_first is None:
                    t_first = time.perf_counter() - t0[0]
                self.conns[r].send(("load_piece", (piece, 0, -1)))
                sent += 1
            self._timed("load: inflate + deal pieces (workers already loading)", t0)
            sent = 0                                         # (from here on _collect takes every worker's answer, errors included)
            tw = time.perf_counter()
            try:
                res = self._collect()
            finally:
                self.wait_s = getattr(self, "wait_s", 0.0) + (time.perf_counter() - tw)
        except BaseException:
            for r in range(sent):                            # (drain what the workers still answer, so that the pipes stay in step)
                try:
                    self.conns[r].recv()
                except Exception:
                    pass
            L.itsx_stream_close(h, 0)
            self._sweep()
            for f in glob.glob(os.path.join(self._xdir, "reads.*")):
                self._sweep_file(f)
            raise
        L.itsx_stream_close(h, 0)
        rec = np.asarray([int(x) for x in res], np.int64)
        base = np.concatenate([[0], np.cumsum(rec)])
        self._each("set_base", [(int(base[r]),) for r in range(N)])
        self.first_worker_busy_s = t_first
        self.n_reads = int(base[-1])
        self._bases = [int(b) for b in base[:-1]]
        self._nloc = [int(x) for x in rec]
        self._derep = None
        self._final = False
        self._last_merge = None
        return self.n_reads

    @staticmethod
    def _sweep_file(p):
        try:
            os.unlink(p)
        except OSError:
            pass

    def set_reads(self, seqs, names=None):
        n = len(seqs)
        args = []
        self._bases, self._nloc = [], []
        for r in range(self.world):
            lo, hi = n * r // self.world, n * (r + 1) // self.world
            part = seqs[lo:hi]
            lens = np.fromiter((len(s) for s in part), np.int64, hi - lo)
            offs = np.zeros(hi - lo + 1, np.int64)
            np.cumsum(lens, out=offs[1:])
            blob = ("".join(part)).encode() if (part and isinstance(part[0], str)) else b"".join(part)
            args.append((blob, offs, None if names is None else list(names[lo:hi]), lo))
            self._bases.append(lo)
            self._nloc.append(hi - lo)
        self._send("set_reads", args)
        self._collect()
        self.n_reads = n
        self._derep = None
        self._final = False
        self._last_merge = None
        self._lazy_index = False
        return n

    # -- a1: exact dereplication of the whole sample
    def derep(self, strand_both=True, minseqlength=1):
        """exact dereplication of the whole sample: local derep on every GPU, then the uniques meet at their key's owner (key mod N),
        every worker sorts its Nth of the keys, the verdicts travel back -- three commands, nothing of the data's size in this process"""
        t0 = self._tic()
        self._ensure_room(48 * max(1, self.n_reads) + (1 << 20))      # the keys travel as 32 B per unique, the verdicts as 12
        try:
            self._all("derep_x", bool(strand_both), int(minseqlength))
            self._all("own_x")
            res = self._all("verdict_x")
        except BaseException:
            self._sweep()
            raise
        self.n_unique = int(sum(r[1] for r in res))
        self._lazy_index = True                          # seeds / local -> global maps: only if somebody asks
        self._derep = None
        self._final = False
        self._timed("derep (parent waits for the workers)", t0)
        return self.n_unique

    def cluster(self, cluster_id, strand_both=True):
        if float(cluster_id) >= 1.0:
            return self.derep(strand_both=strand_both, minseqlength=1)     # main.py:534-537: 1.0 is exact dereplication
        raise EngineError(-5, "greedy clustering (cluster_id < 1) is sequential by definition and does not shard over GPUs: "
                              "run it with ITSXPRESS_GPUS=1 (DESIGN.md section 7)")

    # -- a3 / a4
    def load_profiles(self, path=None, text=None):
        if path is not None and not os.path.exists(path):
            raise FileNotFoundError(path)
        res = self._all("profiles", path, text)
        self.n_profiles = int(res[0][0])
        self._pmeta = res[0][1]
        self._final = False
        return self.n_profiles

    def search(self, T=10.0, F1=1e-6, F2=1e-6, F3=1e-6):
        self._search_args = (T, F1, F2, F3)
        self._z = self._all("search", self._mode, T, F1, F2, F3)
        self._final = False

    # -- coordinates per read: composed in the workers, into one array in shared memory
    def trim_coords(self, left, right):
        """per READ of the whole sample: start, stop, tlen (-1 = None), in_ddict"""
        t0 = self._tic()
        path = self._xprefix + "_coords"
        self._ensure_room(16 * self.n_reads + 32 * max(1, self.n_unique) + (1 << 20))
        try:
            for k in range(4):
                out = np.lib.format.open_memmap("%s.%d.npy" % (path, k), mode="w+", dtype=np.int32, shape=(self.n_reads,))
                del out
                # (a memmap file is sparse: reserve its blocks now, so that a full file system is an error here and not a SIGBUS in a worker)
                fd = os.open("%s.%d.npy" % (path, k), os.O_RDWR)
                try:
                    if self.n_reads:
                        os.posix_fallocate(fd, 0, os.fstat(fd).st_size)
                finally:
                    os.close(fd)
            self._all("rows_pub", left, right)
            self._all("rows_compose", path, self.n_reads)
            self._all("rows_done")
            res = []
            for k in range(4):                                # private (copy-on-write) mappings of what the workers wrote: no copy here
                p = "%s.%d.npy" % (path, k)
                res.append(np.load(p, mmap_mode="c") if self.n_reads else np.zeros(0, np.int32))
                os.unlink(p)
        except BaseException:
            self._sweep()
            raise
        self._timed("trim_coords", t0)
        return tuple(res)

    def read_names_raw(self):
        t0 = self._tic()
        paths = [self._xprefix + "_names_%d" % r for r in range(self.world)]
        self._each("names_pub", [(p,) for p in paths])
        blobs, offs, base = [], [np.zeros(1, np.int64)], 0
        for p in paths:
            b, o = np.load(p + ".b.npy"), np.load(p + ".o.npy")
            blobs.append(b.tobytes())
            offs.append(o[1:] + base)
            base += int(o[-1])
            os.unlink(p + ".b.npy")
            os.unlink(p + ".o.npy")
        self._timed("read_names_raw", t0)
        return b"".join(blobs), np.concatenate(offs)

    # -- either side of the path, sharded by record range like the reads: orientation of CCS reads, paired-end merging
    def orient_load_db(self, fasta_path):
        if not os.path.exists(fasta_path):
            raise FileNotFoundError(fasta_path)
        self._orient_db = fasta_path
        return 0

    def orient_file(self, fastq):
        if not os.path.exists(fastq):
            raise FileNotFoundError(fastq)
        pieces, rec = self._shard(fastq, "orient")
        res = self._each("orient_piece", [(pieces[r], self._orient_db) for r in range(self.world)])
        return tuple(np.concatenate([r[k] for r in res]) for k in range(3))

    def orient_profiles(self, F1=1e-6):
        raise EngineError(-5, "orientation by the profiles (orient_profiles) does not shard over GPUs: run it with ITSXPRESS_GPUS=1 "
                              "(DESIGN.md section 9)")

    def orient_profiles_apply(self, F1=1e-6):
        raise EngineError(-5, "orientation by the profiles (orient_profiles_apply) does not shard over GPUs: run it with ITSXPRESS_GPUS=1 "
                              "(DESIGN.md section 9)")

    def trimmed_table(self, region_prefixes=None, start=None, stop=None, min_len=1):
        raise EngineError(-5, "the feature table of the trimmed regions (trimmed_table) does not shard over GPUs: run it with ITSXPRESS_GPUS=1 "
                              "(DESIGN.md section 8)")

    def denoise_table(self, alpha=2.0, minsize=8, max_diffs=None, max_skew=None):
        raise EngineError(-5, "denoising the feature table (denoise_table) does not shard over GPUs: run it with ITSXPRESS_GPUS=1 "
                              "(DESIGN.md section 8)")

    def _merge(self, r1, r2, out, maxdiffs, maxee, allow_stagger):
        for p in (r1, r2):
            if not os.path.exists(p):
                raise FileNotFoundError(p)
        t0 = self._tic()
        p1, rec = self._shard(r1, "r1")
        p2, _ = self._shard(r2, "r2", match=rec)           # R2 cut where R1 was: the same pairs on every worker
        self._timed("merge: inflate + cut", t0)
        outs = [None if out is None else "%s_merged.%d" % (self._xprefix, r) for r in range(self.world)]
        res = self._each("merge_piece", [(p1[r], p2[r], outs[r], int(maxdiffs), float(maxee), bool(allow_stagger), self.merge_join) for r in range(self.world)])
        self.n_joined = int(sum(x[2] for x in res))          # (merge_join: every worker's reads are its merged and its joined pairs)
        self._merged_only = int(sum(x[1] for x in res))
        return int(sum(x[0] for x in res)), [int(x[1]) + int(x[2]) for x in res], outs

    # Whether the workers' merges keep the pairs whose mates do not overlap as joined reads (Engine.merge_join): handed to every worker
    # with its piece.  The counts the merge calls return stay those of the merged pairs; n_reads and n_joined tell the rest.
    @property
    def merge_join(self):
        return getattr(self, "_merge_join", False)

    @merge_join.setter
    def merge_join(self, on):
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("MultiEngine.merge_join is False or True, not %r" % (on,))
        self._merge_join = bool(on)

    def merge_pairs_load(self, r1, r2, maxdiffs=40, maxee=2.0, allow_stagger=False):
        """merge R1 / R2 on every worker's piece; the merged reads are the workers' read sets (nothing written): (pairs, merged)"""
        n, ms, _ = self._merge(r1, r2, None, maxdiffs, maxee, allow_stagger)
        base = np.concatenate([[0], np.cumsum(ms)])
        self._each("set_base", [(int(base[r]),) for r in range(self.world)])
        self.n_reads = int(base[-1])
        self._bases, self._nloc = [int(b) for b in base[:-1]], ms
        self._derep = None
        self._final = False
        self._last_merge = dict(r1=r1, r2=r2, maxdiffs=int(maxdiffs), maxee=float(maxee), allow_stagger=bool(allow_stagger), join=self.merge_join)
        return n, self._merged_only

    def merge_pairs_files(self, r1, r2, out, maxdiffs=40, maxee=2.0, allow_stagger=False):
        """the merged reads as ONE file (seq.fq): every worker merges its piece, the pieces are joined in order"""
        n, ms, outs = self._merge(r1, r2, out, maxdiffs, maxee, allow_stagger)
        with open(out, "wb") as f:
            for p in outs:
                with open(p, "rb") as g:
                    while True:
                        b = g.read(64 << 20)
                        if not b:
                            break
                        f.write(b)
                os.unlink(p)
        return n, self._merged_only

    def write_merged_fastq(self, path):
        lm = self._last_merge
        if lm is None:
            raise EngineError(-1, "write_merged_fastq: this engine's reads do not come from merge_pairs_load")
        # (the same merge once more, into files this time: itsx_merge_pairs_files leaves a context's read set and results alone)
        keep, self.merge_join = self.merge_join, bool(lm.get("join", False))      # the same merge: joined records too, where the reads hold them
        try:
            n, m = self.merge_pairs_files(lm["r1"], lm["r2"], path, maxdiffs=lm["maxdiffs"], maxee=lm["maxee"], allow_stagger=lm["allow_stagger"])
            m += self.n_joined
        finally:
            self.merge_join = keep
        if m != self.n_reads:
            raise EngineError(-1, "write_merged_fastq: %d merged records written, the engines hold %d" % (m, self.n_reads))
        return m


def _devices_from_env(n):
    """ITSXPRESS_GPU_IDS="0,2,5" names the devices; otherwise 0..N-1.  (A one-GPU box may rehearse N workers on device 0 with
    ITSXPRESS_GPU_IDS="0,0".)"""
    ids = os.environ.get("ITSXPRESS_GPU_IDS", "").strip()
    if ids:
        d = [int(x) for x in ids.split(",") if x.strip() != ""]
        if len(d) != n:
            raise ValueError("ITSXPRESS_GPU_IDS names %d devices, ITSXPRESS_GPUS asks for %d" % (len(d), n))
        return d
    return list(range(n))


def gpus_from_env():
    v = os.environ.get("ITSXPRESS_GPUS", "").strip()
    return int(v) if v else 1
