"""CPU checks of greedy clustering over several GPUs (itsx_cluster_multi): the C ABI declares and exports the entry point, and
SeqSample.cluster routes a sample with ITSXPRESS_GPUS > 1 at cluster_id < 1 to a leader Engine plus helper Engines on the named
devices (recorded by a fake Engine: no GPU is touched)."""
import importlib
import os

import pytest

from itsxpress_amd import _lib

ss = importlib.import_module("itsxpress_amd.SeqSample")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_and_exports_cluster_multi():
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        hdr = f.read()
    assert ("int itsx_cluster_multi(itsx_ctx *ctx, itsx_ctx *const *helpers, int32_t n_helpers, double id, int strand_both, "
            "int64_t *n_unique);") in hdr
    assert "itsx_cluster_multi" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "itsx_cluster_multi")


class _Log:
    def __init__(self):
        self.events = []


class _FakeEngine:
    log = None

    def __init__(self, device=None):
        self.device = device
        self.world = 1
        self.closed = False
        self.log.events.append(("open", device, self))

    def load_reads_file(self, path):
        self.log.events.append(("load", self.device, path))

    def cluster(self, cid, strand_both=True, **kw):
        helpers = kw.get("helpers")
        self.log.events.append(("cluster", self.device, cid, None if helpers is None else [h.device for h in helpers]))
        assert all(not h.closed for h in helpers or [])
        return 1

    def derep(self, **kw):
        return 1

    def write_uc(self, path):
        self.log.events.append(("write_uc", self.device))

    def write_rep_fasta(self, path):
        self.log.events.append(("write_rep", self.device))

    def close(self):
        self.closed = True
        self.log.events.append(("close", self.device))


class _FakeWorkers(_FakeEngine):
    def __init__(self, world):
        super().__init__("workers")
        self.world = world


@pytest.fixture
def fake(monkeypatch, tmp_path):
    log = _Log()
    monkeypatch.setattr(_FakeEngine, "log", log)
    monkeypatch.setattr(ss, "Engine", _FakeEngine)
    for k in ("ITSXPRESS_GPU_IDS", "ITSXPRESS_CLUSTER_GPUS", "ITSXPRESS_GPUS", "ITSXPRESS_ARRAYS", "ITSXPRESS_STREAM"):
        monkeypatch.delenv(k, raising=False)

    def make(world):
        s = ss.SeqSample(str(tmp_path / "reads.fq"), str(tmp_path))
        s.seq_file = str(tmp_path / "reads.fq")
        s.fast = False
        s._engine = _FakeWorkers(world)
        return s
    return log, make


def test_three_gpus_cluster_with_a_leader_and_two_helpers(fake, monkeypatch):
    log, make = fake
    monkeypatch.setenv("ITSXPRESS_GPU_IDS", "4,1,7")
    s = make(3)
    s.cluster(threads=1, cluster_id=0.995)
    ev = log.events
    assert ("close", "workers") in ev
    opened = [e[1] for e in ev if e[0] == "open" and e[1] != "workers"]
    assert opened == [4, 1, 7]
    clusters = [e for e in ev if e[0] == "cluster"]
    assert clusters == [("cluster", 4, 0.995, [1, 7])]
    assert ("load", 4, s.seq_file) in ev
    # the helpers are closed once the call returns; the leader stays for _search
    assert ("close", 1) in ev and ("close", 7) in ev and ("close", 4) not in ev
    assert ev.index(("close", 1)) > ev.index(clusters[0])
    assert s.engine.device == 4 and not s.engine.closed
    assert ("write_uc", 4) in ev and ("write_rep", 4) in ev


def test_cluster_gpus_one_keeps_the_one_gpu_route(fake, monkeypatch):
    log, make = fake
    monkeypatch.setenv("ITSXPRESS_GPU_IDS", "0,1,2")
    monkeypatch.setenv("ITSXPRESS_CLUSTER_GPUS", "1")
    s = make(3)
    s.cluster(threads=1, cluster_id=0.99)
    ev = log.events
    opened = [e[1] for e in ev if e[0] == "open" and e[1] != "workers"]
    assert opened == [None]                                  # Engine(): today's device choice
    assert [e for e in ev if e[0] == "cluster"] == [("cluster", None, 0.99, None)]


def test_cluster_gpus_limits_the_helpers(fake, monkeypatch):
    log, make = fake
    monkeypatch.setenv("ITSXPRESS_GPU_IDS", "0,0,0,0")
    monkeypatch.setenv("ITSXPRESS_CLUSTER_GPUS", "2")
    s = make(4)
    s.cluster(threads=1, cluster_id=0.99)
    assert [e for e in log.events if e[0] == "cluster"] == [("cluster", 0, 0.99, [0])]


def test_cluster_id_one_stays_on_the_workers(fake, monkeypatch):
    log, make = fake
    monkeypatch.setenv("ITSXPRESS_GPU_IDS", "0,1")
    s = make(2)
    s.cluster(threads=1, cluster_id=1.0)
    ev = log.events
    assert [e for e in ev if e[0] == "cluster"] == [("cluster", "workers", 1.0, None)]
    assert ("close", "workers") not in ev


def test_one_gpu_is_unchanged(fake):
    log, make = fake
    s = make(1)
    s.cluster(threads=1, cluster_id=0.97)
    ev = log.events
    assert [e for e in ev if e[0] == "cluster"] == [("cluster", "workers", 0.97, None)]
    assert [e for e in ev if e[0] == "open"] == [("open", "workers", s.engine)]
