"""CPU checks of the batched greedy clustering's interface: SampleBatch.cluster_per_sample takes SeqSample.cluster's
leading arguments, and the C ABI declares and exports itsx_cluster_samples."""
import inspect
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cluster_per_sample_takes_seqsample_cluster_arguments():
    from itsxpress_amd.SeqSample import SeqSample
    from itsxpress_amd.batch import SampleBatch
    mine = inspect.signature(SampleBatch.cluster_per_sample).parameters
    ref = inspect.signature(SeqSample.cluster).parameters
    assert list(mine)[: len(ref)] == list(ref)
    for k in ref:
        assert mine[k].default == ref[k].default and mine[k].annotation == ref[k].annotation


def test_abi_declares_and_exports_cluster_samples():
    from itsxpress_amd import _lib
    with open(os.path.join(ROOT, "include", "itsx_hip.h")) as f:
        hdr = f.read()
    assert "int itsx_cluster_samples(itsx_ctx *ctx, double id, int strand_both, int64_t *n_unique);" in hdr
    assert "itsx_cluster_samples" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "itsx_cluster_samples")
