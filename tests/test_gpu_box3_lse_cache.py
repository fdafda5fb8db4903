"""K53 under the version-keyed cache audit of tests/test_gpu_cache_coherence.py: ops._Box3Lse.backward leaves max|G| for T's node with
_remember_amax, as ops._Box3SoftmaxWarp.backward does, so it is a producer site of that audit.  The workload — a row pass and a
transposed pass of ops.box3_lse over one T with one Box3GradSink — runs through that file's three arms (cached, caches off, cached
again: bitwise equal) on its audit object.  Without this file tests/test_gpu_cache_coherence.py::test_every_site_was_reached fails
("_remember_amax sites no workload reached: _Box3Lse.backward"): that audit counts every _remember_amax site of ops.py, and its own
workloads cannot know the new one.

The file name sorts before test_gpu_cache_coherence.py: the site has been reached when that file's "every site was reached" runs."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_cache_coherence as cc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(hip_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no GPU is visible (the HIP path has no fallback)")


def test_box3_lse_pair_with_one_sink_and_two_passes(monkeypatch):
    """the second pass's backward ADDS into the first one's G and replaces its max|G| cell; T's node finds the cell of the sum"""
    from cocosnet_amd import ops
    for name in ("PRECISION", "PROJ_PRECISION", "CONV_PRECISION"):
        monkeypatch.setattr(ops, name, "f16x3")
    B, fh, fw, kc, scale = 1, 4, 64, 256.0 * 9, 100.0

    def workload():
        g = torch.Generator(device=cc.DEV).manual_seed(153)
        q = (cc._rand(g, B, 256, fh, fw) + 0.15).requires_grad_(True)
        k = (0.05 * q.detach().roll((1, 5), (2, 3)) + cc._rand(g, B, 256, fh, fw) - 0.1).requires_grad_(True)
        (mu, a), (nu, b) = ops.unfold3_stats(q, kc), ops.unfold3_stats(k, kc)
        sink = ops.Box3GradSink()
        T = ops.box3_corr_xbox(q, k, sink)
        rows = ops.box3_lse(T, mu, a, nu, b, fh, fw, kc, scale, False, sink)
        cols = ops.box3_lse(T, nu, b, mu, a, fh, fw, kc, scale, True, sink)
        return [rows, cols], [q, k]
    cc._three_arms(workload, monkeypatch, "box3 lse pair")
    site = [s for s in cc._audit().uncovered_producers() if "_Box3Lse" in cc._audit().label(s)]
    assert not site, "the audit did not see _Box3Lse.backward's _remember_amax"
