"""K42 inside red zones, collected with the other match-readout files BEFORE tests/test_gpu_red_zones.py: that file's "every entry
point was reached" audit counts every `cocos_*` name cocosnet_amd/ops.py hands to `_lib.call`, and it only knows the cases that ran
before it.  The case itself (forward + backward of ops.sparse_softmax_warp under tests/guarded_alloc.guarded) is
tests/test_gpu_sparse_warp.py's, which also runs it with the rest of K42's tests."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_sparse_warp as sw  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sw.RZ_CASES))
def test_sparse_warp_inside_red_zones(name, monkeypatch, hip_lib):
    sw.test_op_inside_red_zones(name, monkeypatch)
