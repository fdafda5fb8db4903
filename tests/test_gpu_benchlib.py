"""tools/benchlib.py on the device: the event timing and the peak reading, on a framework op (no kernel of the project runs here)."""
import math
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import benchlib  # noqa: E402

pytestmark = pytest.mark.gpu
MIB = 2 ** 20


def test_time_calls_and_peak_bytes_on_a_fill():
    fill = lambda: torch.empty(MIB, dtype=torch.uint8, device="cuda").fill_(1)
    ms = benchlib.time_calls(fill, 10)
    assert math.isfinite(ms) and ms > 0
    peak = benchlib.peak_bytes(fill)
    assert MIB <= peak < 4 * MIB
