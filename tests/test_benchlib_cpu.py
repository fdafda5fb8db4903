"""tools/benchlib.py without a device: the window arithmetic, the alternation, the summary, the parser of hipcc's kernel-resource-usage
remarks and the shared argument block.  The device is never touched: time_calls is replaced by a fake wherever a function would call it."""
import argparse
import os
import sys
from types import SimpleNamespace

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import benchlib  # noqa: E402

# hipcc --offload-arch=gfx950 --cuda-device-only -Rpass-analysis=kernel-resource-usage on csrc/corr_topk_f16x3.hip, recorded once and
# trimmed to two `Function Name:` blocks (the directory of the header cut from every line)
REMARKS = """\
In file included from corr_topk_f16x3.hip:4:
corr_topk_kernel.h:162:1: remark: Function Name: _ZN5cocos22corr_topk_f16x3_kernelILi1ELb0ELb0ELb0EEEvPKDF16_S2_S2_S2_PKiS4_PiPfS6_iiiiffmS6_PKff [-Rpass-analysis=kernel-resource-usage]
  162 |     float* __restrict__ col_ws = nullptr, const float* __restrict__ k_bias = nullptr, float bias_raw = 0.f /* operand_scale^2 / inv_temperature */) {
      | ^
corr_topk_kernel.h:162:1: remark:     TotalSGPRs: 64 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     VGPRs: 227 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark: Function Name: _ZN5cocos22corr_topk_f16x3_kernelILi8ELb1ELb0ELb0EEEvPKDF16_S2_S2_S2_PKiS4_PiPfS6_iiiiffmS6_PKff [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     TotalSGPRs: 70 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     VGPRs: 245 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     AGPRs: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     Dynamic Stack: False [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]
corr_topk_kernel.h:162:1: remark:     LDS Size [bytes/block]: 0 [-Rpass-analysis=kernel-resource-usage]
"""
K1 = "_ZN5cocos22corr_topk_f16x3_kernelILi1ELb0ELb0ELb0EEEvPKDF16_S2_S2_S2_PKiS4_PiPfS6_iiiiffmS6_PKff"
K8 = "_ZN5cocos22corr_topk_f16x3_kernelILi8ELb1ELb0ELb0EEEvPKDF16_S2_S2_S2_PKiS4_PiPfS6_iiiiffmS6_PKff"


@pytest.fixture
def no_device(monkeypatch):
    """window_counts synchronises after the warm-up: without a device that is a no-op here"""
    monkeypatch.setattr(benchlib.torch.cuda, "synchronize", lambda: None)


@pytest.mark.parametrize("ms_per_call, want", [(0.01, 5000), (1e4, 2), (0.0, 50000)])
def test_window_counts_arithmetic(monkeypatch, no_device, ms_per_call, want):
    """0.05 s of calls of 0.01 ms are 5000; a call longer than the window keeps the floor of 2; a zero time is taken as 1e-3 ms"""
    probes, warmups = [], []
    monkeypatch.setattr(benchlib, "time_calls", lambda fn, n: (probes.append(n), ms_per_call)[1])
    counts = benchlib.window_counts({"a": lambda: warmups.append("a"), "b": lambda: warmups.append("b")}, 0.05, 3)
    assert counts == {"a": want, "b": want}
    assert probes == [2, 2] and warmups == ["a"] * 3 + ["b"] * 3


def test_window_counts_probe_is_the_floor(monkeypatch, no_device):
    monkeypatch.setattr(benchlib, "time_calls", lambda fn, n: 1e4)
    assert benchlib.window_counts({"a": lambda: None}, 0.2, 0, probe=3) == {"a": 3}


def test_alternating_order_and_sample_counts(monkeypatch):
    seen = []
    arms = {"second": lambda: "s", "first": lambda: "f", "third": lambda: "t"}        # dict order, not alphabetical
    counts = {"second": 7, "first": 2, "third": 5}
    monkeypatch.setattr(benchlib, "time_calls", lambda fn, n: (seen.append((fn(), n)), float(len(seen)))[1])
    samples = benchlib.alternating(arms, counts, 4)
    assert seen == [("s", 7), ("f", 2), ("t", 5)] * 4
    assert list(samples) == list(arms) and all(len(v) == 4 for v in samples.values())
    assert samples["second"] == [1.0, 4.0, 7.0, 10.0] and samples["third"] == [3.0, 6.0, 9.0, 12.0]


def test_summary():
    s = benchlib.summary([4.0, 1.0, 2.0, 8.0, 3.0])
    assert (s.median, s.min, s.max, s.spread) == (3.0, 1.0, 8.0, 7.0 / 3.0)
    assert benchlib.summary([2.0, 4.0]).median == 3.0


@pytest.fixture
def recorded_remarks(monkeypatch):
    """hipcc found, its run replaced by the recorded text on stderr; the commands it was given"""
    cmds = []
    monkeypatch.setattr(benchlib, "find_hipcc", lambda: "hipcc")
    monkeypatch.setattr(benchlib.subprocess, "run", lambda cmd, **kw: (cmds.append(cmd), SimpleNamespace(stderr=REMARKS))[1])
    return cmds


def test_resource_usage_parses_both_blocks(recorded_remarks):
    rows = benchlib.resource_usage("corr_topk_f16x3.hip")
    assert [(r.name, r.vgprs, r.agprs, r.scratch, r.occupancy) for r in rows] == [(K1, 227, 0, 0, 2), (K8, 245, 0, 0, 2)]
    assert [r.sgprs for r in rows] == [64, 70]
    (cmd,) = recorded_remarks
    assert cmd[0] == "hipcc" and "--cuda-device-only" in cmd and "-Rpass-analysis=kernel-resource-usage" in cmd
    assert "--offload-arch=gfx950" in cmd and cmd[cmd.index("-c") + 1].endswith(os.path.join("csrc", "corr_topk_f16x3.hip"))


def test_resource_usage_honours_keep(recorded_remarks):
    assert [r.name for r in benchlib.resource_usage("corr_topk_f16x3.hip", keep=("ILi8E",))] == [K8]
    assert [r.name for r in benchlib.resource_usage("corr_topk_f16x3.hip", keep=("ILi8E", "ILi1ELb0E"))] == [K1, K8]
    assert benchlib.resource_usage("corr_topk_f16x3.hip", keep=("no_such_kernel",)) == []


def test_resource_usage_without_hipcc(monkeypatch):
    monkeypatch.setattr(benchlib, "find_hipcc", lambda: None)
    monkeypatch.setattr(benchlib.subprocess, "run", lambda *a, **kw: pytest.fail("nothing to run without hipcc"))
    assert benchlib.resource_usage("corr_topk_f16x3.hip") is None


def test_common_args_defaults_and_the_rounds_floor():
    ap = argparse.ArgumentParser(prog="some_bench.py")
    benchlib.common_args(ap, os.path.join("profiles", "some.txt"))
    args = ap.parse_args([])
    assert (args.out, args.rounds, args.window, args.warmup) == (os.path.join("profiles", "some.txt"), 21, 0.05, 3)
    assert ap.parse_args(["--rounds", "20"]).rounds == 20
    with pytest.raises(SystemExit) as exc:
        ap.parse_args(["--rounds", "19"])
    assert exc.value.code == "some_bench: the medians are over at least 20 rounds"


def test_common_args_own_defaults():
    ap = argparse.ArgumentParser(prog="other_bench.py")
    benchlib.common_args(ap, "x.json", min_rounds=0, rounds=7, window=0.2)
    args = ap.parse_args(["--rounds", "1"])
    assert (args.rounds, args.window) == (1, 0.2) and ap.parse_args([]).rounds == 7
