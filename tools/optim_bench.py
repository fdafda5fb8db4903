"""The tail of the training step on its arms, in ONE process, alternating arm by arm inside every round (K29):
  Adam over the generator step's list (SPADE generator + netCorr, ADE20k flags; two groups as Pix2PixModel.create_optimizers
  builds them) and over the PatchGAN's:
      framework        torch.optim.Adam, its default route
      framework_fused  torch.optim.Adam(fused=True), when this build accepts it (recorded if not)
      k29              cocosnet_amd.optim.fuse_adam
  EMA over the generator step's list:  reference (the loop of models/networks/generator.py:268-274 in torch ops)  vs  k29 (optim.EMA)
  copy: a float4 device-to-device copy (torch's copy_) moving the same number of bytes as the K29 arm's algorithmic traffic
        (28 B per element for Adam, 24 B with beta1 == 0, 12 B for EMA), measured in the same rounds: each K29 arm is also reported
        as a fraction of that copy's rate.
Per arm and round: device time (CUDA events around back-to-back calls, per call) and host time (perf_counter around the same
calls before the synchronise: the Python + launch cost of a call).  The number of calls is chosen per arm, from a calibration
run after the warm-up, so that one timed window lasts at least `--window` seconds (a window of a few milliseconds measures the
clock and the scheduler as much as the kernel); it is reported as `reps`.  The whole alternation runs `--rounds` times; the
report gives every round, the median and the spread (max - min) over the rounds.
Usage (GPU box): python tools/optim_bench.py [--out FILE.json] [--rounds 3] [--window 0.25] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cocosnet_amd import correspondence as cc, optim, translation as tl  # noqa: E402

DEV = torch.device("cuda", 0)


def build_lists():
    torch.manual_seed(0)
    corr = cc.NoVGGCorrespondence(cc.ade20k_options(isTrain=True)).to(DEV)
    opt = tl.celebahq_edge_train_options()
    netG, netD = tl.SPADEGenerator(opt).to(DEV), tl.MultiscaleDiscriminator(opt).to(DEV)
    g_first = [p.detach() for p in netG.parameters()]
    return {"G": (g_first + [p.detach() for p in corr.parameters()], len(g_first)), "D": ([p.detach() for p in netD.parameters()], 0)}


def make_adam(tensors, n_first, which, **extra):
    params = [torch.nn.Parameter(t.clone()) for t in tensors]
    g = torch.Generator(device=DEV).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 0.05
    if which == "G":
        groups = [{"params": params[:n_first], "lr": 1e-4}, {"params": params[n_first:], "lr": 1e-4}]
        return params, torch.optim.Adam(groups, lr=1e-4, betas=(0.0, 0.9), eps=1e-3, **extra)
    return params, torch.optim.Adam(params, lr=4e-4, betas=(0.0, 0.9), **extra)


class _RefEMA:
    def __init__(self, mu):
        self.mu, self.shadow = mu, {}

    def __call__(self, named):
        for name, p in named:
            self.shadow[name] = ((1.0 - self.mu) * p.data + self.mu * self.shadow[name]).clone()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    host = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    optim.ADAM_FUSED = True                                          # the arm under measurement, whatever the shipped default
    lists = build_lists()
    report = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": a.rounds, "window_s": a.window, "cases": {}}
    for which, (tensors, n_first) in lists.items():
        n = sum(t.numel() for t in tensors)
        arms = {}
        _, arms["framework"] = make_adam(tensors, n_first, which)
        try:
            _, o = make_adam(tensors, n_first, which, fused=True)
            o.step()
            arms["framework_fused"] = o
        except Exception as e:                                       # this build declines fused=True: recorded
            report.setdefault("notes", []).append(f"adam {which}: fused=True not accepted: {type(e).__name__}: {e}"[:300])
        _, ok = make_adam(tensors, n_first, which)
        arms["k29"] = optim.fuse_adam(ok)
        calls = {k: o.step for k, o in arms.items()}
        nbytes = 24 * n                                              # beta1 == 0: m is not read
        src = torch.empty(nbytes // 2 // 4, device=DEV)
        dst = torch.empty_like(src)
        calls["copy"] = lambda: dst.copy_(src)                       # reads nbytes / 2, writes nbytes / 2
        case = {"elements": n, "tensors": len(tensors), "algorithmic_bytes": nbytes}
        run_case(case, calls, a)
        case["k29_launches_per_step"] = ok.cocos_last_launches
        report["cases"]["adam_" + which] = case
        del arms, calls, src, dst
        torch.cuda.empty_cache()
    tensors, _ = lists["G"]
    n = sum(t.numel() for t in tensors)
    named = [(f"p{i}", torch.nn.Parameter(t.clone())) for i, t in enumerate(tensors)]

    class _Model:
        def named_parameters(self):
            return iter(named)
    ref, mine = _RefEMA(0.999), optim.EMA(0.999)
    for name, p in named:
        ref.shadow[name] = p.data.clone()
        mine.register(name, p.data)
    model = _Model()
    src = torch.empty(12 * n // 2 // 4, device=DEV)
    dst = torch.empty_like(src)
    case = {"elements": n, "tensors": len(tensors), "algorithmic_bytes": 12 * n}
    run_case(case, {"reference": lambda: ref(named), "k29": lambda: mine(model), "copy": lambda: dst.copy_(src)}, a)
    case["k29_launches_per_call"] = mine.cocos_last_launches
    report["cases"]["ema_G"] = case
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def run_case(case, calls, a):
    for fn in calls.values():
        for _ in range(a.warmup):
            fn()
    reps = {}
    for k, fn in calls.items():                                      # calibration: calls per window of a.window seconds
        dev_ms, host_ms = timed(fn, 5)
        reps[k] = max(5, int(a.window * 1e3 / max(dev_ms, host_ms, 1e-3)) + 1)
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, fn in calls.items():                                  # alternating: every arm once per round
            rounds[k].append(timed(fn, reps[k]))
    case["arms"] = {}
    for k, rs in rounds.items():
        dev = [r[0] for r in rs]
        case["arms"][k] = {"reps": reps[k], "device_ms_rounds": [round(x, 4) for x in dev], "device_ms_median": round(statistics.median(dev), 4),
                           "device_ms_spread": round(max(dev) - min(dev), 4), "host_ms_median": round(statistics.median(r[1] for r in rs), 4)}
    copy_ms = case["arms"]["copy"]["device_ms_median"]
    k29 = case["arms"]["k29"]
    k29["fraction_of_copy_rate"] = round(copy_ms / k29["device_ms_median"], 3)
    k29["algorithmic_TBps"] = round(case["algorithmic_bytes"] / k29["device_ms_median"] / 1e9, 3)
    case["arms"]["copy"]["TBps"] = round(case["algorithmic_bytes"] / copy_ms / 1e9, 3)
    others = [v["device_ms_median"] for name, v in case["arms"].items() if name not in ("k29", "copy")]
    spread = max(v["device_ms_spread"] for name, v in case["arms"].items() if name != "copy")
    case["k29_faster_than_best_other_arm_by_more_than_the_spread"] = bool(min(others) - k29["device_ms_median"] > spread)


if __name__ == "__main__":
    main()
