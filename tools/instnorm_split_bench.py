"""K34 (ops.instnorm_prelu_split) against the two routes a plane above 128 x 128 has today, forward + backward, at the sizes the
adaptors and the PatchGAN run it.     python tools/instnorm_split_bench.py [--out FILE] [--module]

Arms (no residual, slope 0.2 — what producers._conv_norm_act / translation._ConvNormAct call):
  (a) framework   nn.InstanceNorm2d(affine=False) + F.leaky_relu: the branch the callers take with ops.INSTNORM_SPLIT = False
  (b) split       ops.instnorm_prelu_split (K34)
  (c) streaming   ops.instnorm_prelu, which takes K13's one-workgroup-per-plane path at these sizes
Two gradient sets: `all` (x and the one-element weight) and `x_only` (the callers' slope tensor needs no gradient; arm (a) has no
weight, so its two sets are the same computation).  The convolution that reads the output next needs max|y|: arm (b) leaves it,
arm (a) pays `ops.absmax(y)` — timed on its own and reported as `absmax_ms`, never folded into (a).

All arms of a shape run in ONE process, interleaved round by round (boxes differ by a few percent); a figure is the median over the
rounds of HIP-event time per iteration, `spread` = (max - min) / median over the rounds.  GB/s of (b) is the byte accounting of
csrc/instnorm_split.hip (forward 12 B/element, backward 20) over the time between HIP events around each entry point.
--module: one A/B of the whole NoVGGCorrespondence step (bench.py's netcorr scope: same model, same inputs) with the switch off / on."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch
import torch.nn.functional as F

import benchlib
from cocosnet_amd import ops

SHAPES = [(8, 64, 256, 256), (4, 64, 512, 512), (4, 128, 256, 256), (4, 256, 256, 256)]
ROUNDS, ITERS, WARMUP = 7, 10, 3


def _summary(ms):
    s = benchlib.summary(ms)
    return {"median_ms": round(s.median, 4), "spread": round(s.spread, 4), "rounds_ms": [round(v, 4) for v in ms]}


def bench_shape(shape):
    B, C, h, w = shape
    g = torch.Generator(device="cuda").manual_seed(C + h)
    x = (torch.randn(*shape, device="cuda", generator=g) * 3 + 0.5).requires_grad_(True)
    go = torch.randn(*shape, device="cuda", generator=g)
    norm = torch.nn.InstanceNorm2d(C, affine=False)
    arms = {}
    for grads in ("all", "x_only"):
        wt = torch.full((1,), 0.2, device="cuda", requires_grad=(grads == "all"))
        wrt = (x, wt) if grads == "all" else (x,)
        arms[grads] = {
            "a_framework": lambda: torch.autograd.grad(F.leaky_relu(norm(x), 0.2), (x,), go),
            "b_split": lambda wt=wt, wrt=wrt: torch.autograd.grad(ops.instnorm_prelu_split(x, None, wt), wrt, go),
            "c_streaming": lambda wt=wt, wrt=wrt: torch.autograd.grad(ops.instnorm_prelu(x, None, wt), wrt, go),
        }
    y = ops.instnorm_prelu_split(x.detach(), None, torch.full((1,), 0.2, device="cuda"))
    extra = {"absmax": lambda: ops.absmax(y)}
    runs = [(gs, name, f) for gs, d in arms.items() for name, f in d.items()] + [("", n, f) for n, f in extra.items()]
    for _, _, f in runs:
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ms = {(gs, n): [] for gs, n, _ in runs}
    for r in range(ROUNDS):
        for gs, n, f in (runs if r % 2 == 0 else runs[::-1]):
            ms[(gs, n)].append(benchlib.time_calls(f, ITERS))
    out = {"shape": list(shape), "elements": x.numel(), "MB_per_tensor": round(x.numel() * 4 / 1e6, 1)}
    for gs in arms:
        out[gs] = {n: _summary(ms[(gs, n)]) for n in arms[gs]}
    out["absmax_ms"] = _summary(ms[("", "absmax")])
    # the two entry points of (b) between HIP events of their own, against the byte accounting
    with ops.KernelTimer(tags=("instnorm_prelu_split_fwd", "instnorm_prelu_split_bwd")) as kt:
        for _ in range(ITERS):
            arms["all"]["b_split"]()
    k = kt.summary()
    n = x.numel()
    out["b_split_calls"] = {
        "fwd_ms": round(k["instnorm_prelu_split_fwd"]["avg_ms"], 4), "fwd_bytes_per_element": 12,
        "fwd_GBps": round(12 * n / k["instnorm_prelu_split_fwd"]["avg_ms"] / 1e6, 1),
        "bwd_ms": round(k["instnorm_prelu_split_bwd"]["avg_ms"], 4), "bwd_bytes_per_element": 20,
        "bwd_GBps": round(20 * n / k["instnorm_prelu_split_bwd"]["avg_ms"] / 1e6, 1)}
    # results must not change with the route: (b) against (a) on the same input
    ya = F.leaky_relu(norm(x.detach()), 0.2)
    out["max_abs_diff_b_vs_a"] = float((y - ya).abs().max())
    return out


def verdict(rows):
    """The rule of DESIGN §3.19: True only if (b) <= (a) at [8, 64, 256, 256] and (b) is not slower than (a) by more than the measured
    run-to-run spread at any other shape (gradient set `all`)."""
    ok, why = True, []
    for i, r in enumerate(rows):
        a, b = r["all"]["a_framework"], r["all"]["b_split"]
        slack = 0.0 if i == 0 else max(a["spread"], b["spread"]) * a["median_ms"]
        good = b["median_ms"] <= a["median_ms"] + slack
        why.append({"shape": r["shape"], "a_ms": a["median_ms"], "b_ms": b["median_ms"], "slack_ms": round(slack, 4), "ok": good})
        ok = ok and good
    return {"INSTNORM_SPLIT_default": ok, "per_shape": why}


def module_ab(rounds=3, steps=6, warmup=3):
    import bench
    device = torch.device("cuda", 0)
    d = bench.build_inputs(device, "netcorr")
    torch.manual_seed(0)
    model, fwd = bench.make_step("netcorr", device)
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        o = fwd(d)
        torch.autograd.backward([o["warp_out"], o["warp_mask"]], [d["g_out"], d["g_mask"]])
    ms = {False: [], True: []}
    saved = ops.INSTNORM_SPLIT
    try:
        for r in range(rounds):
            for on in ((False, True) if r % 2 == 0 else (True, False)):
                ops.INSTNORM_SPLIT = on
                for _ in range(warmup):
                    step()
                torch.cuda.synchronize()
                ms[on].append(benchlib.time_calls(step, steps))
    finally:
        ops.INSTNORM_SPLIT = saved
    return {"scope": "NoVGGCorrespondence fwd+bwd, batch 8, 256x256, ADE20k flags (bench.py --scope netcorr's step)",
            "INSTNORM_SPLIT_off": _summary(ms[False]), "INSTNORM_SPLIT_on": _summary(ms[True])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "k34_instnorm_split_bench.json"))
    ap.add_argument("--module", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("instnorm_split_bench: no GPU (nothing here can be measured on a CPU)")
    rows = [bench_shape(s) for s in SHAPES]
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "iterations_per_round": ITERS,
           "slice": 16384, "shapes": rows, "rule": verdict(rows)}
    if args.module:
        res["module_ab"] = module_ab()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
