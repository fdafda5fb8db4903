"""K35 (ops.label_conv3x3) against the dense route of the same layer, and the netCorr step with / without label records.
    python tools/label_conv_bench.py [--out FILE] [--module]

Kernel level, two shapes (B = 8, nc = 151), forward and forward + backward (weight and bias gradients):
  layer1      151 -> 64, 256 x 256, zero padding                      (AdaptiveFeatureGenerator.layer1)
  mlp_shared  151 -> 128, 64 x 64 sampled from 256 x 256, reflect + ReLU   (SPADE.mlp_shared in adaptive_model_seg)
  dense arm: producers.Conv2d called as the module calls it WITHOUT a record — nearest resize, operand preparation, max|x| pass,
             split-precision MFMA convolution, ReLU — everything the label arm replaces; label arm: the same call WITH the record.
Module level (--module): bench.py's netcorr step (NoVGGCorrespondence forward + backward, batch 8, 256 x 256, ADE20k flags) with
records attached to the two one-hot maps, against the same step without them — the code path every caller had before this route
existed (the dense route is untouched by it).

Both arms of a measurement run in ONE process, interleaved round by round; a figure is the median over the rounds of HIP-event time
per iteration, `spread` = (max - min) / median."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

import benchlib
from cocosnet_amd import labels, producers

ROUNDS, ITERS, WARMUP = 7, 10, 3
NC, B = 151, 8
SHAPES = {"layer1": dict(cout=64, size=256, sample=1, reflect=0, relu=False),
          "mlp_shared": dict(cout=128, size=256, sample=4, reflect=1, relu=True)}


def _summary(ms):
    s = benchlib.summary(ms)
    return {"median_ms": round(s.median, 4), "spread": round(s.spread, 4), "rounds_ms": [round(v, 4) for v in ms]}


def _interleaved(runs):
    for f in runs.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    ms = {n: [] for n in runs}
    order = list(runs.items())
    for r in range(ROUNDS):
        for n, f in (order if r % 2 == 0 else order[::-1]):
            ms[n].append(benchlib.time_calls(f, ITERS))
    return {n: _summary(v) for n, v in ms.items()}


def bench_shape(name, cout, size, sample, reflect, relu):
    g = torch.Generator(device="cuda").manual_seed(size + cout)
    lab = torch.randint(0, NC, (B, 1, size // 16, size // 16), device="cuda", generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = labels.one_hot(lab, NC)
    rec = labels.record_of(seg)
    torch.manual_seed(0)
    conv = producers.Conv2d(NC, cout, 3, padding=0 if reflect else 1).cuda()
    params = [conv.weight, conv.bias]
    out = size // sample
    go = torch.randn(B, cout, out, out, device="cuda", generator=g)
    call = lambda r: conv(seg, reflect=reflect, labels=r, sample=sample, relu=relu)

    def fwd(r):
        with torch.no_grad():
            return call(r)
    runs = {"fwd_dense": lambda: fwd(None), "fwd_label": lambda: fwd(rec),
            "fwd_bwd_dense": lambda: torch.autograd.grad(call(None), params, go),
            "fwd_bwd_label": lambda: torch.autograd.grad(call(rec), params, go)}
    res = {"shape": name, "B": B, "nc": NC, **SHAPES[name], **_interleaved(runs)}
    res["max_abs_diff_label_vs_dense"] = float((fwd(rec) - fwd(None)).abs().max())
    res["label_not_slower"] = {k: res[k + "_label"]["median_ms"] <= res[k + "_dense"]["median_ms"] for k in ("fwd", "fwd_bwd")}
    return res


def module_ab(rounds=3, steps=6, warmup=3):
    import bench
    device = torch.device("cuda", 0)
    d = bench.build_inputs(device, "netcorr")
    torch.manual_seed(0)
    model, fwd = bench.make_step("netcorr", device)
    params = list(model.parameters())
    for k in ("seg", "ref_seg"):
        labels.attach(d[k], d[k].argmax(1, keepdim=True))

    def step():
        for p in params:
            p.grad = None
        o = fwd(d)
        torch.autograd.backward([o["warp_out"], o["warp_mask"]], [d["g_out"], d["g_mask"]])
    ms = {"0": [], "1": []}
    saved = labels.LABEL_CONV
    calls = {}
    from cocosnet_amd import _lib
    real_call = _lib.call
    for on in ("0", "1"):                     # entry-point calls of one step per arm (counted outside the timed rounds)
        labels.LABEL_CONV, seen = on, []
        _lib.call = lambda name, *a: (seen.append(name), real_call(name, *a))[1]
        try:
            step()
        finally:
            _lib.call = real_call
        calls[on] = {"entry_point_calls": len(seen), "label_conv3x3_fwd": seen.count("cocos_label_conv3x3_fwd"),
                     "label_conv3x3_bwd": seen.count("cocos_label_conv3x3_bwd"), "conv2d_nhwc_prep": sum("nhwc_prep" in n for n in seen)}
    try:
        for r in range(rounds):
            for on in (("0", "1") if r % 2 == 0 else ("1", "0")):
                labels.LABEL_CONV = on
                for _ in range(warmup):
                    step()
                torch.cuda.synchronize()
                ms[on].append(benchlib.time_calls(step, steps))
    finally:
        labels.LABEL_CONV = saved
    return {"scope": "NoVGGCorrespondence fwd+bwd, batch 8, 256x256, ADE20k flags (bench.py --scope netcorr's step)",
            "records_ignored_dense_route": {**_summary(ms["0"]), **calls["0"]},
            "records_used_label_route": {**_summary(ms["1"]), **calls["1"]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "label_conv_ab.txt"))
    ap.add_argument("--module", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("label_conv_bench: no GPU (nothing here can be measured on a CPU)")
    res = {"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "iterations_per_round": ITERS,
           "shapes": [bench_shape(n, **kw) for n, kw in SHAPES.items()]}
    if args.module:
        res["module_ab"] = module_ab()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
