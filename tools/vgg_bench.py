"""The generator step's VGG19 usage (pix2pix_model.py:248, :306, :311) on four arms, in ONE process, alternating:
  framework             ops.CONV_PRECISION = "torch", vgg.FUSED = False: the framework's convolutions and glue
  hip_convs_all_layers  K16 convolutions (f16x3), the framework's glue, and every layer up to pool5 on each call: the reference's
                        class after producers.use_hip_convs, i.e. what a user had before this module
  hip_convs             K16 convolutions, the framework's glue (vgg.FUSED = False), layers up to r52 only
  dropin                K16 convolutions + K27 glue, layers up to r52 only (cocosnet_amd.vgg as shipped)
One step = the ref and the real image forward-only + the generated image forward and input-backward, B = 8, 256 x 256, keys
r12 r22 r32 r42 r52, frozen weights (as Pix2PixModel freezes them).  Reported per arm: median ms per step over the timed rounds
(CUDA events, warm-up discarded), the forward-only and the forward + input-backward parts on their own, and the peak of
max_memory_allocated over one step above what was allocated before it.  The hip_convs and dropin arms are also compared bit for bit
(outputs and input gradient).
Usage (GPU box): python tools/vgg_bench.py [--out FILE.json] [--batch 8] [--size 256] [--rounds 7] [--iters 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from cocosnet_amd import ops, vgg  # noqa: E402
import vgg_case  # noqa: E402

KEYS = ["r12", "r22", "r32", "r42", "r52"]
#: arm -> (ops.CONV_PRECISION, vgg.FUSED, every layer): "hip_convs_all_layers" also runs conv5_3, conv5_4 and pool5 on each call,
#: as the reference's class does (the state of a user who re-classed its convolutions with producers.use_hip_convs)
ARMS = {"framework": ("torch", False, False), "hip_convs_all_layers": ("f16x3", False, True), "hip_convs": ("f16x3", False, False),
        "dropin": ("f16x3", True, False)}
_ALL = [False]


def _set(arm):
    ops.CONV_PRECISION, vgg.FUSED, _ALL[0] = ARMS[arm]


def _call(net, x):
    """the five features; with every layer, p5 (the deepest key) is computed too and dropped"""
    return net(x, KEYS + ["p5"])[:5] if _ALL[0] else net(x, KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vgg_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    net = vgg.VGG19_feature_color_torchversion(vgg_normal_correct=True)
    net.load_state_dict(vgg_case.state_dict(), strict=True)
    net = net.to(dev).eval()
    for q in net.parameters():
        q.requires_grad_(False)
    g = torch.Generator(device=dev).manual_seed(0)
    img = lambda: torch.rand(a.batch, 3, a.size, a.size, device=dev, generator=g) * 2 - 1
    ref, real, fake = img(), img(), img()
    with torch.no_grad():
        cot = [torch.randn(o.shape, device=dev, generator=g) for o in net(fake, KEYS)]

    def fwd_only():
        _call(net, ref)
        _call(net, real)

    def fwd_bwd():
        x = fake.detach().requires_grad_(True)
        torch.autograd.backward(_call(net, x), cot)
        return x

    def step():
        fwd_only()
        fwd_bwd()

    res = {arm: {"step_ms": [], "fwd_only_ms": [], "fwd_bwd_ms": []} for arm in ARMS}
    for arm in ARMS:
        _set(arm)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
    for _ in range(a.rounds):
        for arm in ARMS:
            _set(arm)
            res[arm]["step_ms"].append(benchlib.time_calls(step, a.iters))
            res[arm]["fwd_only_ms"].append(benchlib.time_calls(fwd_only, a.iters))
            res[arm]["fwd_bwd_ms"].append(benchlib.time_calls(fwd_bwd, a.iters))
    for arm in ARMS:
        _set(arm)
        res[arm]["peak_mib"] = benchlib.peak_bytes(step) / 2 ** 20
        for k in ("step_ms", "fwd_only_ms", "fwd_bwd_ms"):
            res[arm][k + "_median"] = statistics.median(res[arm][k])
    same = {}
    for arm in ("hip_convs", "dropin"):
        _set(arm)
        with torch.no_grad():
            outs = net(real, KEYS)
        same[arm] = (outs, fwd_bwd().grad)
    bitwise = all(torch.equal(p, q) for p, q in zip(same["hip_convs"][0], same["dropin"][0])) and \
        torch.equal(same["hip_convs"][1], same["dropin"][1])
    _set("dropin")
    out = {
        "workload": f"VGG19 r12..r52, B={a.batch}, {a.size}x{a.size}: 2 forward-only calls + 1 forward + input-backward, frozen weights",
        "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
        "rounds": a.rounds, "iters_per_round": a.iters, "warmup_steps": a.warmup,
        "arms": res,
        "speedup_dropin_vs_hip_convs": res["hip_convs"]["step_ms_median"] / res["dropin"]["step_ms_median"],
        "speedup_dropin_vs_hip_convs_all_layers": res["hip_convs_all_layers"]["step_ms_median"] / res["dropin"]["step_ms_median"],
        "speedup_dropin_vs_framework": res["framework"]["step_ms_median"] / res["dropin"]["step_ms_median"],
        "dropin_equals_hip_convs_bitwise": bool(bitwise),
    }
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({k: round(v["step_ms_median"], 3) for k, v in res.items()} | {"peak_mib": {k: round(v["peak_mib"]) for k, v in
                                                                                                   res.items()}}))


if __name__ == "__main__":
    main()
