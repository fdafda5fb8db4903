"""Frozen-weight inference A/B (cocosnet_amd/inference.py): the same modules, frozen records USED against records IGNORED
(inference.FROZEN = False, i.e. COCOS_FROZEN=0 — the parent's route), alternating in one process.

  (a) netCorr + netG eval() forward under torch.no_grad() at the README's inference shapes: ADE20k B = 6 at 256 x 256, CelebA-HQ B = 4
      with --warp_bilinear --adaptor_kernel 4;
  (b) the three `vggnet_fix` calls of a generator step (fake image with gradient, reference and real image without), forward +
      backward, B = 8 at 256 x 256.

Per case and arm: the median over `--runs` timed runs (device events around one forward) after `--warmup` runs of each arm, arms
alternating run by run, plus the entry-point calls per forward and how many of them prepare weights.  The baseline of any claim is the
unfrozen arm.  Writes a text table to --out (default: stdout only).

    python tools/inference_bench.py --runs 30 --warmup 5 --out profiles/inference_frozen_ab.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cocosnet_amd import _lib, inference, vgg  # noqa: E402
from cocosnet_amd import correspondence as cc  # noqa: E402
from cocosnet_amd import translation as tl  # noqa: E402

DEV = torch.device("cuda", 0)
PREP = ("cocos_conv2d_weight_planes", "cocos_split_f16_rows", "cocos_spectral_weight_fwd", "cocos_proj_weight_")


def _translation_case(opt, B, seed):
    torch.manual_seed(seed)
    corr = cc.NoVGGCorrespondence(opt).to(DEV)
    corr.init_weights(opt.init_type, opt.init_variance)
    G = tl.SPADEGenerator(opt).to(DEV)
    G.init_weights(opt.init_type, opt.init_variance)
    corr.eval(), G.eval()
    g = torch.Generator(device=DEV).manual_seed(seed + 1)
    nc, S = opt.semantic_nc, opt.crop_size
    ref = torch.rand(B, 3, S, S, device=DEV, generator=g) * 2 - 1
    real = torch.rand(B, 3, S, S, device=DEV, generator=g) * 2 - 1
    lab = lambda: torch.zeros(B, nc, S, S, device=DEV).scatter_(1, torch.randint(0, nc, (B, 1, S, S), device=DEV, generator=g), 1.0)
    seg, ref_seg = lab(), lab()

    def run():
        with torch.no_grad():
            out = corr(ref, real, seg, ref_seg, alpha=1.0)
            return G(seg, warp_out=torch.cat((out["warp_out"], seg), 1))
    return {"netCorr": corr, "netG": G}, run


def _vgg_case(B=8, S=256, seed=5):
    torch.manual_seed(seed)
    v = vgg.VGG19_feature_color_torchversion().to(DEV).eval()
    for p in v.parameters():
        p.requires_grad_(False)
    g = torch.Generator(device=DEV).manual_seed(seed)
    fake = (torch.rand(B, 3, S, S, device=DEV, generator=g)).requires_grad_(True)
    ref, real = torch.rand(B, 3, S, S, device=DEV, generator=g), torch.rand(B, 3, S, S, device=DEV, generator=g)
    keys = ["r12", "r22", "r32", "r42", "r52"]

    def run():
        fake.grad = None
        f = v(fake, keys, preprocess=True)
        r = v(ref, keys, preprocess=True)
        t = v(real, keys, preprocess=True)
        loss = sum((a - b.detach()).pow(2).mean() for a, b in zip(f, t)) + (f[-2] - r[-2].detach()).abs().mean()
        loss.backward()
        return fake.grad
    return v, run


def _weight_pointers(target):
    """data_ptr of every parameter and buffer, and of the records' effective weights (W / sigma of spectral layers)"""
    ptrs = set()
    for m in (target.values() if isinstance(target, dict) else [target]):
        for t in list(m.parameters()) + list(m.buffers()):
            ptrs.add(t.data_ptr())
        for sub in m.modules():
            rec = inference.record_of(sub)
            if rec is not None and rec.weight is not None:
                ptrs.add(rec.weight.data_ptr())
    return ptrs


def _count_calls(run, target):
    """(entry-point calls, weight-preparation calls, of which max|w| passes over a weight) of one run"""
    names, weight_absmax = [], [0]
    real = _lib.call
    ptrs = _weight_pointers(target)

    def logged(name, *args):
        names.append(name)
        if name.startswith("cocos_absmax"):
            where = args[0:12:3] if name == "cocos_absmax4" else args[0:1]
            weight_absmax[0] += any(isinstance(a, int) and a in ptrs for a in where)
        return real(name, *args)
    _lib.call = logged
    try:
        run()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    prep = [n for n in names if n.startswith(PREP)]
    return len(names), len(prep) + weight_absmax[0], weight_absmax[0]


def _time_once(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ab(name, target, run, runs, warmup, lines):
    report = inference.freeze(target)
    times = {True: [], False: []}
    for arm in (True, False):
        inference.FROZEN = arm
        for _ in range(warmup):
            run()
    torch.cuda.synchronize()
    for _ in range(runs):
        for arm in (False, True):          # alternating, the baseline first
            inference.FROZEN = arm
            times[arm].append(_time_once(run))
    counts = {}
    for arm in (False, True):
        inference.FROZEN = arm
        counts[arm] = _count_calls(run, target)
    inference.FROZEN = True
    med = {arm: statistics.median(ts) for arm, ts in times.items()}
    q = lambda ts: (sorted(ts)[len(ts) // 4], sorted(ts)[(3 * len(ts)) // 4])
    lines.append(f"{name}: {report}")
    for arm, label in ((False, "unfrozen (COCOS_FROZEN=0)"), (True, "frozen")):
        lo, hi = q(times[arm])
        c = counts[arm]
        lines.append(f"  {label:28s} median {med[arm]:8.3f} ms  (quartiles {lo:.3f} .. {hi:.3f}, {len(times[arm])} runs)   entry-point calls "
                     f"{c[0]}, weight-preparation calls {c[1]} (of which max|w| passes over a weight: {c[2]})")
    lines.append(f"  frozen / unfrozen = {med[True] / med[False]:.4f}   ({med[False] - med[True]:+.3f} ms per run)")
    inference.unfreeze(target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--cases", default="ade20k,celebahq,vgg")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inference_bench needs a GPU: timings on a CPU say nothing about the MI355X")
    if a.runs < 20:
        raise SystemExit("--runs: at least 20 timed runs per arm")
    lines = [f"frozen-weight inference A/B on {torch.cuda.get_device_name(0)}: medians over {a.runs} runs per arm after {a.warmup} warm-up "
             "runs, arms alternating in one process"]
    for case in a.cases.split(","):
        if case == "ade20k":
            nets, run = _translation_case(cc.ade20k_options(), 6, 0)
            ab("(a) ADE20k B=6 256x256, netCorr + netG eval() forward", nets, run, a.runs, a.warmup, lines)
        elif case == "celebahq":
            nets, run = _translation_case(cc.celebahq_edge_options(), 4, 10)
            ab("(a) CelebA-HQ B=4 256x256 --warp_bilinear --adaptor_kernel 4, netCorr + netG eval() forward", nets, run, a.runs, a.warmup, lines)
        elif case == "vgg":
            v, run = _vgg_case()
            ab("(b) three vggnet_fix calls of a generator step, forward + backward, B=8 256x256", v, run, a.runs, a.warmup, lines)
        else:
            raise SystemExit(f"unknown case {case!r}")
        del run
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
