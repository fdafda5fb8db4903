"""K44 cost: NoVGGCorrespondence.match(hard_warp=True) against match(hard_warp=True, refine=1 | 2) at B = 8 on a 64 x 64 grid (a 256 x 256
crop), and the two new kernels alone on the same operands.

Timing arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the
rounds (>= 20) after a warm-up:
    match                   net.match(hard_warp=True): the baseline (this call is unchanged by K44)
    match refine=r          net.match(hard_warp=True, refine=r), r = 1, 2: + ops.match_refine + ops.gather_patches_subcell + glue
    refine r (kernel)       ops.match_refine alone on ready operand planes, r = 1, 2, 3
    gather hard / subcell   ops.gather_patches / ops.gather_patches_subcell alone

    python tools/match_refine_bench.py [--out profiles/k44_match_refine.txt] [--rounds 21] [--window 0.05]
"""
import argparse
import os
import re
import statistics
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, CROP, NC, INV_T = 8, 256, 151, 100.0


def register_rows():
    """[(kernel, VGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of the two new kernels from hipcc's kernel-resource-usage remarks;
    None without hipcc"""
    rows = []
    for unit, want in (("plane_pair.hip", "match_refine_kernel"), ("gather_warp.hip", "gather_patches_subcell_kernel")):
        usage = benchlib.resource_usage(unit, keep=(want,))
        if usage is None:
            return None
        for u in usage:
            inst = re.search(r"kernelILi(\d+)E", u.name)
            rows.append((want + (f"<{inst.group(1)}>" if inst else ""), u.vgprs, u.sgprs, u.scratch, u.occupancy))
    return rows


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k44_match_refine.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_refine_bench")
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import ops
    dev = torch.device("cuda", 0)
    opt = cc.ade20k_options(crop_size=CROP, semantic_nc=NC, match_kernel=1)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(dev)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    g = torch.Generator(device=dev).manual_seed(4)
    onehot = lambda: torch.zeros(B, NC, CROP, CROP, device=dev).scatter_(1, torch.randint(0, NC, (B, 1, CROP, CROP), device=dev, generator=g), 1.0)
    ref_img = torch.rand(B, 3, CROP, CROP, device=dev, generator=g) * 2 - 1
    seg, ref_seg = onehot(), onehot()
    side = CROP // opt.down
    N = side * side
    with torch.no_grad():
        theta_raw, phi_raw = net.project(ref_img, None, seg, ref_seg, None, lazy=True)
        planes = ops.OperandPlanes()
        flat = lambda t: t.raw().detach().reshape(B, 256, N)
        qn = ops.center_l2norm_planes(flat(theta_raw), 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(flat(phi_raw), 1, planes, want_chan=False)
        idx, _, _ = ops.corr_match(qn, kn, INV_T, planes)
        off1, _ = ops.match_refine(qn, kn, idx, (side, side), INV_T, 1, planes)

    arms = {"match": lambda: net.match(ref_img, seg, ref_seg, hard_warp=True),
            "match refine=1": lambda: net.match(ref_img, seg, ref_seg, hard_warp=True, refine=1),
            "match refine=2": lambda: net.match(ref_img, seg, ref_seg, hard_warp=True, refine=2),
            "refine 1 (kernel)": lambda: ops.match_refine(qn, kn, idx, (side, side), INV_T, 1, planes),
            "refine 2 (kernel)": lambda: ops.match_refine(qn, kn, idx, (side, side), INV_T, 2, planes),
            "refine 3 (kernel)": lambda: ops.match_refine(qn, kn, idx, (side, side), INV_T, 3, planes),
            "gather hard": lambda: ops.gather_patches(ref_img, idx, side, side, opt.down),
            "gather subcell": lambda: ops.gather_patches_subcell(ref_img, idx, off1, (side, side), (side, side), opt.down)}
    lines = [f"# tools/match_refine_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {CROP} x {CROP} crop, {side} x {side} grid, "
             f"match_kernel 1, PONO_C, ade20k options ({NC} labels), randomly initialised network",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)",
             f"# row reads of ops.match_refine: B N (2 r + 1)^2 rows of 1 KiB (hi + lo) = "
             + ", ".join(f"{B * N * (2 * r + 1) ** 2 * 1024 / 1e9:.2f} GB at r = {r}" for r in (1, 2, 3))]
    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    for name in arms:
        v = samples[name]
        lines.append(f"{name:20s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window)")
    lines.append("ratios (medians): " + "   ".join(f"match refine={r} / match = {med[f'match refine={r}'] / med['match']:.3f}" for r in (1, 2)))
    lines.append("effective row-read rate of the kernel: " + "   ".join(
        f"r = {r}: {B * N * (2 * r + 1) ** 2 * 1024 / 1e9 / (med[f'refine {r} (kernel)'] * 1e-3):.0f} GB/s" for r in (1, 2, 3)))
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:32s} VGPRs {v:3d}  SGPRs {s:3d}  scratch {sc} B/lane  waves/SIMD {o}" for name, v, s, sc, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
