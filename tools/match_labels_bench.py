"""K47 cost of the label mask: the label-restricted scan (ops.corr_topk_labelled, the LABELS instantiations of corr_topk_f16x3.hip)
against the unlabelled scan (ops.corr_topk, K39a) on the SAME operand planes.

Arms per k, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the
rounds (>= 20) after a warm-up:
    unlabelled          ops.corr_topk — the baseline: existing code, not the code under test
    one label           ops.corr_topk_labelled with one label everywhere: every pair allowed, the pure overhead of the mask
    7 blocky classes    ops.corr_topk_labelled with the labels hot_path.cell_labels gives for a synthetic segmentation of 7 classes in
                        rectangular blocks (a different layout on the content and on the exemplar side)
Tile skipping is not built, so there is no on / off pair of rows.

    python tools/match_labels_bench.py [--out profiles/k47_match_labels.txt] [--rounds 21] [--window 0.05] [--shape 8x64] [--ks 1,4]
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

DOWN, NC, INV_T = 4, 7, 100.0


def register_rows():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of corr_topk_f16x3.hip from hipcc's kernel-resource-usage remarks;
    None without hipcc"""
    usage = benchlib.resource_usage("corr_topk_f16x3.hip")
    if usage is None:
        return None
    rows = []
    for u in usage:
        inst = re.search(r"kernelILi(\d+)ELb([01])E", u.name)
        label = f"corr_topk_f16x3_kernel<{inst.group(1)}, {'true' if inst.group(2) == '1' else 'false'}>" if inst else u.name
        rows.append((label, u.vgprs, u.agprs, u.scratch, u.occupancy))
    return rows


def blocky_segmentation(B, H, W, blocks, seed, dev):
    """one-hot [B,NC,H,W]: a blocks x blocks chessboard of rectangles with random cuts, each rectangle one of NC classes"""
    g = torch.Generator().manual_seed(seed)
    lab = torch.zeros(B, H, W, dtype=torch.int64)
    for b in range(B):
        ys = [0] + sorted(torch.randperm(H - 1, generator=g)[:blocks - 1].add(1).tolist()) + [H]
        xs = [0] + sorted(torch.randperm(W - 1, generator=g)[:blocks - 1].add(1).tolist()) + [W]
        for i in range(blocks):
            for j in range(blocks):
                lab[b, ys[i]:ys[i + 1], xs[j]:xs[j + 1]] = int(torch.randint(0, NC, (1,), generator=g))
    return torch.zeros(B, NC, H, W).scatter_(1, lab.unsqueeze(1), 1.0).to(dev)


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k47_match_labels.txt"))
    ap.add_argument("--shape", default="8x64", help="B x grid side")
    ap.add_argument("--ks", default="1,4")
    args = ap.parse_args()
    benchlib.require_gpu("match_labels_bench")
    from cocosnet_amd import hot_path, ops
    dev = torch.device("cuda", 0)
    B, side = (int(v) for v in args.shape.split("x"))
    H = W = side
    N = H * W
    lines = [f"# tools/match_labels_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {H} x {W} grid (Nq = Nk = {N}), K = 256, "
             f"inv_t = {INV_T:g}; the same operand planes for every arm; tile skipping: not built",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)"]
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, N, device=dev, generator=g) + 0.1
    phi = theta.roll(37, 2) + 0.5 * torch.randn(B, 256, N, device=dev, generator=g) - 0.05
    with torch.no_grad():
        planes = ops.OperandPlanes()
        qn = ops.center_l2norm_planes(theta, 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(phi, 1, planes, want_chan=False)
        one = torch.zeros(B, N, dtype=torch.int32, device=dev)
        q_lab = hot_path.cell_labels(blocky_segmentation(B, H * DOWN, W * DOWN, 4, 1, dev), DOWN).reshape(B, N)
        k_lab = hot_path.cell_labels(blocky_segmentation(B, H * DOWN, W * DOWN, 4, 2, dev), DOWN).reshape(B, N)
    share = (q_lab.unsqueeze(2) == k_lab.unsqueeze(1)).float().mean().item()
    lines.append(f"# 7 blocky classes: 4 x 4 rectangles per image, {share:.3f} of the (query, key) pairs allowed")
    for k in (int(v) for v in args.ks.split(",")):
        q_eff, k_eff, restricted = hot_path.restrict_fallback(q_lab, k_lab, k)
        lines.append(f"## k = {k}  ({int(restricted.sum())} of {restricted.numel()} positions restricted after the fallback rule)")
        arms = {"unlabelled": lambda: ops.corr_topk(qn, kn, INV_T, k, planes),
                "one label": lambda: ops.corr_topk_labelled(qn, kn, one, one, INV_T, k, planes),
                "7 blocky classes": lambda: ops.corr_topk_labelled(qn, kn, q_eff, k_eff, INV_T, k, planes)}
        a, b_ = arms["unlabelled"](), arms["one label"]()
        lines.append("one label == unlabelled bitwise: " + str(all(torch.equal(x, y) for x, y in zip(a, b_))))
        counts = benchlib.window_counts(arms, args.window, args.warmup)
        samples = benchlib.alternating(arms, counts, args.rounds)
        med = {name: statistics.median(v) for name, v in samples.items()}
        for name in arms:
            v = samples[name]
            lines.append(f"{name:20s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window)")
        base = samples["unlabelled"]
        lines.append(f"ratios (medians): one label / unlabelled = {med['one label'] / med['unlabelled']:.4f}   "
                     f"7 blocky classes / unlabelled = {med['7 blocky classes'] / med['unlabelled']:.4f}   "
                     f"spread of the unlabelled windows (max - min) / median = {(max(base) - min(base)) / med['unlabelled']:.4f}")

    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:36s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
