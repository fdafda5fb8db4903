"""K48 cost of the second direction: both directions of the hard match from ONE sweep of the correlation (cocos_corr_match_mutual_f16x3
and its finishing kernel) against two sweeps of the existing readout (cocos_corr_match_f16x3: rows, then the operands exchanged), on the
SAME operand planes.

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up:
    (a) two readouts       ops._corr_match_planes(q, k) + ops._corr_match_planes(k, q) — the baseline: existing code
    (b) fused + finish     ops._corr_match_mutual_planes(q, k): the MUTUAL instantiation and corr_match_mutual_finish_kernel
    (c) round trip alone   ops.match_round_trip on (b)'s two index maps
ops.MATCH_MUTUAL_FUSED defaults to True only if (b)'s median is below (a)'s by more than the spread (max - min) of (a)'s windows; the
last lines of the report say which way the measurement went.

    python tools/match_mutual_bench.py [--out profiles/k48_match_mutual.txt] [--rounds 21] [--window 0.05] [--shape 8x64]
"""
import argparse
import os
import re
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INV_T = 100.0


def register_rows():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of corr_match_mutual_f16x3.hip and of the K = 1 readout it is compared
    with, from hipcc's kernel-resource-usage remarks; None without hipcc"""
    rows = []
    for unit, keep in (("corr_match_mutual_f16x3.hip", None), ("corr_topk_f16x3.hip", ("ILi1ELb0ELb0E",))):
        usage = benchlib.resource_usage(unit, keep=keep)
        if usage is None:
            return None
        for u in usage:
            inst = re.search(r"kernelILi(\d+)ELb([01])ELb([01])E", u.name)
            tf = lambda c: "true" if c == "1" else "false"
            label = (f"corr_topk_f16x3_kernel<{inst.group(1)}, {tf(inst.group(2))}, {tf(inst.group(3))}>" if inst else
                     re.sub(r"^_ZN5cocos\d+", "", u.name).split("E", 1)[0])
            rows.append((label, u.vgprs, u.agprs, u.scratch, u.occupancy))
    return rows


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k48_match_mutual.txt"))
    ap.add_argument("--shape", default="8x64", help="B x grid side")
    args = ap.parse_args()
    benchlib.require_gpu("match_mutual_bench")
    from cocosnet_amd import ops
    dev = torch.device("cuda", 0)
    B, side = (int(v) for v in args.shape.split("x"))
    N = side * side
    lines = [f"# tools/match_mutual_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {side} x {side} grid (Nq = Nk = {N}), K = 256, "
             f"inv_t = {INV_T:g}; the same operand planes for every arm",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)"]
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, N, device=dev, generator=g) + 0.1
    phi = theta.roll(37, 2) + 0.5 * torch.randn(B, 256, N, device=dev, generator=g) - 0.05
    with torch.no_grad():
        planes = ops.OperandPlanes()
        qn = ops.center_l2norm_planes(theta, 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(phi, 1, planes, want_chan=False)
        qh, ql = planes.get(qn, True, ops.SPLIT_OPERAND_SCALE)
        kh, kl = planes.get(kn, True, ops.SPLIT_OPERAND_SCALE)
        rows, cols = ops._corr_match_mutual_planes(qh, ql, kh, kl, INV_T)
        want_r, want_c = ops._corr_match_planes(qh, ql, kh, kl, INV_T), ops._corr_match_planes(kh, kl, qh, ql, INV_T)
        lines.append("rows == cocos_corr_match_f16x3 bitwise: " + str(all(torch.equal(x, y) for x, y in zip(rows, want_r))))
        same = (cols[0] == want_c[0]).float().mean().item()
        lines.append(f"columns against the exchanged readout: equal indices {same:.6f}  equal maxima (bitwise) "
                     f"{(cols[1] == want_c[1]).float().mean().item():.6f}  max |lse - lse| = {(cols[2] - want_c[2]).abs().max().item():.3e}")
        back = ops.match_round_trip(rows[0], cols[0], (side, side), (side, side))
        lines.append(f"mutual nearest neighbours: {(back[1] == 0).float().mean().item():.4f} of the content positions, "
                     f"{(back[3] == 0).float().mean().item():.4f} of the exemplar positions")
        arms = {"(a) two readouts": lambda: (ops._corr_match_planes(qh, ql, kh, kl, INV_T), ops._corr_match_planes(kh, kl, qh, ql, INV_T)),
                "(b) fused + finish": lambda: ops._corr_match_mutual_planes(qh, ql, kh, kl, INV_T),
                "(c) round trip alone": lambda: ops.match_round_trip(rows[0], cols[0], (side, side), (side, side))}
        counts = benchlib.window_counts(arms, args.window, args.warmup)
        samples = benchlib.alternating(arms, counts, args.rounds)
    stats = {name: benchlib.summary(v) for name, v in samples.items()}
    med = {name: s.median for name, s in stats.items()}
    for name, s in stats.items():
        lines.append(f"{name:22s} {s.median:9.4f} ms  ({s.min:.4f} .. {s.max:.4f}; spread (max - min) / median = "
                     f"{s.spread:.4f}; {counts[name]} calls per window)")
    a, b = "(a) two readouts", "(b) fused + finish"
    spread = stats[a].max - stats[a].min
    wins = med[a] - med[b] > spread
    lines.append(f"(b) / (a) = {med[b] / med[a]:.4f}   (a) - (b) = {med[a] - med[b]:+.4f} ms   spread of (a)'s windows = {spread:.4f} ms")
    lines.append(f"rule: MATCH_MUTUAL_FUSED defaults to True only if (a) - (b) > the spread of (a)'s windows -> {'True' if wins else 'False'}")

    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:44s} VGPRs {v:3d}  AGPRs {a_:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a_, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
