"""K55 timing: the label mask inside the match_kernel-3 readout of T — what the LABELS instantiations of box3_topk_kernel cost over the
unlabelled ones — at the two benchmark shapes, B = 8 on a 64 x 64 grid and B = 1 on a 128 x 128 grid, rows and transposed, k = 1 and 4.

Arms, all on one ready T, timed with device events inside ONE process, alternating window by window; the figure of an arm is the
median over the windows after a warm-up:
    plain k / plain k T          ops.box3_topk (cocos_box3_topk_f16x3): the stream the mask rides on
    one label k / ... T          ops.box3_topk_labelled with one label everywhere: the mask's instructions, no element masked
    7 classes k / ... T          the same entry with 7 blocky classes (blocks of 8 x 8 cells) on both sides
The ratio of every labelled arm against its plain arm is printed next to the plain arm's window spread, then, when hipcc is at hand,
the register figures of every instantiation.

    python tools/match_box3_labels_bench.py [--out profiles/k55_match_box3_labels.txt] [--rounds 21] [--window 0.05]
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

SHAPES = ((8, 64, 64), (1, 128, 128))
INV_T, KC = 100.0, 2304.0
KS = (1, 4)


def register_rows():
    """[(flavour, K, chunked, VGPRs, AGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of every box3_topk_kernel instantiation; None
    without hipcc"""
    usage = benchlib.resource_usage("box3_fused_f16x3.hip", keep=("box3_topk_kernel",))
    if usage is None:
        return None
    rows = []
    for u in usage:
        k, chunked, bias, labels = re.search(r"kernelILi(\d+)ELb([01])ELb([01])ELb([01])E", u.name).groups()
        rows.append(("LABELS" if int(labels) else "BIAS" if int(bias) else "plain", int(k), int(chunked), u.vgprs, u.agprs, u.sgprs, u.scratch,
                     u.occupancy))
    return sorted(rows)


def blocky(B, H, W, classes, cell, gen, dev):
    lab = torch.randint(0, classes, (B, H // cell, W // cell), device=dev, generator=gen)
    return lab.repeat_interleave(cell, 1).repeat_interleave(cell, 2).reshape(B, H * W).to(torch.int32).contiguous()


def bench_shape(B, H, W, args, lines):
    from cocosnet_amd import ops
    dev = torch.device("cuda", 0)
    N = H * W
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1
    phi = 0.3 * theta.roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)
    one = torch.zeros(B, N, device=dev, dtype=torch.int32)
    q7, k7 = blocky(B, H, W, 7, 8, g, dev), blocky(B, H, W, 7, 8, g, dev)

    def plain(k, transposed):
        q, kk = ((nu, b), (mu, a)) if transposed else ((mu, a), (nu, b))
        return ops.box3_topk(t, *q, *kk, H, W, KC, INV_T, k, transposed=transposed)

    def labelled(ql, kl, k, transposed):
        q, kk = ((nu, b), (mu, a)) if transposed else ((mu, a), (nu, b))
        if transposed:
            ql, kl = kl, ql
        return ops.box3_topk_labelled(t, *q, *kk, ql, kl, H, W, KC, INV_T, k, transposed=transposed)

    arms = {}
    for k in KS:
        for transposed in (False, True):
            tag = f"k{k}{' T' if transposed else ''}"
            arms[f"plain {tag}"] = lambda k=k, tr=transposed: plain(k, tr)
            arms[f"one label {tag}"] = lambda k=k, tr=transposed: labelled(one, one, k, tr)
            arms[f"7 classes {tag}"] = lambda k=k, tr=transposed: labelled(q7, k7, k, tr)
    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    same = all(torch.equal(x, y) for x, y in zip(plain(4, False), labelled(one, one, 4, False)))
    allowed = float((q7.unsqueeze(2) == k7.unsqueeze(1)).float().mean()) if N <= 4096 else float((q7[:, ::4].unsqueeze(2) == k7.unsqueeze(1)).float().mean())

    lines.append(f"## B = {B}, {H} x {W} grid (HW = {N}); T is {B * N * N * 4 / 2**20:.0f} MiB; 7 classes allow {allowed:.3f} of the pairs; "
                 f"one label is box3_topk bit for bit: {same}")
    for name in arms:
        v = samples[name]
        lines.append(f"{name:18s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window)")
    spread = lambda n: (max(samples[n]) - min(samples[n])) / med[n]
    for k in KS:
        for transposed in (False, True):
            tag = f"k{k}{' T' if transposed else ''}"
            base = f"plain {tag}"
            lines.append(f"{tag:5s} one label / plain = {med['one label ' + tag] / med[base]:.3f}   7 classes / plain = "
                         f"{med['7 classes ' + tag] / med[base]:.3f}   (plain window spread {spread(base):.3f}; T at "
                         f"{B * N * N * 4 / (med[base] * 1e-3) / 1e12:.2f} TB/s plain, {B * N * N * 4 / (med['7 classes ' + tag] * 1e-3) / 1e12:.2f} TB/s masked)")


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k55_match_box3_labels.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_labels_bench")
    lines = [f"# tools/match_box3_labels_bench.py on {torch.cuda.get_device_name(0)}: match_kernel 3, PONO_C, the readout of one ready T",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)"]
    for B, H, W in SHAPES:
        bench_shape(B, H, W, args, lines)
        torch.cuda.empty_cache()
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, __launch_bounds__(256, 2); the budget at 2 waves per SIMD is 256 "
                 "VGPRs + AGPRs; LDS is dynamic: LABELS 12 Nk bytes of statistics and label bits, 48 KiB in the chunked flavour, + 18 KiB transposed)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{fl:6s} K = {k}  {'chunked' if c else 'whole  '}  VGPRs {v:3d}  AGPRs {ag:3d}  SGPRs {sg:3d}  scratch {s} B/lane  waves/SIMD {o}"
                  for fl, k, c, v, ag, sg, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
