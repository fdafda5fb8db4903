"""K39 timing: the top-k match readout at the benchmark shape (B = 8, 64 x 64 grid, match_kernel 1, PONO_C) against the ways to the same
answer that need the HW x HW matrix, and against the argmax readout (K36a) it extends.

Arms, all timed with device events inside ONE process, alternating round by round so that drift and neighbours on the host hit all of
them alike; the figure of an arm is the median over the rounds (>= 20) after a warm-up:
    k36a                 hot_path.correspondence_match(topk=1) from raw theta / phi: K12, split, K36a
    k39a k               the same call with topk=k, ops.MATCH_FUSED = True: K12, split, K39a
    materialise+k39b k   the same call with ops.MATCH_FUSED = False: the logits as forward(return_corr=True) returns them, read once by K39b
    parent k             the way before K39: the same logits, then torch.topk and torch.logsumexp
    kernel k36a / k39a k the two fused kernels alone on ready operand planes
plus the peak memory above the inputs of the three routes and, when hipcc is at hand, the register figures of every K39a instantiation.
The rule the file records: a k at which `k39a` is slower than `materialise+k39b` at this shape leaves ops.corr_topk_ok.

    python tools/match_topk_bench.py [--out profiles/k39_match_topk.txt] [--rounds 21] [--window 0.05]
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

B, H, W, INV_T = 8, 64, 64, 100.0
KS = (2, 4, 8)


def register_rows():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of every instantiation in corr_topk_f16x3.hip (K = 1 is K36a) from
    hipcc's kernel-resource-usage remarks (device code only, a few seconds); None without hipcc"""
    usage = benchlib.resource_usage("corr_topk_f16x3.hip")
    if usage is None:
        return None
    rows = sorted((int(re.search(r"kernelILi(\d+)E", u.name).group(1)), u.vgprs, u.agprs, u.scratch, u.occupancy) for u in usage)
    return [("K36a (K = 1)" if k == 1 else f"K39a K = {k}", *rest) for k, *rest in rows]


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k39_match_topk.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_topk_bench")
    from cocosnet_amd import hot_path, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    N = H * W
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1
    phi = 0.3 * theta.roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05

    def match(fused, k):
        ops.MATCH_FUSED = fused
        try:
            return correspondence_match(theta, phi, cfg, topk=k)
        finally:
            ops.MATCH_FUSED = True

    def parent(k):
        with torch.no_grad():
            f = hot_path._scaled_logits(theta, phi, cfg, INV_T, False, 1)       # the matrix forward(return_corr=True) returns
            top = torch.topk(f, k, dim=2)
            return top.values, top.indices, torch.logsumexp(f, dim=2)

    with torch.no_grad():
        flat = lambda t: t.reshape(B, 256, N)
        qh, ql, _ = ops.center_l2norm_planes_fwd(flat(theta), 1)
        kh, kl, _ = ops.center_l2norm_planes_fwd(flat(phi), 1)

    arms = {"k36a": lambda: match(True, 1), "kernel k36a": lambda: ops._corr_match_planes(qh, ql, kh, kl, INV_T)}
    for k in KS:
        arms[f"k39a {k}"] = lambda k=k: match(True, k)
        arms[f"materialise+k39b {k}"] = lambda k=k: match(False, k)
        arms[f"parent {k}"] = lambda k=k: parent(k)
        arms[f"kernel k39a {k}"] = lambda k=k: ops._corr_topk_planes(qh, ql, kh, kl, INV_T, k)
    fused_ks = [k for k in KS if ops.corr_topk_ok(k)]

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {"k36a": benchlib.peak_bytes(lambda: match(True, 1))}
    for k in KS:
        peaks[f"k39a {k}"] = benchlib.peak_bytes(lambda: match(True, k))
        peaks[f"materialise+k39b {k}"] = benchlib.peak_bytes(lambda: match(False, k))
        peaks[f"parent {k}"] = benchlib.peak_bytes(lambda: parent(k))
    # the fused and the materialised route agree on what they return (the picks may differ where two logits are closer than the kernels' error)
    a, b = match(True, 8), match(False, 8)
    parity = (float((a.index == b.index).float().mean()), float((a.logit - b.logit).abs().max()), float((a.lse - b.lse).abs().max()))

    lines = [f"# tools/match_topk_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {H} x {W} grid (HW = {N}), match_kernel 1, PONO_C; "
             f"the HW x HW fp32 matrix is {B * N * N * 4 / 2**20:.0f} MiB",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)",
             f"# fused instantiations in this build (ops.corr_topk_ok): k <= {max(fused_ks) if fused_ks else 1}"]
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:24s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    lines.append("# ratios (medians)")
    for k in KS:
        lines.append(f"k = {k}: k39a / parent = {med[f'k39a {k}'] / med[f'parent {k}']:.3f}   k39a / (materialise+k39b) = "
                     f"{med[f'k39a {k}'] / med[f'materialise+k39b {k}']:.3f}   k39a / k36a = {med[f'k39a {k}'] / med['k36a']:.3f}   "
                     f"kernel k39a / kernel k36a = {med[f'kernel k39a {k}'] / med['kernel k36a']:.3f}")
    slower = [k for k in fused_ks if med[f"k39a {k}"] > med[f"materialise+k39b {k}"]]
    lines.append("# rule: a k at which k39a is slower than materialise+k39b at this shape leaves ops.corr_topk_ok — "
                 + (f"k = {slower} must leave it" if slower else "none is: every fused instantiation stays"))
    lines.append(f"# fused against materialised route at k = 8: equal indices {parity[0]:.6f}, max |logit diff| {parity[1]:.3e}, max |lse diff| {parity[2]:.3e}")
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the budget at 2 waves per SIMD is 256 VGPRs + AGPRs)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:12s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
