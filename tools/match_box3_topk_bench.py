"""K41 timing: the top-k match readout on the fused match_kernel-3 route (PONO_C) against the route it replaces for k > 1 — the
materialised chain (c_raw, the box-filtered logits, one sweep by K39b) — and against the argmax readout (K37) it extends, at the two
benchmark shapes: B = 8 on a 64 x 64 grid and B = 1 on a 128 x 128 grid.

Arms, all timed with device events inside ONE process, alternating round by round so that drift and neighbours on the host hit all of
them alike; the figure of an arm is the median over the rounds (>= 20) after a warm-up:
    k37                      hot_path.correspondence_match(topk=1) from raw theta / phi: K12, split, the x-box GEMM, K37
    k41 k                    the same call with topk=k, ops.MATCH_FUSED = True: K12, split, the x-box GEMM, K41
    chain k                  the same call with ops.MATCH_FUSED = False — the route of every k > 1 before K41: c_raw, box filter, K39b
    kernel k37 / k41 k       the readout kernel alone on a ready T, rows and transposed (`T`)
plus the peak memory above the inputs of both routes and, when hipcc is at hand, the register figures of every instantiation.
The rule the file records: a k at which `k41` is slower than `chain` at either shape leaves ops.box3_topk_ok.

    python tools/match_box3_topk_bench.py [--out profiles/k41_match_box3_topk.txt] [--rounds 21] [--window 0.05]
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
KS = (2, 4, 8)


def register_rows():
    """[(K, chunked, VGPRs, AGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of every box3_topk_kernel instantiation (K = 1 is K37) from
    hipcc's kernel-resource-usage remarks (device code only); None without hipcc.  LDS is dynamic: the report says 0."""
    usage = benchlib.resource_usage("box3_fused_f16x3.hip", keep=("box3_topk_kernel",))
    if usage is None:
        return None
    rows = []
    for u in usage:
        k, chunked, bias = re.search(r"kernelILi(\d+)ELb([01])ELb([01])E", u.name).groups()
        if bias == "1":       # K54's instantiations: tools/match_box3_transport_bench.py
            continue
        rows.append((int(k), int(chunked), u.vgprs, u.agprs, u.sgprs, u.scratch, u.occupancy))
    return sorted(rows)


def bench_shape(B, H, W, args, lines):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    N = H * W
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1
    phi = 0.3 * theta.roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05

    def match(fused, k, direction="rows"):
        ops.MATCH_FUSED = fused
        try:
            return correspondence_match(theta, phi, cfg, topk=k, direction=direction)
        finally:
            ops.MATCH_FUSED = True

    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)

    def kernel(k, transposed):
        q, kk = ((nu, b), (mu, a)) if transposed else ((mu, a), (nu, b))
        if k == 1:
            return ops.box3_match(t, *q, *kk, H, W, KC, INV_T, transposed=transposed)
        return ops.box3_topk(t, *q, *kk, H, W, KC, INV_T, k, transposed=transposed)

    arms = {"k37": lambda: match(True, 1), "kernel k37": lambda: kernel(1, False), "kernel k37 T": lambda: kernel(1, True)}
    for k in KS:
        arms[f"k41 {k}"] = lambda k=k: match(True, k)
        arms[f"chain {k}"] = lambda k=k: match(False, k)
        arms[f"kernel k41 {k}"] = lambda k=k: kernel(k, False)
        arms[f"kernel k41 {k} T"] = lambda k=k: kernel(k, True)
    shipped = [k for k in KS if ops.box3_topk_ok(k)]

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {"k37": benchlib.peak_bytes(lambda: match(True, 1))}
    for k in KS:
        peaks[f"k41 {k}"] = benchlib.peak_bytes(lambda: match(True, k))
        peaks[f"chain {k}"] = benchlib.peak_bytes(lambda: match(False, k))
    # both routes agree on what they return (the picks may differ where two logits are closer than the kernels' error)
    x, y = match(True, 8), match(False, 8)
    parity = (float((x.index == y.index).float().mean()), float((x.logit - y.logit).abs().max()), float((x.lse - y.lse).abs().max()))
    del x, y

    lines.append(f"## B = {B}, {H} x {W} grid (HW = {N}); one HW x HW fp32 tensor is {B * N * N * 4 / 2**20:.0f} MiB")
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:18s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    for k in KS:
        lines.append(f"k = {k}: chain / k41 = {med[f'chain {k}'] / med[f'k41 {k}']:.3f}   k41 / k37 = {med[f'k41 {k}'] / med['k37']:.3f}   "
                     f"kernel k41 / kernel k37 = {med[f'kernel k41 {k}'] / med['kernel k37']:.3f} (rows), "
                     f"{med[f'kernel k41 {k} T'] / med['kernel k37 T']:.3f} (transposed)")
    lines.append(f"new route against the chain at k = 8: equal indices {parity[0]:.6f}, max |logit diff| {parity[1]:.3e}, max |lse diff| {parity[2]:.3e}")
    return [k for k in shipped if med[f"k41 {k}"] > med[f"chain {k}"]]


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k41_match_box3_topk.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_topk_bench")
    from cocosnet_amd import ops
    lines = [f"# tools/match_box3_topk_bench.py on {torch.cuda.get_device_name(0)}: match_kernel 3, PONO_C",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)",
             f"# instantiations in this build (ops.box3_topk_ok): k <= {max([1] + [k for k in KS if ops.box3_topk_ok(k)])}"]
    slower = set()
    for B, H, W in SHAPES:
        slower |= set(bench_shape(B, H, W, args, lines))
        torch.cuda.empty_cache()
    lines.append("# rule: a k at which k41 is slower than the chain at either shape leaves ops.box3_topk_ok — "
                 + (f"k = {sorted(slower)} must leave it" if slower else "none is: every instantiation stays"))
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, __launch_bounds__(256, 2); the budget at 2 waves per SIMD is 256 "
                 "VGPRs + AGPRs; LDS is dynamic: 8 Nk bytes of statistics, 32 KiB in the chunked flavour, + 18 KiB transposed)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{'K37 (K = 1)' if k == 1 else f'K41 K = {k}':12s} {'chunked' if c else 'whole  '}  VGPRs {v:3d}  AGPRs {ag:3d}  SGPRs {sg:3d}  "
                  f"scratch {s} B/lane  waves/SIMD {o}" for k, c, v, ag, sg, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
