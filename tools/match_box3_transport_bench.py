"""K54 timing: transport on the fused match_kernel-3 route (PONO_C) — the biased readout of T and the Sinkhorn iteration on it — at the
two benchmark shapes, B = 8 on a 64 x 64 grid and B = 1 on a 128 x 128 grid.

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
after a warm-up:
    kernel k37 / k37 T           cocos_box3_match_f16x3 on a ready T, rows and transposed: the unbiased stream the half-step extends
    half-step / half-step T      cocos_box3_topk_bias_f16x3 at k = 1 on the same T with a Sinkhorn potential as the bias
    biased k4 / biased k4 T      the same entry at k = 4
    sinkhorn 5                   ops.box3_sinkhorn(iters = 5) on the ready T: 11 launches and the affine updates
    materialised 5               the same iteration on the box logits: hot_path._box3_logits, then torch.logsumexp over both axes per
                                 iteration and once more for row_lse (the logits are made inside the timed call, as T is NOT: see total)
    T                            ops.box3_corr_xbox alone: what `sinkhorn 5` needs before it starts
    route / route k4             hot_path.correspondence_transport_box3(iters = 5) end to end from raw theta / phi (K12, split, the x-box
                                 GEMM, 11 biased launches, the column launch; k4: + the top-4 launch)
    sparse / sparse transport    hot_path.correspondence_sparse_box3 forward + backward at k = 4 without and with
                                 transport = dict(iters = 5, tau = 1)
plus the peak memory above the inputs of both routes and, when hipcc is at hand, the register figures of the BIAS instantiations.

    python tools/match_box3_transport_bench.py [--out profiles/k54_match_box3_transport.txt] [--rounds 21] [--window 0.05]
"""
import argparse
import math
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
ITERS = 5


def register_rows():
    """[(K, chunked, bias, VGPRs, AGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of every box3_topk_kernel instantiation; None
    without hipcc"""
    usage = benchlib.resource_usage("box3_fused_f16x3.hip", keep=("box3_topk_kernel",))
    if usage is None:
        return None
    rows = []
    for u in usage:
        k, chunked, bias, labels = re.search(r"kernelILi(\d+)ELb([01])ELb([01])ELb([01])E", u.name).groups()
        if int(labels):      # (K55's flavour: tools/match_box3_labels_bench.py lists it)
            continue
        rows.append((int(bias), int(k), int(chunked), u.vgprs, u.agprs, u.sgprs, u.scratch, u.occupancy))
    return sorted(rows)


def bench_shape(B, H, W, args, lines):
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, _box3_logits, correspondence_sparse_box3, correspondence_transport_box3
    dev = torch.device("cuda", 0)
    N = H * W
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1
    phi = 0.3 * theta.roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05
    with torch.no_grad():
        (mu, a), (nu, b) = ops.unfold3_stats(theta, KC), ops.unfold3_stats(phi, KC)
        t = ops.box3_corr_xbox(theta, phi)
        f, gpot, _ = ops.box3_sinkhorn(t, mu, a, nu, b, H, W, KC, INV_T, ITERS)

    def plain(transposed):
        q, kk = ((nu, b), (mu, a)) if transposed else ((mu, a), (nu, b))
        return ops.box3_match(t, *q, *kk, H, W, KC, INV_T, transposed=transposed)

    def biased(k, transposed):
        q, kk = ((nu, b), (mu, a)) if transposed else ((mu, a), (nu, b))
        return ops.box3_topk_biased(t, *q, *kk, f if transposed else gpot, H, W, KC, INV_T, k, transposed=transposed)

    def materialised():
        with torch.no_grad():
            L = _box3_logits(theta, phi, INV_T)
            log_m = -math.log(N)
            gg = torch.zeros(B, N, device=dev)
            for _ in range(ITERS):
                ff = log_m - torch.logsumexp(L + gg.unsqueeze(1), 2)
                gg = log_m - torch.logsumexp(L + ff.unsqueeze(2), 1)
            return ff, gg, torch.logsumexp(L + gg.unsqueeze(1), 2)

    def xbox():
        with torch.no_grad():
            return ops.box3_corr_xbox(theta, phi)

    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, warp_mask_losstype="direct")
    ref_img = torch.rand(B, 3, H * 4, W * 4, device=dev, generator=g) * 2 - 1
    seg = torch.zeros(B, 5, H * 4, W * 4, device=dev).scatter_(1, torch.randint(0, 5, (B, 1, H * 4, W * 4), device=dev, generator=g), 1.0)
    th_g, ph_g = theta.clone().requires_grad_(True), phi.clone().requires_grad_(True)

    def sparse(transport):
        th_g.grad = ph_g.grad = None
        out = correspondence_sparse_box3(th_g, ph_g, ref_img, seg, seg, cfg, 1.0 / INV_T, 4, transport=transport)
        (out["warp_out"].square().sum() + out["warp_mask"].square().sum()).backward()

    arms = {"kernel k37": lambda: plain(False), "kernel k37 T": lambda: plain(True),
            "half-step": lambda: biased(1, False), "half-step T": lambda: biased(1, True),
            "biased k4": lambda: biased(4, False), "biased k4 T": lambda: biased(4, True),
            "sinkhorn 5": lambda: ops.box3_sinkhorn(t, mu, a, nu, b, H, W, KC, INV_T, ITERS),
            "materialised 5": materialised, "T": xbox,
            "route": lambda: correspondence_transport_box3(theta, phi, cfg, 1.0 / INV_T, iters=ITERS),
            "route k4": lambda: correspondence_transport_box3(theta, phi, cfg, 1.0 / INV_T, iters=ITERS, topk=4),
            "sparse": lambda: sparse(None), "sparse transport": lambda: sparse(dict(iters=ITERS, tau=1.0))}
    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {"sinkhorn 5": benchlib.peak_bytes(arms["sinkhorn 5"]), "materialised 5": benchlib.peak_bytes(materialised),
             "T": benchlib.peak_bytes(xbox), "route": benchlib.peak_bytes(arms["route"]), "route k4": benchlib.peak_bytes(arms["route k4"]),
             "sparse": benchlib.peak_bytes(arms["sparse"]), "sparse transport": benchlib.peak_bytes(arms["sparse transport"])}
    x, y = ops.box3_sinkhorn(t, mu, a, nu, b, H, W, KC, INV_T, ITERS), materialised()
    parity = [float((p - q).abs().max()) for p, q in zip(x, y)]

    lines.append(f"## B = {B}, {H} x {W} grid (HW = {N}); one HW x HW fp32 tensor is {B * N * N * 4 / 2**20:.0f} MiB")
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:18s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    spread = lambda n: (max(samples[n]) - min(samples[n])) / med[n]
    lines.append(f"half-step / kernel k37 = {med['half-step'] / med['kernel k37']:.3f} (rows; window spread {spread('kernel k37'):.3f}), "
                 f"{med['half-step T'] / med['kernel k37 T']:.3f} (transposed; spread {spread('kernel k37 T'):.3f})")
    lines.append(f"T at {B * N * N * 4 / (med['half-step'] * 1e-3) / 1e12:.2f} TB/s (rows), "
                 f"{B * N * N * 4 / (med['half-step T'] * 1e-3) / 1e12:.2f} TB/s (transposed) in the half-step")
    lines.append(f"materialised 5 / (T + sinkhorn 5) = {med['materialised 5'] / (med['T'] + med['sinkhorn 5']):.3f}   "
                 f"peak: materialised {peaks['materialised 5'] / 2**20:.1f} MiB against T {peaks['T'] / 2**20:.1f} + "
                 f"{peaks['sinkhorn 5'] / 2**20:.1f} MiB")
    lines.append(f"sparse transport / sparse (forward + backward, k = 4) = {med['sparse transport'] / med['sparse']:.3f}")
    lines.append(f"both routes agree: max |f diff| {parity[0]:.3e}, |g diff| {parity[1]:.3e}, |row_lse diff| {parity[2]:.3e}")


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k54_match_box3_transport.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_transport_bench")
    lines = [f"# tools/match_box3_transport_bench.py on {torch.cuda.get_device_name(0)}: match_kernel 3, PONO_C",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)"]
    for B, H, W in SHAPES:
        bench_shape(B, H, W, args, lines)
        torch.cuda.empty_cache()
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, __launch_bounds__(256, 2); the budget at 2 waves per SIMD is 256 "
                 "VGPRs + AGPRs; LDS is dynamic: BIAS 12 Nk bytes of statistics, 48 KiB in the chunked flavour, + 18 KiB transposed)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{'BIAS' if bi else 'plain'} K = {k}  {'chunked' if c else 'whole  '}  VGPRs {v:3d}  AGPRs {ag:3d}  SGPRs {sg:3d}  "
                  f"scratch {s} B/lane  waves/SIMD {o}" for bi, k, c, v, ag, sg, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
