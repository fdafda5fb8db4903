"""K50 cost of the transport match: one Sinkhorn half-step (cocos_corr_topk_bias_f16x3 at K = 1), ops.corr_sinkhorn at iters = 5 and
hot_path.correspondence_transport (what NoVGGCorrespondence.transport_match runs behind its projection), against the same iteration on
a materialised matrix with the ops the parent commit already has (ops.corr_materialize + torch.logsumexp over either axis).

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up; peak memory is torch's max_memory_allocated above the live memory over one call of the arm:
    (a) half-step                 ops._corr_topk_bias_planes(q, k, g, k = 1)
    (b) unbiased readout          ops._corr_match_planes(q, k) — what the bias costs on top of K36a
    (c) corr_sinkhorn iters = 5   11 launches of (a) and the affine updates on [B,N] vectors
    (d) correspondence_transport  planes, (c), the readout over z and one column launch
    (e) materialised iters = 5    f = corr_materialize(qn, kn, inv_t) once, then torch.logsumexp(f + g, 2) / (f + f_i, 1) five times

    python tools/match_transport_bench.py [--out profiles/k50_match_transport_bench.txt] [--rounds 21] [--window 0.05] [--shape 8x64]
"""
import argparse
import math
import os
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INV_T = 100.0
ITERS = 5


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k50_match_transport_bench.txt"))
    ap.add_argument("--shape", default="8x64", help="B x grid side")
    args = ap.parse_args()
    benchlib.require_gpu("match_transport_bench")
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_transport
    dev = torch.device("cuda", 0)
    B, side = (int(v) for v in args.shape.split("x"))
    N = side * side
    lines = [f"# tools/match_transport_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {side} x {side} grid (Nq = Nk = {N}), K = 256, "
             f"inv_t = {INV_T:g}, tau = 1; the same operand planes for (a), (b), (c)",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows); peak = bytes above the live memory during one call"]
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = torch.randn(B, 256, side, side, device=dev, generator=g) + 0.1
    phi = theta.roll(37, 3) + 0.5 * torch.randn(B, 256, side, side, device=dev, generator=g) - 0.05
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=4)
    with torch.no_grad():
        planes = ops.OperandPlanes()
        qn = ops.center_l2norm_planes(theta.reshape(B, 256, N), 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(phi.reshape(B, 256, N), 1, planes, want_chan=False)
        qh, ql = planes.get(qn, True, ops.SPLIT_OPERAND_SCALE)
        kh, kl = planes.get(kn, True, ops.SPLIT_OPERAND_SCALE)
        q32, k32 = ops.center_l2norm(theta.reshape(B, 256, N), 1), ops.center_l2norm(phi.reshape(B, 256, N), 1)
        f, gk, row_lse = ops._sinkhorn_planes(qh, ql, kh, kl, INV_T, ITERS, 1.0)
        log_m = -math.log(N)

        def materialised():
            m = ops.corr_materialize(q32, k32, INV_T)
            gg = torch.zeros(B, N, device=dev)
            for _ in range(ITERS):
                ff = log_m - torch.logsumexp(m + gg.unsqueeze(1), 2)
                gg = log_m - torch.logsumexp(m + ff.unsqueeze(2), 1)
            return ff, gg, torch.logsumexp(m + gg.unsqueeze(1), 2)

        ref = materialised()
        lines.append(f"fused against the materialised iteration: max |f - f| = {(f - ref[0]).abs().max().item():.3e}  max |g - g| = "
                     f"{(gk - ref[1]).abs().max().item():.3e}  max |row_lse - row_lse| = {(row_lse - ref[2]).abs().max().item():.3e}")
        plain = ops._corr_match_planes(qh, ql, kh, kl, INV_T)[0]
        moved = ops._corr_topk_bias_planes(qh, ql, kh, kl, gk, INV_T, 1)[0][..., 0]
        share = lambda ix: max(int(torch.bincount(ix[b].long(), minlength=N).max()) for b in range(B))
        lines.append(f"most-used exemplar cell: {share(plain)} queries under the softmax, {share(moved)} under the balanced plan; "
                     f"{(plain != moved).float().mean().item():.4f} of the matches move")
        arms = {"(a) half-step": lambda: ops._corr_topk_bias_planes(qh, ql, kh, kl, gk, INV_T, 1),
                "(b) unbiased readout": lambda: ops._corr_match_planes(qh, ql, kh, kl, INV_T),
                "(c) corr_sinkhorn iters=5": lambda: ops._sinkhorn_planes(qh, ql, kh, kl, INV_T, ITERS, 1.0),
                "(d) correspondence_transport": lambda: correspondence_transport(theta, phi, cfg, 1.0 / INV_T, iters=ITERS),
                "(e) materialised iters=5": materialised}
        del ref
        counts = benchlib.window_counts(arms, args.window, args.warmup)
        peaks = {name: benchlib.peak_bytes(fn) for name, fn in arms.items()}
        samples = benchlib.alternating(arms, counts, args.rounds)
    stats = {name: benchlib.summary(v) for name, v in samples.items()}
    med = {name: s.median for name, s in stats.items()}
    for name, s in stats.items():
        lines.append(f"{name:30s} {s.median:9.4f} ms  ({s.min:.4f} .. {s.max:.4f}; spread (max - min) / median = "
                     f"{s.spread:.4f}; {counts[name]} calls per window)  peak {peaks[name] / 2 ** 20:8.1f} MiB")
    flops = 2.0 * B * N * N * 256
    lines.append(f"half-step: {flops / med['(a) half-step'] / 1e9:.0f} TFLOP/s of useful work; (a) / (b) = "
                 f"{med['(a) half-step'] / med['(b) unbiased readout']:.4f}; (c) / 11 (a) = "
                 f"{med['(c) corr_sinkhorn iters=5'] / (11 * med['(a) half-step']):.4f}; (e) / (c) = "
                 f"{med['(e) materialised iters=5'] / med['(c) corr_sinkhorn iters=5']:.2f}")
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
