"""K49 cost of the trainable match readout: forward + backward of ops.corr_pair_nll (cocos_corr_match_mutual_f16x3, the pair kernels,
two sweeps of cocos_corr_lse_bwd_f16x3) against the materialised arm built from ops that existed before it, on the same operands:

    (a) materialised       ops.corr_materialize -> torch.logsumexp over both axes -> gather of the target's logit and column lse,
                           autograd through the [B,N,N] matrix
    (b) corr_pair_nll      nothing N x N in memory
    (c) the sweep alone    one cocos_corr_lse_bwd_f16x3 call (d qn with both g), and its share of the f16 MFMA peak / 3:
                           2 products x 2 N^2 256 FLOP of useful work, three f16 terms each

Alternating windows, median and spread, as tools/match_mutual_bench.py; peak allocation growth of one forward + backward per arm.
    python tools/match_nll_bench.py [--out profiles/k49_match_nll_timing.txt] [--shapes 8x64,1x128]
"""
import argparse
import os
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INV_T = 100.0
F16_MFMA_PEAK_TFLOPS = 2516.6      # MI355X dense f16 matrix peak (vendor figure); the split product spends three terms per useful one


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k49_match_nll_timing.txt"), min_rounds=0)
    ap.add_argument("--shapes", default="8x64,1x128", help="comma-separated B x grid side")
    args = ap.parse_args()
    benchlib.require_gpu("match_nll_bench")
    from cocosnet_amd import ops
    dev = torch.device("cuda", 0)
    lines = [f"# tools/match_nll_bench.py on {torch.cuda.get_device_name(0)}: K = 256, inv_t = {INV_T:g}; ms per call: median of {args.rounds} "
             f"alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)"]
    for shape in args.shapes.split(","):
        B, side = (int(v) for v in shape.split("x"))
        N = side * side
        g = torch.Generator(device=dev).manual_seed(1000 + N)
        unit = lambda x: torch.nn.functional.normalize(x - x.mean(1, keepdim=True), dim=1).contiguous()
        q0 = unit(torch.randn(B, 256, N, device=dev, generator=g))
        k0 = unit(q0.roll(37, 2) + 0.5 * torch.randn(B, 256, N, device=dev, generator=g))
        t = ((torch.arange(N, device=dev) + 37) % N).unsqueeze(0).expand(B, -1).contiguous()
        q, k = q0.clone().requires_grad_(True), k0.clone().requires_grad_(True)

        def materialised():
            L = ops.corr_materialize(q, k, INV_T)
            s = L.gather(2, t.unsqueeze(2)).squeeze(2)
            loss = (torch.logsumexp(L, 2) - s).mean() + (torch.logsumexp(L, 1).gather(1, t) - s).mean()
            q.grad = k.grad = None
            loss.backward()

        def fused():
            r, c = ops.corr_pair_nll(q, k, t, INV_T)
            q.grad = k.grad = None
            (r.mean() + c.mean()).backward()

        with torch.no_grad():
            pl = (*ops.split_f16(q0, True, ops.SPLIT_OPERAND_SCALE), *ops.split_f16(k0, True, ops.SPLIT_OPERAND_SCALE))
            rows, cols = ops._corr_match_mutual_planes(*pl, INV_T)
            ga, gb = torch.randn(B, N, device=dev, generator=g), torch.randn(B, N, device=dev, generator=g)
        sweep = lambda: ops._corr_lse_bwd_planes(*pl, rows[2], cols[2], ga, gb, INV_T)
        arms = {"(b) corr_pair_nll fwd+bwd": fused, "(c) the sweep alone": sweep}
        try:
            mem_a = benchlib.peak_bytes(materialised) / 2 ** 20
            arms = dict({"(a) materialised fwd+bwd": materialised}, **arms)
        except torch.cuda.OutOfMemoryError:
            mem_a = None
        mem_b = benchlib.peak_bytes(fused) / 2 ** 20
        lines.append(f"## B = {B}, {side} x {side} grid (Nq = Nk = {N})")
        lines.append("peak allocation growth of one forward + backward: (a) " + ("out of memory" if mem_a is None else f"{mem_a:.1f} MiB")
                     + f"   (b) {mem_b:.1f} MiB")
        counts = benchlib.window_counts(arms, args.window, args.warmup)
        samples = benchlib.alternating(arms, counts, args.rounds)
        stats = {name: benchlib.summary(v) for name, v in samples.items()}
        med = {name: s.median for name, s in stats.items()}
        for name, s in stats.items():
            lines.append(f"{name:28s} {s.median:9.4f} ms  ({s.min:.4f} .. {s.max:.4f}; spread (max - min) / median = "
                         f"{s.spread:.4f}; {counts[name]} calls per window)")
        useful = 2 * 2.0 * B * N * N * 256
        tf = useful / (med["(c) the sweep alone"] * 1e-3) / 1e12
        lines.append(f"the sweep: {useful / 1e9:.1f} GFLOP useful -> {tf:.1f} TFLOP/s = {100 * tf / (F16_MFMA_PEAK_TFLOPS / 3):.1f} % of the f16 MFMA peak / 3 "
                     f"({F16_MFMA_PEAK_TFLOPS / 3:.0f} TFLOP/s)")
        if "(a) materialised fwd+bwd" in med:
            lines.append(f"(b) / (a) = {med['(b) corr_pair_nll fwd+bwd'] / med['(a) materialised fwd+bwd']:.4f}")
        del q, k, q0, k0, pl, rows, cols
        torch.cuda.empty_cache()
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
