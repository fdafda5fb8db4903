"""K37 timing: the match readout on the fused match_kernel-3 route against the materialised chain it replaces there.

Rows, per shape (B = 8 at 64 x 64; B = 1 at 128 x 128), all timed with device events inside ONE process, the rows alternating round by
round so that drift and neighbours on the host hit all of them alike:
    k37_kernel          ops.box3_match on a ready T (cocos_box3_match_f16x3 alone), rows and transposed
    xbox_gemm+k37       ops.box3_corr_xbox (operand split + x-box GEMM) followed by ops.box3_match
    match_new           hot_path.correspondence_match from raw theta / phi, ops.MATCH_FUSED = True  (K12, split, GEMM, K37)
    match_parent        the same call with ops.MATCH_FUSED = False: K12, K3 (c_raw), K6 (logits), K36b — the route before K37
and the peak memory above the inputs of the two match() routes, plus how far the two routes' results are apart.

    python tools/match_box3_bench.py [--out profiles/k37_match_box3_timing.json] [--rounds 7] [--window 0.2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

import benchlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8, 64, 64), (1, 128, 128)]
KC, INV_T = 2304.0, 100.0


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k37_match_box3_timing.json"), min_rounds=0, rounds=7, window=0.2)
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_bench")
    from cocosnet_amd import ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window, "unit": "ms per call", "shapes": []}
    for B, h, w in SHAPES:
        N = h * w
        g = torch.Generator(device=dev).manual_seed(1000 + N)
        theta = torch.randn(B, 256, h, w, device=dev, generator=g) + 0.1
        phi = 0.3 * theta.roll((1, 7), (2, 3)) + torch.randn(B, 256, h, w, device=dev, generator=g) - 0.05
        assert ops.box3_fused_ok(B, 256, h, w)
        with torch.no_grad():
            mu, a = ops.unfold3_stats(theta, KC)
            nu, b = ops.unfold3_stats(phi, KC)
            t = ops.box3_corr_xbox(theta, phi)

        def match(fused, direction):
            ops.MATCH_FUSED = fused
            try:
                return correspondence_match(theta, phi, cfg, direction=direction)
            finally:
                ops.MATCH_FUSED = True

        def gemm_k37():
            with torch.no_grad():
                return ops.box3_match(ops.box3_corr_xbox(theta, phi), mu, a, nu, b, h, w, KC, INV_T)

        rows = {
            "k37_kernel": lambda: ops.box3_match(t, mu, a, nu, b, h, w, KC, INV_T),
            "k37_kernel_transposed": lambda: ops.box3_match(t, nu, b, mu, a, h, w, KC, INV_T, transposed=True),
            "xbox_gemm+k37": gemm_k37,
            "match_new": lambda: match(True, "rows"),
            "match_parent": lambda: match(False, "rows"),
            "match_new_cols": lambda: match(True, "cols"),
            "match_parent_cols": lambda: match(False, "cols"),
        }
        counts = benchlib.window_counts(rows, args.window, args.warmup, probe=3)
        samples = benchlib.alternating(rows, counts, args.rounds)
        new, old = match(True, "rows"), match(False, "rows")
        parity = {"equal_indices": float((new.index == old.index).float().mean()),
                  "max_abs_lse_diff": float((new.lse - old.lse).abs().max()),
                  "max_abs_max_logit_diff": float((new.max_logit - old.max_logit).abs().max())}
        del new, old
        entry = {"B": B, "grid": [h, w], "N": N, "matrix_bytes": B * N * N * 4,
                 "rows": {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "iters_per_window": counts[name], "windows": v}
                          for name, v in samples.items()},
                 "peak_bytes_above_inputs": {"match_new": benchlib.peak_bytes(lambda: match(True, "rows")),
                                             "match_parent": benchlib.peak_bytes(lambda: match(False, "rows"))},
                 "new_vs_parent": parity}
        result["shapes"].append(entry)
        print(f"B = {B}, {h} x {w}:")
        for name, v in samples.items():
            print(f"  {name:24s} median {statistics.median(v):8.4f} ms  (min {min(v):.4f}, max {max(v):.4f}; {counts[name]} calls per window)")
        pk = entry["peak_bytes_above_inputs"]
        print(f"  peak above inputs: new {pk['match_new'] / 2**20:.1f} MiB, parent {pk['match_parent'] / 2**20:.1f} MiB; new vs parent: {parity}")
        del t, theta, phi
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
