#!/usr/bin/env python3
"""K30: hot-path forward + backward per flag set with ops.WARP_HEAD_MODES on and off, arms alternating inside each round of ONE
process (every shape warmed first, windows of at least --window seconds), and the same arm repeated as the spread.

    python tools/warp_head_bench.py --out profiles/k30_head_bench.json

Reports per flag set and arm: ms per step (median of the rounds), the spread of the rounds, peak allocated memory."""
import argparse
import json
import os
import sys
import time

import torch

import benchlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cocosnet_amd import ops                                                     # noqa: E402
from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path         # noqa: E402

# name -> (flags, B, grid, label channels): the README training commands at their shapes
SETS = {
    "celeba_edge_mk1": (dict(match_kernel=1, warp_bilinear=True, warp_cycle_w=1.0, warp_mask_losstype="none"), 16, 64, 15),
    "celeba_edge_mk3": (dict(match_kernel=3, warp_bilinear=True, warp_cycle_w=1.0, warp_mask_losstype="none"), 16, 64, 15),
    "celeba_mask_mk3": (dict(match_kernel=3, warp_bilinear=True, warp_cycle_w=0.1, warp_mask_losstype="direct"), 8, 64, 19),
    "fashion_256_mk3": (dict(match_kernel=3, warp_patch=True, warp_bilinear=True, warp_mask_losstype="none"), 4, 64, 20),
    "fashion_512_mk3": (dict(match_kernel=3, warp_patch=True, warp_bilinear=True, warp_mask_losstype="none"), 2, 128, 20),
}


def make(name):
    flags, B, n, nc = SETS[name]
    g = torch.Generator(device="cuda").manual_seed(1)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    th, ph = r(B, 256, n, n).requires_grad_(True), r(B, 256, n, n).requires_grad_(True)
    img, real = torch.rand(B, 3, 4 * n, 4 * n, device="cuda") * 2 - 1, torch.rand(B, 3, 4 * n, 4 * n, device="cuda") * 2 - 1
    lab = torch.randint(0, nc, (B, 1, 4 * n, 4 * n), device="cuda")
    seg = torch.zeros(B, nc, 4 * n, 4 * n, device="cuda").scatter_(1, lab, 1.0)
    cfg = HotPathConfig(PONO_C=True, down=4, isTrain=True, **flags)
    cot = {}

    def step():
        th.grad = ph.grad = None
        out = correspondence_hot_path(th, ph, img, real, seg, seg, cfg)
        keys = sorted(out)
        for k in keys:
            if k not in cot:
                cot[k] = torch.randn(out[k].shape, device="cuda", generator=g)
        torch.autograd.backward([out[k] for k in keys], [cot[k] for k in keys])
    return step


def window(step, seconds):
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            step()
        n += 5
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--sets", default=",".join(SETS))
    a = ap.parse_args()
    res = {}
    for name in a.sets.split(","):
        step = make(name)
        times, peak = {False: [], True: []}, {}
        for modes in (False, True):                  # warm both arms (code objects, workspace pools, allocator)
            ops.WARP_HEAD_MODES = modes
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            peak[modes] = torch.cuda.max_memory_allocated()
        for _ in range(a.rounds):
            for modes in (False, True):
                ops.WARP_HEAD_MODES = modes
                times[modes].append(window(step, a.window))
        ops.WARP_HEAD_MODES = True
        stats = {m: benchlib.summary(v) for m, v in times.items()}
        med = {m: s.median for m, s in stats.items()}
        res[name] = {
            "B": SETS[name][1], "grid": SETS[name][2],
            "framework_route_ms": round(med[False], 4), "new_route_ms": round(med[True], 4),
            "difference_ms": round(med[True] - med[False], 4),
            "spread_ms": {("new" if m else "framework"): round(s.max - s.min, 4) for m, s in stats.items()},
            "peak_MiB": {("new" if m else "framework"): round(p / 2 ** 20, 1) for m, p in peak.items()},
        }
        print(json.dumps({name: res[name]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
