"""Prepared-exemplar inference A/B (inference.prepare_exemplar): the whole NoVGGCorrespondence eval() forward under torch.no_grad()
at the ADE20k bench shape (256 x 256, B = 8, match_kernel 1 unless --match_kernel 3), after inference.freeze(), three arms
alternating run by run in one process:

  (a) no record — the ordinary forward(ref_img, real_img, seg_map, ref_seg_map);
  (b) a record with Be == B — forward(None, real_img, seg_map, None, exemplar=record);
  (c) a record with Be == 1 — ONE exemplar for all B inputs ((a) and (b) are fed that exemplar repeated B times, so the three arms
      compute the same thing).

Per arm: the median over `--runs` timed runs (device events around one forward) after `--warmup` runs of each arm, and the
entry-point calls per forward.  Writes a text table to --out (default: stdout only).

    python tools/exemplar_bench.py --runs 30 --warmup 5 --out profiles/exemplar_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cocosnet_amd import _lib, inference  # noqa: E402
from cocosnet_amd import correspondence as cc  # noqa: E402

DEV = torch.device("cuda", 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--match_kernel", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("exemplar_bench needs a GPU")
    B, S = args.batch, args.size
    opt = cc.ade20k_options(crop_size=S, match_kernel=args.match_kernel)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(DEV)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    report = inference.freeze(net)
    g = torch.Generator(device=DEV).manual_seed(1)
    nc = opt.semantic_nc
    lab = lambda n: torch.zeros(n, nc, S, S, device=DEV).scatter_(1, torch.randint(0, nc, (n, 1, S, S), device=DEV, generator=g), 1.0)
    ref1, ref_seg1 = torch.rand(1, 3, S, S, device=DEV, generator=g) * 2 - 1, lab(1)
    refB, ref_segB = ref1.expand(B, -1, -1, -1).contiguous(), ref_seg1.expand(B, -1, -1, -1).contiguous()
    real, seg = torch.rand(B, 3, S, S, device=DEV, generator=g) * 2 - 1, lab(B)
    with torch.no_grad():
        recB = inference.prepare_exemplar(net, refB, ref_segB)
        rec1 = inference.prepare_exemplar(net, ref1, ref_seg1)
    arms = {
        "(a) no record": lambda: net(refB, real, seg, ref_segB),
        "(b) record, Be == B": lambda: net(None, real, seg, None, exemplar=recB),
        "(c) record, Be == 1": lambda: net(None, real, seg, None, exemplar=rec1),
    }
    times = {k: [] for k in arms}
    outs = {}
    with torch.no_grad():
        for i in range(args.warmup + args.runs):
            for name, run in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                outs[name] = run()
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        calls = {}
        real_call = _lib.call
        for name, run in arms.items():
            n = [0]

            def counting(fn, *a, _n=n):
                _n[0] += 1
                return real_call(fn, *a)
            _lib.call = counting
            try:
                run()
            finally:
                _lib.call = real_call
            calls[name] = n[0]
    torch.cuda.synchronize()
    base = outs["(a) no record"]
    lines = [f"prepared-exemplar inference A/B on {torch.cuda.get_device_name(0)}: NoVGGCorrespondence eval() forward, ADE20k flags, "
             f"match_kernel {args.match_kernel}, B={B} {S}x{S}, after freeze() ({report}); medians over {args.runs} runs per arm after "
             f"{args.warmup} warm-up runs, arms alternating in one process"]
    med = {}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4)
        med[name] = statistics.median(ts)
        diff = max((outs[name][k] - base[k]).abs().max().item() for k in base)
        lines.append(f"  {name:22s} median {med[name]:8.3f} ms  (quartiles {q[0]:.3f} .. {q[2]:.3f}, {len(ts)} runs)   entry-point calls "
                     f"{calls[name]}   max |out - (a)| over the dictionary {diff:.3e}")
    a = med["(a) no record"]
    lines.append(f"  (b) / (a) = {med['(b) record, Be == B'] / a:.4f}   (c) / (a) = {med['(c) record, Be == 1'] / a:.4f}   "
                 f"(c) / (b) = {med['(c) record, Be == 1'] / med['(b) record, Be == B']:.4f}")
    lines.append(f"  repreparations: Be == B {recB.repreparations}, Be == 1 {rec1.repreparations}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
