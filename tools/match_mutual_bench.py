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
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

INV_T = 100.0


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def register_table():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of corr_match_mutual_f16x3.hip and of the K = 1 readout it is compared
    with, from hipcc's kernel-resource-usage remarks; None without hipcc"""
    from cocosnet_amd import build
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        return None
    rows = []
    with tempfile.TemporaryDirectory(prefix="cocos_k48_") as tmp:
        for unit, keep in (("corr_match_mutual_f16x3.hip", None), ("corr_topk_f16x3.hip", "ILi1ELb0ELb0E")):
            cmd = [hipcc, *build.HIP_FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                   os.path.join(build.CSRC_DIR, unit), "-o", os.path.join(tmp, unit + ".o")]
            text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
            for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size", text, flags=re.S):
                if keep is not None and keep not in name:
                    continue
                get = lambda what: int(re.search(what + r"[^:\n]*: (\d+)", body).group(1))
                inst = re.search(r"kernelILi(\d+)ELb([01])ELb([01])E", name)
                tf = lambda c: "true" if c == "1" else "false"
                label = (f"corr_topk_f16x3_kernel<{inst.group(1)}, {tf(inst.group(2))}, {tf(inst.group(3))}>" if inst else
                         re.sub(r"^_ZN5cocos\d+", "", name).split("E", 1)[0])
                rows.append((label, get(r" VGPRs"), get("AGPRs"), get("ScratchSize"), get("Occupancy")))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "k48_match_mutual.txt"))
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default="8x64", help="B x grid side")
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("match_mutual_bench: the medians are over at least 20 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("match_mutual_bench: no GPU visible (a timing needs the device; there is no fallback)")
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
        counts = {}
        for name, fn in arms.items():            # warm-up of every arm, and the iteration count of its window
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            counts[name] = max(2, int(args.window * 1e3 / max(_time(fn, 2), 1e-3)))
        samples = {name: [] for name in arms}
        for _ in range(args.rounds):                 # alternating: one window of every arm per round
            for name, fn in arms.items():
                samples[name].append(_time(fn, counts[name]))
    med = {name: statistics.median(v) for name, v in samples.items()}
    for name in arms:
        v = samples[name]
        lines.append(f"{name:22s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; spread (max - min) / median = "
                     f"{(max(v) - min(v)) / med[name]:.4f}; {counts[name]} calls per window)")
    a, b = "(a) two readouts", "(b) fused + finish"
    spread = max(samples[a]) - min(samples[a])
    wins = med[a] - med[b] > spread
    lines.append(f"(b) / (a) = {med[b] / med[a]:.4f}   (a) - (b) = {med[a] - med[b]:+.4f} ms   spread of (a)'s windows = {spread:.4f} ms")
    lines.append(f"rule: MATCH_MUTUAL_FUSED defaults to True only if (a) - (b) > the spread of (a)'s windows -> {'True' if wins else 'False'}")

    table = register_table()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:44s} VGPRs {v:3d}  AGPRs {a_:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a_, s, o in table]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
