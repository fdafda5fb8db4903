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
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = ((8, 64, 64), (1, 128, 128))
INV_T, KC = 100.0, 2304.0
KS = (2, 4, 8)


def _time(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def register_table():
    """[(K, chunked, VGPRs, AGPRs, SGPRs, scratch bytes / lane, LDS bytes, waves / SIMD)] of every box3_topk_kernel instantiation (K = 1
    is K37) from hipcc's kernel-resource-usage remarks (device code only); None without hipcc.  LDS is dynamic: the report says 0."""
    from cocosnet_amd import build
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        return None
    rows = []
    with tempfile.TemporaryDirectory(prefix="cocos_k41_") as tmp:
        unit = "box3_fused_f16x3.hip"
        cmd = [hipcc, *build.HIP_FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(build.CSRC_DIR, unit), "-o", os.path.join(tmp, unit + ".o")]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        for name, body in re.findall(r"Function Name: (\S*box3_topk_kernel\S*)(.*?)LDS Size[^:\n]*: (?:\d+)", text, flags=re.S):
            get = lambda what: int(re.search(what + r"[^:\n]*: (\d+)", body).group(1))
            k, chunked = re.search(r"kernelILi(\d+)ELb([01])E", name).groups()
            rows.append((int(k), int(chunked), get(r" VGPRs"), get("AGPRs"), get("TotalSGPRs"), get("ScratchSize"), get("Occupancy")))
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

    counts = {}
    for name, fn in arms.items():                # warm-up of every arm, and the iteration count of its window
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        counts[name] = max(2, int(args.window * 1e3 / max(_time(fn, 2), 1e-3)))
    samples = {name: [] for name in arms}
    for _ in range(args.rounds):                 # alternating: one window of every arm per round
        for name, fn in arms.items():
            samples[name].append(_time(fn, counts[name]))
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {"k37": _peak(lambda: match(True, 1))}
    for k in KS:
        peaks[f"k41 {k}"] = _peak(lambda: match(True, k))
        peaks[f"chain {k}"] = _peak(lambda: match(False, k))
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
    ap.add_argument("--out", default=os.path.join("profiles", "k41_match_box3_topk.txt"))
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--window", type=float, default=0.05, help="seconds of work per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.rounds < 20:
        raise SystemExit("match_box3_topk_bench: the medians are over at least 20 rounds")
    if not torch.cuda.is_available():
        raise SystemExit("match_box3_topk_bench: no GPU visible (a timing needs the device; there is no fallback)")
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
    table = register_table()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, __launch_bounds__(256, 2); the budget at 2 waves per SIMD is 256 "
                 "VGPRs + AGPRs; LDS is dynamic: 8 Nk bytes of statistics, 32 KiB in the chunked flavour, + 18 KiB transposed)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{'K37 (K = 1)' if k == 1 else f'K41 K = {k}':12s} {'chunked' if c else 'whole  '}  VGPRs {v:3d}  AGPRs {ag:3d}  SGPRs {sg:3d}  "
                  f"scratch {s} B/lane  waves/SIMD {o}" for k, c, v, ag, sg, s, o in table]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
