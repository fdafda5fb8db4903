"""The measurement protocol of the kernel benches under tools/, once.  A bench stays a script: its main() builds its own arms (a dict
name -> callable) and formats its own report; what it shares with the others is here.

    time_calls      HIP events around n calls on the current stream -> ms per call
    peak_bytes      torch's max_memory_allocated above the live memory over one call
    window_counts   warm every arm up, then size its timed window: calls per window of ~window_s seconds
    alternating     one window of every arm per round, in the arms' order, so that drift and neighbours hit all arms alike
    summary         median, min, max and the spread (max - min) / median of an arm's windows
    resource_usage  registers, scratch and occupancy of a translation unit's kernels, from hipcc's kernel-resource-usage remarks
    common_args, require_gpu, write_report      the argument block, the refusal without a device, the closing print-and-write
"""
import collections
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

Summary = collections.namedtuple("Summary", "median min max spread")
#: one kernel of a translation unit: the mangled name, then integers (scratch in bytes per lane, occupancy in waves per SIMD)
KernelResources = collections.namedtuple("KernelResources", "name vgprs agprs scratch occupancy sgprs")


def time_calls(fn, n):
    """ms per call of n calls of fn between two events on the current stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def peak_bytes(fn):
    """bytes fn allocates at its peak above what was live before it (its result is alive while the peak is read)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def window_counts(arms, window_s, warmup, probe=2):
    """{name: calls per timed window}: `warmup` calls of every arm, then `probe` timed calls size a window of ~window_s seconds
    (never fewer than `probe` calls)"""
    counts = {}
    for name, fn in arms.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        counts[name] = max(probe, int(window_s * 1e3 / max(time_calls(fn, probe), 1e-3)))
    return counts


def alternating(arms, counts, rounds):
    """{name: [ms per call of each window]}: one window of every arm per round, in the arms' order"""
    samples = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            samples[name].append(time_calls(fn, counts[name]))
    return samples


def summary(ms):
    med = statistics.median(ms)
    return Summary(med, min(ms), max(ms), (max(ms) - min(ms)) / med)


def find_hipcc():
    return next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)


def resource_usage(unit, keep=None):
    """[KernelResources] of the kernels of csrc/<unit>, in the compiler's order, from a device-only compile with the library's own flags
    (a few seconds); with `keep` (strings), only the kernels whose mangled name contains one of them.  None without hipcc."""
    from cocosnet_amd import build
    hipcc = find_hipcc()
    if hipcc is None:
        return None
    with tempfile.TemporaryDirectory(prefix="cocos_bench_") as tmp:
        cmd = [hipcc, *build.HIP_FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(build.CSRC_DIR, unit), "-o", os.path.join(tmp, unit + ".o")]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    rows = []
    for name, body in re.findall(r"Function Name: (\S+)(.*?)LDS Size", text, flags=re.S):
        if keep is not None and not any(k in name for k in keep):
            continue
        get = lambda what: int(re.search(what + r"[^:\n]*: (\d+)", body).group(1))
        rows.append(KernelResources(name, get(r" VGPRs"), get("AGPRs"), get("ScratchSize"), get("Occupancy"), get("TotalSGPRs")))
    return rows


def common_args(parser, default_out, min_rounds=20, rounds=21, window=0.05):
    """--out, --rounds, --window and --warmup; a --rounds below min_rounds ends the program, named after parser.prog"""
    tool = os.path.splitext(os.path.basename(parser.prog))[0]

    def rounds_arg(text):
        n = int(text)
        if n < min_rounds:
            raise SystemExit(f"{tool}: the medians are over at least {min_rounds} rounds")
        return n

    parser.add_argument("--out", default=default_out)
    parser.add_argument("--rounds", type=rounds_arg, default=rounds)
    parser.add_argument("--window", type=float, default=window, help="seconds of work per timed window")
    parser.add_argument("--warmup", type=int, default=3)


def require_gpu(tool_name):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool_name}: no GPU visible (a timing needs the device; there is no fallback)")


def write_report(lines, out_path):
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print("wrote", out_path)
