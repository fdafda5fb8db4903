"""K53 cost: forward + backward of the match loss on the match_kernel-3 route (hot_path.correspondence_nll_box3) from raw theta / phi
at B = 8 on 64 x 64 and B = 1 on 128 x 128, against the materialised arm that computes the same loss, and the new kernel alone.
These are the kernel's first measurements: nothing here was tuned.

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up:
    nll box3           correspondence_nll_box3 (symmetric, unweighted) forward + backward
    materialised       the same loss from hot_path._box3_logits (K3 -> K6: the logits matrix in HBM), torch.logsumexp over both axes,
                       torch.gather at the target, nll_reduce; forward + backward through autograd
    lse_bwd rows       cocos_box3_lse_bwd_f16x3 alone, the row pass (writes G)
    lse_bwd cols+acc   the same entry with COCOS_BOX3_T_TRANSPOSED | COCOS_BOX3_G_ACCUMULATE (reads and rewrites G)
    match rows         context: cocos_box3_match_f16x3, the forward readout over the same T (reads T, writes nothing HW x HW)
plus the peak memory above the inputs of the two routes, the kernel's achieved rate against its compulsory traffic (T read once + G
written once, + G read once under ACCUMULATE; the two neighbour blocks of the y box are counted as cache hits) and, when hipcc is at
hand, the register figures.  The report is the cost section of profiles/k53_match_box3_nll.txt.

    python tools/match_box3_nll_bench.py [--shape 8x64 | 1x128 | both] [--out profiles/k53_match_box3_nll_bench.txt] [--rounds 21]
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

INV_T, KC = 100.0, 2304.0
SHAPES = {"8x64": (8, 64), "1x128": (1, 128)}


def register_rows():
    usage = benchlib.resource_usage("box3_lse_bwd_f16x3.hip")
    if usage is None:
        return None
    return [(re.search(r"\d+(box3_lse_[a-z_0-9]+_kernel)", u.name).group(1) + ("<chunked>" if "ILb1" in u.name else ""), u.vgprs, u.agprs,
             u.scratch, u.occupancy) for u in usage]


def bench_shape(B, H, args):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, _box3_logits, correspondence_nll_box3, nll_reduce
    dev = torch.device("cuda", 0)
    W, N = H, H * H
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=4, isTrain=True)
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = (torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1).requires_grad_(True)
    phi = (0.05 * theta.detach().roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05).requires_grad_(True)
    target = torch.randint(0, N, (B, H, W), device=dev, generator=g)
    target[:, 0, ::5] = -1
    tgt = target.reshape(B, N)

    def fused():
        theta.grad = phi.grad = None
        out = correspondence_nll_box3(theta, phi, target, cfg, 1.0 / INV_T)
        out["loss_match"].backward()
        return out["loss_match"]

    def materialised():
        theta.grad = phi.grad = None
        z = _box3_logits(theta, phi, INV_T)                                   # [B, N queries, N keys]
        row_lse, col_lse = torch.logsumexp(z, dim=2), torch.logsumexp(z, dim=1)
        tc = tgt.clamp_min(0)
        z_t = torch.gather(z, 2, tc.unsqueeze(2)).squeeze(2)
        sup, zero = tgt >= 0, torch.zeros((), device=dev)
        loss = nll_reduce(torch.where(sup, row_lse - z_t, zero), torch.where(sup, torch.gather(col_lse, 1, tc) - z_t, zero), tgt, None, True)
        loss.backward()
        return loss

    arms = {"nll box3": fused, "materialised": materialised}

    # the kernel alone: T, the statistics, the two lse vectors and every output ready
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        th, ph = theta.detach(), phi.detach()
        (mu, a), (nu, b) = ops.unfold3_stats(th, KC), ops.unfold3_stats(ph, KC)
        T = ops.box3_corr_xbox(th, ph)
        row = ops.box3_match(T, mu, a, nu, b, H, W, KC, INV_T)[2]
        col = ops.box3_match(T, nu, b, mu, a, H, W, KC, INV_T, transposed=True)[2]
        new = lambda *s: torch.empty(s, device=dev)
        G = torch.zeros(B * N * N, device=dev)
        g_row, g_col = torch.randn(B, N, device=dev, generator=g), torch.randn(B, N, device=dev, generator=g)
        dmu, da, dnu, db, gmax = new(B, N), new(B, N), new(B, N), new(B, N), new(1)
        colpart = new(_lib.load().cocos_box3_lse_bwd_colpart_bytes(B, N, N) // 4)
        idx, mx, lse = torch.empty(B, N, device=dev, dtype=torch.int32), new(B, N), new(B, N)
    p = lambda t: t.data_ptr()
    bwd = lambda q, k, l, gl, flags: _lib.call("cocos_box3_lse_bwd_f16x3", p(T), p(q[0]), p(q[1]), p(k[0]), p(k[1]), p(l), p(gl), p(G), p(dmu),
                                               p(da), p(dnu), p(db), p(colpart), p(gmax), B, N, N, H, W, KC, INV_T, flags, st)
    arms["lse_bwd rows"] = lambda: bwd((mu, a), (nu, b), row, g_row, 0)
    g_tiny = g_col * 1e-30                                                     # (G stays finite over many accumulating windows)
    arms["lse_bwd cols+acc"] = lambda: bwd((nu, b), (mu, a), col, g_tiny, 3)
    arms["match rows"] = lambda: _lib.call("cocos_box3_match_f16x3", p(T), p(mu), p(a), p(nu), p(b), p(idx), p(mx), p(lse), B, N, N, H, W, KC,
                                           INV_T, 0, st)

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {}
    for name in ("nll box3", "materialised"):
        theta.grad = phi.grad = None
        peaks[name] = benchlib.peak_bytes(arms[name])
    theta.grad = phi.grad = None

    hw = B * N * N * 4
    lines = [f"# B = {B}, {H} x {W} grid (HW = {N}), match_kernel 3, PONO_C; one HW x HW fp32 tensor (T or G) is {hw / 2**20:.0f} MiB"]
    for name in arms:
        s = benchlib.summary(samples[name])
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:18s} {s.median:9.4f} ms  ({s.min:.4f} .. {s.max:.4f}; spread {100 * s.spread:.1f} %; {counts[name]} calls per window){pk}")
    lines.append("# the new kernel against its compulsory traffic")
    for name, nbytes, what in (("lse_bwd rows", 2 * hw, "T read + G written"), ("lse_bwd cols+acc", 3 * hw, "T read + G read + G written"),
                               ("match rows", hw, "T read")):
        lines.append(f"{name:18s} {nbytes / 2**20:8.0f} MiB ({what}) in {med[name]:.4f} ms = {nbytes / med[name] / 1e6:7.0f} GB/s")
    lines.append(f"# ratios (medians): nll box3 / materialised = {med['nll box3'] / med['materialised']:.3f}   two lse_bwd passes / nll box3 = "
                 f"{(med['lse_bwd rows'] + med['lse_bwd cols+acc']) / med['nll box3']:.3f}   peak nll box3 / materialised = "
                 f"{peaks['nll box3'] / peaks['materialised']:.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k53_match_box3_nll_bench.txt"))
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["both"], default="both")
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_nll_bench")
    lines = [f"# tools/match_box3_nll_bench.py on {torch.cuda.get_device_name(0)}: ms per call, median of {args.rounds} alternating windows of "
             f"~{args.window} s after {args.warmup} warm-up calls (min .. max and spread of the windows)"]
    for name in (sorted(SHAPES, reverse=True) if args.shape == "both" else [args.shape]):
        lines += bench_shape(*SHAPES[name], args)
        torch.cuda.empty_cache()
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:40s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
