"""K52 cost: forward + backward of the sub-cell flow warp on the match_kernel-3 route (hot_path.correspondence_flow_box3) from raw
theta / phi at B = 8 on 64 x 64 and B = 1 on 128 x 128, for r = 1, 2, 3.  These are the kernels' first measurements: nothing here was
tuned, and the window kernels do not stage the (2 r + 3)^2 distinct phi rows of a window (the cache serves the repeats).

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up:
    flow r             correspondence_flow_box3(radius=r) forward + backward (warp_out and match_offset both receive a gradient)
    sparse 4           context: correspondence_sparse_box3(topk=4) forward + backward (K51; a DIFFERENT function)
    dense              context: correspondence_hot_path with match_kernel 3 forward + backward (a DIFFERENT function)
    selection          correspondence_match alone: what the flow route spends before its refinement (K12, the x-box GEMM, K37)
    fwd / pair / theta / key r     the four K52 kernels alone on the selected centres
    key hub r          the key kernel on the table where EVERY query names key 0 (one list of HW entries, walked for up to 9 W pairs)
plus the peak memory above the inputs and, when hipcc is at hand, the register figures of the K52 kernels.  The report is the cost
section of profiles/k52_match_box3_flow.txt (whose first section holds the errors the GPU tests print).

    python tools/match_box3_flow_bench.py [--shape 8x64 | 1x128 | both] [--out profiles/k52_match_box3_flow_bench.txt] [--rounds 21]
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

DOWN, NC, INV_T = 4, 151, 100.0
RADII = (1, 2, 3)
SHAPES = {"8x64": (8, 64), "1x128": (1, 128)}


def register_rows():
    usage = benchlib.resource_usage("box3_pair.hip", keep=("box3_refine_", "WindowSet"))      # this route's four of the unit's eight kernels
    if usage is None:
        return None
    return [(re.search(r"\d+(box3_[a-z_0-9]+_kernel)", u.name).group(1) + ("<WindowSet>" if "WindowSet" in u.name else ""), u.vgprs, u.agprs,
             u.scratch, u.occupancy) for u in usage]


def bench_shape(B, H, args):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import (HotPathConfig, correspondence_flow_box3, correspondence_hot_path, correspondence_match,
                                       correspondence_sparse_box3)
    dev = torch.device("cuda", 0)
    W, N = H, H * H
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=DOWN, isTrain=True)
    cfg_mask = HotPathConfig(match_kernel=3, PONO_C=True, down=DOWN, warp_mask_losstype="direct", isTrain=True)
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = (torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1).requires_grad_(True)
    phi = (0.05 * theta.detach().roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05).requires_grad_(True)
    ref_img = torch.rand(B, 3, H * DOWN, W * DOWN, device=dev, generator=g) * 2 - 1
    real_img = torch.rand(B, 3, H * DOWN, W * DOWN, device=dev, generator=g) * 2 - 1
    onehot = lambda: torch.zeros(B, NC, H * DOWN, W * DOWN, device=dev).scatter_(
        1, torch.randint(0, NC, (B, 1, H * DOWN, W * DOWN), device=dev, generator=g), 1.0)
    seg, ref_seg = onehot(), onehot()
    g_out = torch.randn(B, 3, H * DOWN, W * DOWN, device=dev, generator=g)
    g_mask = torch.randn(B, NC, H, W, device=dev, generator=g)
    g_off = torch.randn(B, 2, H, W, device=dev, generator=g)

    def step(route, outs, grads):
        theta.grad = phi.grad = None
        out = route()
        torch.autograd.backward([out[n] for n in outs], grads)

    flow = lambda r: step(lambda: correspondence_flow_box3(theta, phi, ref_img, cfg, 1.0 / INV_T, radius=r), ("warp_out", "match_offset"),
                          [g_out, g_off])
    sparse = lambda: step(lambda: correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg_mask, 1.0 / INV_T, 4),
                          ("warp_out", "warp_mask"), [g_out, g_mask])
    dense = lambda: step(lambda: correspondence_hot_path(theta, phi, ref_img, real_img, seg, ref_seg, cfg_mask), ("warp_out", "warp_mask"),
                         [g_out, g_mask])
    arms = {f"flow {r}": (lambda r=r: flow(r)) for r in RADII}
    arms.update({"sparse 4": sparse, "dense": dense, "selection": lambda: correspondence_match(theta, phi, cfg, 1.0 / INV_T)})

    # the four kernels alone: ready rows, statistics, tables and outputs
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        th, ph = theta.detach(), phi.detach()
        th_t, ph_t = ops._transpose(th.reshape(B, 256, N)), ops._transpose(ph.reshape(B, 256, N))
        (mu, a), (nu, b) = ops.unfold3_stats(th, 2304.0), ops.unfold3_stats(ph, 2304.0)
        idx = correspondence_match(th, ph, cfg, 1.0 / INV_T).index.reshape(B, N).to(torch.int32).contiguous()
        hub = torch.zeros_like(idx)
        new = lambda *s: torch.empty(s, device=dev)
        doff = torch.randn(B, N, 2, device=dev, generator=g)
        off, lse, dmu, da, dnu, db, dth_t, dph_t = new(B, N, 2), new(B, N), new(B, N), new(B, N), new(B, N), new(B, N), new(B, N, 256), new(B, N, 256)
        tables = {"": ops._inverse_index_table(idx.view(B, N, 1), N), " hub": ops._inverse_index_table(hub.view(B, N, 1), N)}
    p = lambda t: t.data_ptr()
    dims = (B, 256, H, W, H, W)
    for r in RADII:
        slots = (2 * r + 1) ** 2
        c, gg, hb = new(B, N, slots), new(B, N, slots), new(B, N, slots)
        fwd = lambda r=r, c=c: _lib.call("cocos_box3_match_refine_fwd", p(th_t), p(ph_t), p(mu), p(a), p(nu), p(b), p(idx), p(off), p(lse), p(c),
                                         *dims, r, INV_T, st)
        pair = lambda r=r, c=c, gg=gg, hb=hb: _lib.call("cocos_box3_match_refine_bwd_pair", p(idx), p(c), p(a), p(nu), p(b), p(doff), p(gg), p(hb),
                                                        p(dmu), p(da), *dims, r, INV_T, st)
        tht = lambda r=r, gg=gg: _lib.call("cocos_box3_match_refine_bwd_theta", p(ph_t), p(idx), p(gg), p(dth_t), *dims, r, st)
        key = lambda t, r=r, gg=gg, hb=hb: _lib.call("cocos_box3_match_refine_bwd_key", p(th_t), p(gg), p(hb), p(mu), p(tables[t][0]),
                                                     p(tables[t][1]), p(dph_t), p(dnu), p(db), *dims, r, st)
        fwd(), pair()      # c, g and hb hold real values when the gradient kernels are timed
        arms.update({f"fwd {r}": fwd, f"pair {r}": pair, f"theta {r}": tht, f"key {r}": lambda key=key: key(""),
                     f"key hub {r}": lambda key=key: key(" hub")})

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    peaks = {}
    for name in [f"flow {r}" for r in RADII] + ["sparse 4", "dense"]:
        theta.grad = phi.grad = None
        peaks[name] = benchlib.peak_bytes(arms[name])
    theta.grad = phi.grad = None

    lines = [f"# B = {B}, {H} x {W} grid (HW = {N}), match_kernel 3, PONO_C; one HW x HW fp32 tensor (T) is {B * N * N * 4 / 2**20:.0f} MiB; "
             f"fused selection: {ops.box3_fused_ok(B, 256, H, W)}"]
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:14s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    lines.append("# ratios (medians)")
    for r in RADII:
        lines.append(f"r = {r}: flow / dense = {med[f'flow {r}'] / med['dense']:.3f}   flow / sparse 4 = {med[f'flow {r}'] / med['sparse 4']:.3f}   "
                     f"selection / flow = {med['selection'] / med[f'flow {r}']:.3f}   four kernels / flow = "
                     f"{sum(med[f'{n} {r}'] for n in ('fwd', 'pair', 'theta', 'key')) / med[f'flow {r}']:.3f}   key hub / key = "
                     f"{med[f'key hub {r}'] / med[f'key {r}']:.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k52_match_box3_flow_bench.txt"))
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["both"], default="both")
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_flow_bench")
    lines = [f"# tools/match_box3_flow_bench.py on {torch.cuda.get_device_name(0)}: forward + backward from raw theta / phi, ms per call: "
             f"median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)",
             "# flow, sparse and dense compute DIFFERENT functions: a cost table of first measurements, not a replacement claim"]
    for name in (sorted(SHAPES, reverse=True) if args.shape == "both" else [args.shape]):
        lines += bench_shape(*SHAPES[name], args)
        torch.cuda.empty_cache()
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:32s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
