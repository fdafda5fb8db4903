"""K51 cost: forward + backward of the k-sparse warp on the match_kernel-3 route (hot_path.correspondence_sparse_box3) from raw theta /
phi against the dense route a user would otherwise train through (hot_path.correspondence_hot_path with match_kernel 3 on the same
inputs and flags), at B = 8 on 64 x 64 and B = 1 on 128 x 128 with the ADE20k value width 3 + 151 = 154.  The two compute DIFFERENT
functions — a softmax over k selected keys against one over all HW — so the table is a cost comparison, not a replacement claim.

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up:
    dense              correspondence_hot_path forward + backward (warp_out and warp_mask both receive a gradient)
    sparse k           correspondence_sparse_box3(topk=k) forward + backward, the same cotangents
    selection k        correspondence_match(topk=k) alone: what the sparse route spends before its warp (K12, the x-box GEMM, K41)
    fwd / pair / theta / key k     the four K51 kernels alone on the selected table
    key hub k          the key kernel on the table where EVERY query names key 0 in rank 0 (one wave walks a list of HW entries for up to
                       nine taps: the worst case of the gather)
plus the peak memory above the inputs of both routes and, when hipcc is at hand, the register figures of the K51 kernels.  The report is
the cost section of profiles/k51_match_box3_sparse.txt (whose first section holds the errors the GPU tests print).

    python tools/match_box3_sparse_bench.py [--shape 8x64 | 1x128 | both] [--out profiles/k51_match_box3_sparse_bench.txt] [--rounds 21]
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
KS = (1, 2, 4, 8)
K_ALONE = 4
SHAPES = {"8x64": (8, 64), "1x128": (1, 128)}


def register_rows():
    usage = benchlib.resource_usage("box3_pair.hip", keep=("box3_sparse_", "TopkSet"))      # this route's four of the unit's eight kernels
    if usage is None:
        return None
    return [(re.search(r"\d+(box3_[a-z_0-9]+_kernel)", u.name).group(1) + ("<TopkSet>" if "TopkSet" in u.name else ""), u.vgprs, u.agprs,
             u.scratch, u.occupancy) for u in usage]


def bench_shape(B, H, args):
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path, correspondence_match, correspondence_sparse_box3
    dev = torch.device("cuda", 0)
    W, N, Cv = H, H * H, 3 + NC
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=DOWN, warp_mask_losstype="direct", isTrain=True)
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

    def step(route):
        theta.grad = phi.grad = None
        out = route()
        torch.autograd.backward([out["warp_out"], out["warp_mask"]], [g_out, g_mask])

    dense = lambda: step(lambda: correspondence_hot_path(theta, phi, ref_img, real_img, seg, ref_seg, cfg))
    sparse = lambda k: step(lambda: correspondence_sparse_box3(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, k))
    arms = {"dense": dense}
    for k in KS:
        arms[f"sparse {k}"] = lambda k=k: sparse(k)
    arms[f"selection {K_ALONE}"] = lambda: correspondence_match(theta, phi, cfg, 1.0 / INV_T, topk=K_ALONE)

    # the four kernels alone at k = K_ALONE: ready rows, statistics, tables and outputs
    k = K_ALONE
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        th, ph = theta.detach(), phi.detach()
        th_t, ph_t = ops._transpose(th.reshape(B, 256, N)), ops._transpose(ph.reshape(B, 256, N))
        (mu, a), (nu, b) = ops.unfold3_stats(th, 2304.0), ops.unfold3_stats(ph, 2304.0)
        idx = correspondence_match(th, ph, cfg, 1.0 / INV_T, topk=k).index.reshape(B, k, N).permute(0, 2, 1).to(torch.int32).contiguous()
        hub = idx.clone()
        hub[:, :, 0] = 0
        new = lambda *s: torch.empty(s, device=dev)
        vt, dout_t = torch.randn(B, N, Cv, device=dev, generator=g), torch.randn(B, N, Cv, device=dev, generator=g)
        out_t, w, c, gg, hb = new(B, N, Cv), new(B, N, k), new(B, N, k), new(B, N, k), new(B, N, k)
        dmu, da, dnu, db, dth_t, dph_t, dv_t = new(B, N), new(B, N), new(B, N), new(B, N), new(B, N, 256), new(B, N, 256), new(B, N, Cv)
    p = lambda t: t.data_ptr()
    dims = (B, 256, H, W, H, W)
    fwd = lambda: _lib.call("cocos_box3_sparse_softmax_warp_fwd", p(th_t), p(ph_t), p(mu), p(a), p(nu), p(b), p(vt), p(idx), p(out_t), p(w),
                            p(c), *dims, Cv, k, INV_T, st)
    pair = lambda: _lib.call("cocos_box3_sparse_softmax_warp_bwd_pair", p(vt), p(dout_t), p(idx), p(w), p(c), p(a), p(nu), p(b), p(gg), p(hb),
                             p(dmu), p(da), *dims, Cv, k, INV_T, st)
    tht = lambda: _lib.call("cocos_box3_sparse_softmax_warp_bwd_theta", p(ph_t), p(idx), p(gg), p(dth_t), *dims, k, st)

    def key_arm(table):
        entries, offsets = ops._inverse_index_table(table, N)
        return lambda: _lib.call("cocos_box3_sparse_softmax_warp_bwd_key", p(th_t), p(dout_t), p(gg), p(hb), p(w), p(mu), p(entries), p(offsets),
                                 p(dph_t), p(dv_t), p(dnu), p(db), *dims, Cv, k, st)

    fwd(), pair()      # w, c, g and hb hold real values when the gradient kernels are timed
    arms.update({f"fwd {k}": fwd, f"pair {k}": pair, f"theta {k}": tht, f"key {k}": key_arm(idx), f"key hub {k}": key_arm(hub)})

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    theta.grad = phi.grad = None
    peaks = {"dense": benchlib.peak_bytes(dense)}
    for kk in KS:
        theta.grad = phi.grad = None
        peaks[f"sparse {kk}"] = benchlib.peak_bytes(lambda: sparse(kk))
    theta.grad = phi.grad = None

    lines = [f"# B = {B}, {H} x {W} grid (HW = {N}), match_kernel 3, PONO_C, warp_mask_losstype direct (Cv = {Cv}); one HW x HW fp32 tensor "
             f"(T) is {B * N * N * 4 / 2**20:.0f} MiB; fused selection: {ops.box3_fused_ok(B, 256, H, W) and ops.box3_topk_ok(K_ALONE)}"]
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:14s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    lines.append("# ratios (medians)")
    for kk in KS:
        lines.append(f"k = {kk}: sparse / dense = {med[f'sparse {kk}'] / med['dense']:.3f}   peak sparse / dense = "
                     f"{peaks[f'sparse {kk}'] / peaks['dense']:.4f}")
    lines.append(f"k = {k}: selection / sparse = {med[f'selection {k}'] / med[f'sparse {k}']:.3f}   four kernels / sparse = "
                 f"{sum(med[f'{n} {k}'] for n in ('fwd', 'pair', 'theta', 'key')) / med[f'sparse {k}']:.3f}   key hub / key = "
                 f"{med[f'key hub {k}'] / med[f'key {k}']:.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k51_match_box3_sparse_bench.txt"))
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["both"], default="both")
    args = ap.parse_args()
    benchlib.require_gpu("match_box3_sparse_bench")
    lines = [f"# tools/match_box3_sparse_bench.py on {torch.cuda.get_device_name(0)}: forward + backward from raw theta / phi, ms per call: "
             f"median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls (min .. max of the windows)",
             "# dense and sparse compute DIFFERENT functions (softmax over all HW keys / over the k selected ones): a cost table, not a replacement claim"]
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
