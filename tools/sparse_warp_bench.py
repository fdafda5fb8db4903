"""K42 cost: forward + backward of the k-sparse warp (hot_path.correspondence_sparse) from raw theta / phi at the benchmark shape
(B = 8, 64 x 64 grid, match_kernel 1, PONO_C, the ADE20k value width 3 + 151 = 154) against the dense route a user would otherwise
train through (hot_path.correspondence_hot_path on the same inputs and flags).  The two compute DIFFERENT functions — a softmax over k
selected keys against one over all HW — so the table is a cost comparison, not a replacement claim.

Arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the rounds
(>= 20) after a warm-up:
    dense              correspondence_hot_path forward + backward (warp_out and warp_mask both receive a gradient)
    sparse k           correspondence_sparse(topk=k) forward + backward, the same cotangents
    key kernel hub k   cocos_sparse_softmax_warp_bwd_key_f16x3 alone on the table where EVERY query names key 0 in rank 0 (one wave
                       walks a list of HW entries: the worst case of the gather), and `key kernel topk k` on the selected table
plus the peak memory above the inputs of both routes and, when hipcc is at hand, the register figures of the K42 kernels.

    python tools/sparse_warp_bench.py [--out profiles/k42_sparse_warp.txt] [--rounds 21] [--window 0.05]
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

B, H, W, DOWN, NC, INV_T = 8, 64, 64, 4, 151, 100.0
KS = (1, 2, 4, 8)


def register_rows():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of plane_pair.hip from hipcc's kernel-resource-usage remarks;
    None without hipcc"""
    usage = benchlib.resource_usage("plane_pair.hip")
    if usage is None:
        return None
    return [(re.search(r"\d+([a-z_0-9]+_kernel)", u.name).group(1), u.vgprs, u.agprs, u.scratch, u.occupancy) for u in usage]


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k42_sparse_warp.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("sparse_warp_bench")
    from cocosnet_amd import _lib, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path, correspondence_sparse
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=DOWN, warp_mask_losstype="direct", isTrain=True)
    N = H * W
    g = torch.Generator(device=dev).manual_seed(1000 + N)
    theta = (torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1).requires_grad_(True)
    phi = (0.3 * theta.detach().roll((1, 7), (2, 3)) + torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05).requires_grad_(True)
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
    sparse = lambda k: step(lambda: correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=k))

    # the key-side kernel alone: ready planes, w / ds of the right shape, the inverse table of the selected and of the hub index table
    with torch.no_grad():
        flat = lambda t: t.detach().reshape(B, 256, N)
        qh, ql, _ = ops.center_l2norm_planes_fwd(flat(theta), 1)
        kh, kl, _ = ops.center_l2norm_planes_fwd(flat(phi), 1)
        dout_t = torch.randn(B, N, 3 + NC, device=dev, generator=g)
        dk_t = torch.empty(B, N, 256, device=dev)
        dv_t = torch.empty(B, N, 3 + NC, device=dev)
    key_arms = {}
    for k in KS:
        idx, _, _ = ops._corr_topk_planes(qh, ql, kh, kl, INV_T, k)
        hub = idx.clone()
        hub[:, :, 0] = 0
        w = torch.softmax(torch.randn(B, N, k, device=dev, generator=g), dim=-1)
        ds = torch.randn(B, N, k, device=dev, generator=g) * w
        for tag, table in (("topk", idx), ("hub", hub)):
            entries, offsets = ops._inverse_index_table(table, N)
            key_arms[f"key kernel {tag} {k}"] = lambda e=entries, o=offsets, w=w, ds=ds, k=k: _lib.call(
                "cocos_sparse_softmax_warp_bwd_key_f16x3", qh.data_ptr(), ql.data_ptr(), dout_t.data_ptr(), ds.data_ptr(), w.data_ptr(),
                e.data_ptr(), o.data_ptr(), dk_t.data_ptr(), dv_t.data_ptr(), B, 256, N, N, 3 + NC, k, INV_T, ops.SPLIT_OPERAND_SCALE,
                torch.cuda.current_stream().cuda_stream)

    arms = {"dense": dense}
    for k in KS:
        arms[f"sparse {k}"] = lambda k=k: sparse(k)
    arms.update(key_arms)

    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    theta.grad = phi.grad = None
    peaks = {"dense": benchlib.peak_bytes(dense)}
    for k in KS:
        theta.grad = phi.grad = None
        peaks[f"sparse {k}"] = benchlib.peak_bytes(lambda: sparse(k))

    lines = [f"# tools/sparse_warp_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {H} x {W} grid (HW = {N}), match_kernel 1, PONO_C, "
             f"warp_mask_losstype direct (Cv = {3 + NC}); one HW x HW fp32 matrix is {B * N * N * 4 / 2**20:.0f} MiB",
             f"# forward + backward from raw theta / phi, ms per call: median of {args.rounds} alternating windows of ~{args.window} s after "
             f"{args.warmup} warm-up calls (min .. max of the windows)",
             "# dense and sparse compute DIFFERENT functions (softmax over all HW keys / over the k selected ones): a cost comparison, not a replacement claim"]
    for name in arms:
        v = samples[name]
        pk = f"  peak above inputs {peaks[name] / 2**20:8.1f} MiB" if name in peaks else ""
        lines.append(f"{name:22s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window){pk}")
    lines.append("# ratios (medians)")
    for k in KS:
        lines.append(f"k = {k}: sparse / dense = {med[f'sparse {k}'] / med['dense']:.3f}   peak sparse / dense = "
                     f"{peaks[f'sparse {k}'] / peaks['dense']:.4f}   key kernel hub / topk = "
                     f"{med[f'key kernel hub {k}'] / med[f'key kernel topk {k}']:.2f}")
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:32s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
