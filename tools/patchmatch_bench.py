"""K43 cost and recall: the PatchMatch candidate selector (ops.patchmatch_topk behind hot_path.correspondence_sparse(search="patchmatch"))
against the dense scan (ops.corr_topk, K39a) it stands next to, at k = 4.

Timing arms per shape, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median
over the rounds (>= 20) after a warm-up:
    select dense        ops.corr_topk on the full-grid operand planes
    select patchmatch   the whole PatchMatch selection on the same planes: coarse start (2 x 2 pooling, K1 planes of the pooled
                        features, dense top-k at the half grid, expansion) + the default iterations
    pm iterations       the default iterations alone, from a ready start table
    pm one step         one launch (stride 1) of the default search
    sparse dense / sparse patchmatch    correspondence_sparse forward + backward from raw theta / phi with either selector
Recall of the PatchMatch candidates against the dense top-k on the same planes (recall@1: the dense best key is PatchMatch's rank 0;
recall@k: the share of the dense k keys PatchMatch returns), per iteration count, from the coarse and from the random start, on the
theta / phi of a randomly initialised network and on a planted translation plus noise.

    python tools/patchmatch_bench.py [--out profiles/k43_patchmatch.txt] [--rounds 21] [--window 0.05] [--shapes 8x64,1x128,1x256]
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

DOWN, NC, INV_T, K = 4, 151, 100.0, 4
SCHEDULE = (1, 2, 1, 1, 2, 1)      # recall is reported for every prefix of this list of strides


def register_rows():
    """[(kernel, VGPRs, AGPRs, scratch bytes / lane, waves / SIMD)] of patchmatch_f16x3.hip from hipcc's kernel-resource-usage remarks;
    None without hipcc"""
    usage = benchlib.resource_usage("patchmatch_f16x3.hip")
    if usage is None:
        return None
    rows = []
    for u in usage:
        inst = re.search(r"kernelILi(\d+)E", u.name)
        rows.append((f"patchmatch_step_kernel<{inst.group(1) if inst else '?'}>", u.vgprs, u.agprs, u.scratch, u.occupancy))
    return rows


def _recall(pm, dense):
    """(recall@1, recall@k) of pm [B,N,k] against dense [B,N,k]"""
    r1 = (pm[:, :, 0] == dense[:, :, 0]).float().mean().item()
    rk = (pm.unsqueeze(3) == dense.unsqueeze(2)).any(dim=2).float().mean().item()
    return r1, rk


def recall_lines(tag, theta, phi, ops, hot_path):
    """recall per iteration count from both starts, default search radii"""
    B, _, h, w = theta.shape
    flat = lambda t: t.detach().reshape(B, 256, h * w)
    d = ops.PATCHMATCH_DEFAULTS
    with torch.no_grad():
        planes = ops.OperandPlanes()
        qn = ops.center_l2norm_planes(flat(theta), 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(flat(phi), 1, planes, want_chan=False)
        dense = ops.corr_topk(qn, kn, INV_T, K, planes)[0]
        coarse = hot_path._patchmatch_coarse_init(theta.detach(), phi.detach(), INV_T, K)
        lines = [f"# recall, {tag}: B = {B}, {h} x {w} grid, k = {K}; strides = prefix of {SCHEDULE}, seed {d['seed']}"]
        starts = [("coarse start", coarse, (d["radii"], d["radius0"])), ("random start", "random", (d["radii"], max(h, w) // 2))]
        for name, init, radii in starts:
            if isinstance(init, str) and name == "coarse start":
                lines.append(f"{name}: the half grid is out of the dense readout's reach at this shape")
                continue
            cells = []
            if not isinstance(init, str):
                cells.append("0 it: %.3f / %.3f" % _recall(init.to(torch.int32), dense))
            for n in range(1, len(SCHEDULE) + 1):
                pm = ops.patchmatch_topk(qn, kn, INV_T, K, ((h, w), (h, w)), init, SCHEDULE[:n], radii, d["seed"], planes)[0]
                cells.append("%d it: %.3f / %.3f" % ((n,) + _recall(pm, dense)))
            lines.append(f"{name} (radii {radii[0]} from {radii[1]}), recall@1 / recall@{K}:  " + "   ".join(cells))
    return lines


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k43_patchmatch.txt"))
    ap.add_argument("--shapes", default="8x64,1x128,1x256", help="comma-separated B x grid side")
    args = ap.parse_args()
    benchlib.require_gpu("patchmatch_bench")
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import hot_path, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_sparse
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=1, PONO_C=True, down=DOWN, warp_mask_losstype="direct", isTrain=True)
    d = ops.PATCHMATCH_DEFAULTS
    lines = [f"# tools/patchmatch_bench.py on {torch.cuda.get_device_name(0)}: k = {K}, match_kernel 1, PONO_C, warp_mask_losstype direct "
             f"(Cv = {3 + NC}); PatchMatch defaults: strides {d['strides']}, radii {d['radii']} from {d['radius0']}, seed {d['seed']}",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)"]

    for shape in args.shapes.split(","):
        B, side = (int(v) for v in shape.split("x"))
        H = W = side
        N = H * W
        g = torch.Generator(device=dev).manual_seed(1000 + N)
        theta = (torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1).requires_grad_(True)
        phi = (theta.detach().roll((3, -5), (2, 3)) + 0.5 * torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05).requires_grad_(True)
        lines.append(f"## B = {B}, {H} x {W} grid (HW = {N}); dense scan: {N * N * 256 * B / 1e9:.1f} G multiply-adds, one PatchMatch "
                     f"step: {B * N * K * (5 + d['radii']) * 256 / 1e9:.3f} G")
        if not ops.corr_split_ok(B, 256, N, N, 1, False):
            lines.append("the dense readout does not take this shape")
            continue
        ref_img = torch.rand(B, 3, H * DOWN, W * DOWN, device=dev, generator=g) * 2 - 1
        onehot = lambda: torch.zeros(B, NC, H * DOWN, W * DOWN, device=dev).scatter_(
            1, torch.randint(0, NC, (B, 1, H * DOWN, W * DOWN), device=dev, generator=g), 1.0)
        seg, ref_seg = onehot(), onehot()
        g_out = torch.randn(B, 3, H * DOWN, W * DOWN, device=dev, generator=g)
        g_mask = torch.randn(B, NC, H, W, device=dev, generator=g)
        with torch.no_grad():
            planes = ops.OperandPlanes()
            flat = lambda t: t.detach().reshape(B, 256, N)
            qn = ops.center_l2norm_planes(flat(theta), 1, planes, want_chan=False)
            kn = ops.center_l2norm_planes(flat(phi), 1, planes, want_chan=False)
            start = hot_path._patchmatch_coarse_init(theta.detach(), phi.detach(), INV_T, K)
        grids = ((H, W), (H, W))
        radii = (d["radii"], d["radius0"])

        def sparse(search):
            theta.grad = phi.grad = None
            out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, topk=K, search=search)
            torch.autograd.backward([out["warp_out"], out["warp_mask"]], [g_out, g_mask])

        def select_pm():
            with torch.no_grad():
                init = hot_path._patchmatch_coarse_init(theta.detach(), phi.detach(), INV_T, K)
                ops.patchmatch_topk(qn, kn, INV_T, K, grids, init, d["strides"], radii, d["seed"], planes)

        arms = {"select dense": lambda: ops.corr_topk(qn, kn, INV_T, K, planes),
                "select patchmatch": select_pm,
                "pm iterations": lambda: ops.patchmatch_topk(qn, kn, INV_T, K, grids, start, d["strides"], radii, d["seed"], planes),
                "pm one step": lambda: ops.patchmatch_topk(qn, kn, INV_T, K, grids, start, (1,), radii, d["seed"], planes),
                "sparse dense": lambda: sparse("dense"),
                "sparse patchmatch": lambda: sparse("patchmatch")}
        counts = {}
        try:
            for name, fn in arms.items():            # one arm at a time: a refusal below names its arm
                counts.update(benchlib.window_counts({name: fn}, args.window, args.warmup))
        except (ValueError, ops._lib.CocosHipError) as e:      # a shape one of the routes refuses: said, not timed
            lines.append(f"{name}: refused at this shape: {e}")
            continue
        samples = benchlib.alternating(arms, counts, args.rounds)
        med = {name: statistics.median(v) for name, v in samples.items()}
        for name in arms:
            v = samples[name]
            lines.append(f"{name:20s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window)")
        lines.append(f"ratios (medians): select patchmatch / dense = {med['select patchmatch'] / med['select dense']:.3f}   "
                     f"sparse patchmatch / dense = {med['sparse patchmatch'] / med['sparse dense']:.3f}")
        lines += recall_lines("planted translation (3, -5) + noise 0.5", theta, phi, ops, hot_path)
        del seg, ref_seg, g_mask, g_out, ref_img
        torch.cuda.empty_cache()

    # theta / phi of a randomly initialised network at a 256 x 256 crop (a 64 x 64 grid)
    opt = cc.ade20k_options(crop_size=256, semantic_nc=NC, match_kernel=1)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(dev)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    g = torch.Generator(device=dev).manual_seed(4)
    onehot = lambda: torch.zeros(2, NC, 256, 256, device=dev).scatter_(1, torch.randint(0, NC, (2, 1, 256, 256), device=dev, generator=g), 1.0)
    ref_img, real = (torch.rand(2, 3, 256, 256, device=dev, generator=g) * 2 - 1 for _ in range(2))
    with torch.no_grad():
        theta_raw, phi_raw = net.project(ref_img, real, onehot(), onehot(), {}, lazy=True)
        lines += recall_lines("theta / phi of a randomly initialised network (ade20k options, 256 x 256 crop)", theta_raw.raw(), phi_raw.raw(),
                              ops, hot_path)

    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:28s} VGPRs {v:3d}  AGPRs {a:3d}  scratch {s} B/lane  waves/SIMD {o}" for name, v, a, s, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
