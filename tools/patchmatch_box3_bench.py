"""K57 cost and recall: the PatchMatch candidate selector of the match_kernel-3 route (ops.patchmatch_topk_box3 behind
hot_path.correspondence_sparse_box3(search="patchmatch")) against the dense box readout (hot_path.correspondence_match(topk=k): K41 on
the x-box tensor T) it stands next to, at k = 4.

Timing arms per shape, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median
over the rounds after a warm-up:
    select dense        correspondence_match(topk=k) on raw theta / phi (the statistics, T and the readout)
    select patchmatch   the whole PatchMatch selection from raw theta / phi: the K12 statistics, the coarse start, the row transposes
                        and the default iterations
    pm one step         one launch (stride 1) of the default search on ready rows
    sparse dense / sparse patchmatch    correspondence_sparse_box3 forward + backward from raw theta / phi with either selector
At a shape the dense readout does not take (256 x 256: one T is 16 GiB per image) the dense arms are not run: the size of T and the
refusal are reported as numbers, and the peak memory growth of the patchmatch forward + backward is measured.
Recall of the PatchMatch candidates against the dense top-k (recall@1: the dense best key is PatchMatch's rank 0; recall@k: the share
of the dense k keys PatchMatch returns), per iteration count, on a planted translation plus noise and on the theta / phi of a randomly
initialised network.

    python tools/patchmatch_box3_bench.py [--out profiles/k57_patchmatch_box3.txt] [--rounds 21] [--window 0.05] [--shapes 8x64,1x128,1x256]
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
KC = 9 * 256.0
SCHEDULE = (1, 2, 1, 1, 2, 1)      # recall is reported for every prefix of this list of strides
DENSE_T_LIMIT = 4 << 30             # the dense arms are run only where one T stays below this many bytes


def register_rows():
    """[(kernel, VGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of patchmatch_box3.hip from hipcc's kernel-resource-usage remarks;
    None without hipcc"""
    usage = benchlib.resource_usage("patchmatch_box3.hip")
    if usage is None:
        return None
    rows = []
    for u in usage:
        inst = re.search(r"kernelILi(\d+)E", u.name)
        rows.append((f"patchmatch_step_box3_kernel<{inst.group(1) if inst else '?'}>", u.vgprs, getattr(u, "sgprs", -1), u.scratch, u.occupancy))
    return rows


def _recall(pm, dense):
    r1 = (pm[:, :, 0] == dense[:, :, 0]).float().mean().item()
    rk = (pm.unsqueeze(3) == dense.unsqueeze(2)).any(dim=2).float().mean().item()
    return r1, rk


def recall_lines(tag, theta, phi, cfg, ops, hot_path):
    """recall per iteration count from the route's own start, default search radii"""
    B, _, h, w = theta.shape
    d = ops.PATCHMATCH_DEFAULTS
    with torch.no_grad():
        theta, phi = theta.detach(), phi.detach()
        m = hot_path.correspondence_match(theta, phi, cfg, 1.0 / INV_T, topk=K)
        dense = m.index.reshape(B, K, h * w).permute(0, 2, 1).to(torch.int32)
        del m
        stats = (*ops.unfold3_stats(theta, KC), *ops.unfold3_stats(phi, KC))
        init = hot_path._patchmatch_coarse_init_box3(theta, phi, cfg, 1.0 / INV_T, K)
        lines = [f"# recall, {tag}: B = {B}, {h} x {w} grid, k = {K}; strides = prefix of {SCHEDULE}, seed {d['seed']}"]
        radii = (d["radii"], d["radius0"]) if not isinstance(init, str) else (d["radii"], max(h, w) // 2)
        name = "random start" if isinstance(init, str) else f"coarse start ({hot_path._patchmatch_coarse_route_box3(B, 256, h, w, h, w, K)})"
        cells = []
        if not isinstance(init, str):
            cells.append("0 it: %.3f / %.3f" % _recall(init.to(torch.int32), dense))
        for n in range(1, len(SCHEDULE) + 1):
            pm = ops.patchmatch_topk_box3(theta, phi, *stats, INV_T, K, init, SCHEDULE[:n], radii, d["seed"])[0]
            cells.append("%d it: %.3f / %.3f" % ((n,) + _recall(pm, dense)))
        lines.append(f"{name} (radii {radii[0]} from {radii[1]}), recall@1 / recall@{K}:  " + "   ".join(cells))
    return lines


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k57_patchmatch_box3.txt"))
    ap.add_argument("--shapes", default="8x64,1x128,1x256", help="comma-separated B x grid side")
    args = ap.parse_args()
    benchlib.require_gpu("patchmatch_box3_bench")
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd import hot_path, ops
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_match, correspondence_sparse_box3
    dev = torch.device("cuda", 0)
    cfg = HotPathConfig(match_kernel=3, PONO_C=True, down=DOWN, warp_mask_losstype="direct", isTrain=True)
    d = ops.PATCHMATCH_DEFAULTS
    lines = [f"# tools/patchmatch_box3_bench.py on {torch.cuda.get_device_name(0)}: k = {K}, match_kernel 3, PONO_C, warp_mask_losstype "
             f"direct (Cv = {3 + NC}); PatchMatch defaults: strides {d['strides']}, radii {d['radii']} from {d['radius0']}, seed {d['seed']}",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)"]

    for shape in args.shapes.split(","):
        B, side = (int(v) for v in shape.split("x"))
        H = W = side
        N = H * W
        t_bytes = B * N * N * 4
        g = torch.Generator(device=dev).manual_seed(1000 + N)
        theta = (torch.randn(B, 256, H, W, device=dev, generator=g) + 0.1).requires_grad_(True)
        phi = (theta.detach().roll((3, -5), (2, 3)) + 0.5 * torch.randn(B, 256, H, W, device=dev, generator=g) - 0.05).requires_grad_(True)
        lines.append(f"## B = {B}, {H} x {W} grid (HW = {N}); one T: {t_bytes / 2 ** 20:.0f} MiB; one PatchMatch step: "
                     f"{B * N * K * (5 + d['radii'])} pairs of 9 taps")
        ref_img = torch.rand(B, 3, H * DOWN, W * DOWN, device=dev, generator=g) * 2 - 1
        onehot = lambda: torch.zeros(B, NC, H * DOWN, W * DOWN, device=dev).scatter_(
            1, torch.randint(0, NC, (B, 1, H * DOWN, W * DOWN), device=dev, generator=g), 1.0)
        seg = onehot()
        g_out = torch.randn(B, 3, H * DOWN, W * DOWN, device=dev, generator=g)
        g_mask = torch.randn(B, NC, H, W, device=dev, generator=g)
        dense_runs = t_bytes <= DENSE_T_LIMIT and ops.box3_fused_ok(B, 256, H, W) and ops.box3_topk_ok(K)
        radii = (d["radii"], d["radius0"])
        with torch.no_grad():
            stats = (*ops.unfold3_stats(theta.detach(), KC), *ops.unfold3_stats(phi.detach(), KC))
            start = hot_path._patchmatch_coarse_init_box3(theta.detach(), phi.detach(), cfg, 1.0 / INV_T, K)
        lines.append(f"coarse start: {hot_path._patchmatch_coarse_route_box3(B, 256, H, W, H, W, K)}")

        def sparse(search):
            theta.grad = phi.grad = None
            out = correspondence_sparse_box3(theta, phi, ref_img, seg, seg, cfg, topk=K, search=search)
            torch.autograd.backward([out["warp_out"], out["warp_mask"]], [g_out, g_mask])

        def select_pm():
            with torch.no_grad():
                th, ph = theta.detach(), phi.detach()
                st = (*ops.unfold3_stats(th, KC), *ops.unfold3_stats(ph, KC))
                init = hot_path._patchmatch_coarse_init_box3(th, ph, cfg, 1.0 / INV_T, K)
                ops.patchmatch_topk_box3(th, ph, *st, INV_T, K, init, d["strides"], radii, d["seed"])

        arms = {"select patchmatch": select_pm,
                "pm one step": lambda: ops.patchmatch_topk_box3(theta, phi, *stats, INV_T, K, start, (1,), radii, d["seed"]),
                "sparse patchmatch": lambda: sparse("patchmatch")}
        if dense_runs:
            arms["select dense"] = lambda: correspondence_match(theta.detach(), phi.detach(), cfg, 1.0 / INV_T, topk=K)
            arms["sparse dense"] = lambda: sparse("dense")
        else:
            lines.append(f"dense arms not run: one T is {t_bytes} bytes ({t_bytes / 2 ** 30:.1f} GiB) per batch at this shape; "
                         f"ops.box3_fused_ok = {ops.box3_fused_ok(B, 256, H, W)}")
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
        if dense_runs:
            lines.append(f"ratios (medians): select patchmatch / dense = {med['select patchmatch'] / med['select dense']:.3f}   "
                         f"sparse patchmatch / dense = {med['sparse patchmatch'] / med['sparse dense']:.3f}")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        sparse("patchmatch")
        torch.cuda.synchronize()
        lines.append(f"sparse patchmatch forward + backward: peak memory growth {(torch.cuda.max_memory_allocated() - before) / 2 ** 20:.1f} MiB")
        if dense_runs:
            lines += recall_lines("planted translation (3, -5) + noise 0.5", theta, phi, cfg, ops, hot_path)
        del seg, g_mask, g_out, ref_img
        torch.cuda.empty_cache()

    # theta / phi of a randomly initialised network at a 256 x 256 crop (a 64 x 64 grid)
    opt = cc.ade20k_options(crop_size=256, semantic_nc=NC, match_kernel=3)
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
                              cfg, ops, hot_path)

    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:34s} VGPRs {v:3d}  SGPRs {s:3d}  scratch {sc} B/lane  waves/SIMD {o}" for name, v, s, sc, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
