"""K46 cost: hot_path.correspondence_flow, forward + backward, at B = 8 on a 64 x 64 grid (a 256 x 256 crop), the three new kernels
alone on the same operands, and hot_path.correspondence_sparse at k = 4, forward + backward, as context.

Timing arms, all timed with device events inside ONE process, alternating round by round; the figure of an arm is the median over the
rounds (>= 20) after a warm-up:
    flow r fwd+bwd          correspondence_flow(radius=r) on theta_raw / phi_raw leaves + the backward of a photometric and an offset
                            term to both leaves, r = 1, 2, 3 (K1 and its backward, the selection, K44, K46, the glue)
    sparse k=4 fwd+bwd      correspondence_sparse(topk=4) + the backward of its warp_out / warp_mask to both leaves (K42; context)
    bwd query r (kernel)    cocos_match_refine_bwd_query_f16x3 alone (ds and dq_t), r = 1, 2, 3
    bwd key r (kernel)      cocos_match_refine_bwd_key_f16x3 alone on the inverse table of the selected centres, r = 1, 2, 3
    gather bwd (kernel)     cocos_gather_patches_subcell_bwd_off alone

    python tools/match_flow_bench.py [--out profiles/k46_match_flow.txt] [--rounds 21] [--window 0.05]
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

B, CROP, NC, INV_T = 8, 256, 151, 100.0
KERNELS = (("plane_pair.hip", ("match_refine_bwd_query_kernel", "match_refine_bwd_key_kernel")),
           ("gather_warp.hip", ("gather_patches_subcell_bwd_off_kernel",)))


def register_rows():
    """[(kernel, VGPRs, SGPRs, scratch bytes / lane, waves / SIMD)] of the new kernels from hipcc's kernel-resource-usage remarks; None
    without hipcc"""
    rows = []
    for unit, wanted in KERNELS:
        usage = benchlib.resource_usage(unit, keep=wanted)
        if usage is None:
            return None
        for u in usage:
            want = next(w for w in wanted if w in u.name)
            inst = re.search(r"kernelILi(\d+)E", u.name)
            rows.append((want + (f"<{inst.group(1)}>" if inst else ""), u.vgprs, u.sgprs, u.scratch, u.occupancy))
    return sorted(rows)


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, os.path.join("profiles", "k46_match_flow.txt"))
    args = ap.parse_args()
    benchlib.require_gpu("match_flow_bench")
    from cocosnet_amd import _lib, ops
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_flow, correspondence_sparse
    dev = torch.device("cuda", 0)
    opt = cc.ade20k_options(crop_size=CROP, semantic_nc=NC, match_kernel=1)
    torch.manual_seed(0)
    net = cc.NoVGGCorrespondence(opt).to(dev)
    cfg = HotPathConfig.from_opt(opt, down=opt.down)      # (the module sets opt.down)
    net.init_weights(opt.init_type, opt.init_variance)
    net.eval()
    g = torch.Generator(device=dev).manual_seed(4)
    onehot = lambda: torch.zeros(B, NC, CROP, CROP, device=dev).scatter_(1, torch.randint(0, NC, (B, 1, CROP, CROP), device=dev, generator=g), 1.0)
    ref_img = torch.rand(B, 3, CROP, CROP, device=dev, generator=g) * 2 - 1
    seg, ref_seg = onehot(), onehot()
    side, down = CROP // opt.down, opt.down
    N = side * side
    rnd = lambda *shape: torch.randn(*shape, device=dev, generator=g)
    with torch.no_grad():
        theta_raw, phi_raw = net.project(ref_img, None, seg, ref_seg, None, lazy=True)
        theta, phi = theta_raw.raw().detach().clone(), phi_raw.raw().detach().clone()
        planes = ops.OperandPlanes()
        qn = ops.center_l2norm_planes(theta.reshape(B, 256, N), 1, planes, want_chan=False)
        kn = ops.center_l2norm_planes(phi.reshape(B, 256, N), 1, planes, want_chan=False)
        qh, ql = planes.get(qn, True, ops.SPLIT_OPERAND_SCALE)
        kh, kl = planes.get(kn, True, ops.SPLIT_OPERAND_SCALE)
        idx, _, _ = ops.corr_match(qn, kn, INV_T, planes)
        idx = idx.reshape(B, N).clamp(0, N - 1).contiguous()
        off1, _ = ops.match_refine(qn, kn, idx, (side, side), INV_T, 1, planes)
        entries, offsets = ops._inverse_index_table(idx.view(B, N, 1), N)
    theta.requires_grad_(True)
    phi.requires_grad_(True)
    g_out, g_off, g_mask = rnd(B, 3, CROP, CROP), rnd(B, 2, side, side), rnd(B, NC, side, side)
    doff, stream = rnd(B, N, 2), torch.cuda.current_stream().cuda_stream
    ds = {r: torch.empty(B, N, (2 * r + 1) ** 2, device=dev) for r in (1, 2, 3)}
    dq_t, dk_t, doff_out = torch.empty(B, N, 256, device=dev), torch.empty(B, N, 256, device=dev), torch.empty(B, N, 2, device=dev)

    def flow(r):
        theta.grad = phi.grad = None
        out = correspondence_flow(theta, phi, ref_img, cfg, 1.0 / INV_T, radius=r)
        torch.autograd.backward([out["warp_out"], out["match_offset"]], [g_out, g_off])

    def sparse():
        theta.grad = phi.grad = None
        out = correspondence_sparse(theta, phi, ref_img, seg, ref_seg, cfg, 1.0 / INV_T, 4)
        torch.autograd.backward([out["warp_out"], out["warp_mask"]], [g_out, g_mask])

    dims = lambda r: (B, 256, N, N, side, side, r, INV_T, ops.SPLIT_OPERAND_SCALE, stream)
    query = lambda r: _lib.call("cocos_match_refine_bwd_query_f16x3", qh.data_ptr(), ql.data_ptr(), kh.data_ptr(), kl.data_ptr(),
                                idx.data_ptr(), doff.data_ptr(), ds[r].data_ptr(), dq_t.data_ptr(), *dims(r))
    key = lambda r: _lib.call("cocos_match_refine_bwd_key_f16x3", qh.data_ptr(), ql.data_ptr(), ds[r].data_ptr(), entries.data_ptr(),
                              offsets.data_ptr(), dk_t.data_ptr(), *dims(r))
    gather = lambda: _lib.call("cocos_gather_patches_subcell_bwd_off", ref_img.data_ptr(), idx.data_ptr(), off1.data_ptr(), g_out.data_ptr(),
                               doff_out.data_ptr(), B, 3, side, side, side, side, down, 3 * CROP * CROP, stream)
    arms = {}
    for r in (1, 2, 3):
        arms[f"flow {r} fwd+bwd"] = lambda r=r: flow(r)
    arms["sparse k=4 fwd+bwd"] = sparse
    for r in (1, 2, 3):
        arms[f"bwd query {r} (kernel)"] = lambda r=r: query(r)
    for r in (1, 2, 3):      # (after the query arms' warm-up: ds[r] holds that kernel's output)
        arms[f"bwd key {r} (kernel)"] = lambda r=r: key(r)
    arms["gather bwd (kernel)"] = gather
    group = torch.bincount(idx.long().reshape(-1) + (torch.arange(B, device=dev) * N).repeat_interleave(N), minlength=B * N)
    lines = [f"# tools/match_flow_bench.py on {torch.cuda.get_device_name(0)}: B = {B}, {CROP} x {CROP} crop, {side} x {side} grid, "
             f"match_kernel 1, PONO_C, ade20k options ({NC} labels), randomly initialised network",
             f"# ms per call: median of {args.rounds} alternating windows of ~{args.window} s after {args.warmup} warm-up calls "
             "(min .. max of the windows)",
             f"# centres: {int((group > 0).sum())} distinct of {B * N} queries, the most shared one named by {int(group.max())} queries "
             "(the key kernel walks such a list serially for every key around it)",
             "# row reads of the query kernel: 2 B N (2 r + 1)^2 rows of 1 KiB (scores, then dq) = "
             + ", ".join(f"{2 * B * N * (2 * r + 1) ** 2 * 1024 / 1e9:.2f} GB at r = {r}" for r in (1, 2, 3))]
    counts = benchlib.window_counts(arms, args.window, args.warmup)
    samples = benchlib.alternating(arms, counts, args.rounds)
    med = {name: statistics.median(v) for name, v in samples.items()}
    for name in arms:
        v = samples[name]
        lines.append(f"{name:24s} {med[name]:9.4f} ms  ({min(v):.4f} .. {max(v):.4f}; {counts[name]} calls per window)")
    lines.append("ratios (medians): " + "   ".join(f"flow {r} / sparse k=4 = {med[f'flow {r} fwd+bwd'] / med['sparse k=4 fwd+bwd']:.3f}"
                                                     for r in (1, 2, 3)))
    table = register_rows()
    lines.append("# registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
    if table is None:
        lines.append("(no hipcc on this host)")
    else:
        lines += [f"{name:40s} VGPRs {v:3d}  SGPRs {s:3d}  scratch {sc} B/lane  waves/SIMD {o}" for name, v, s, sc, o in table]
    benchlib.write_report(lines, args.out)


if __name__ == "__main__":
    main()
