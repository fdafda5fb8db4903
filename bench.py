#!/usr/bin/env python
"""Benchmark of the MI355X-native correspondence hot path (driver contract: see README / DESIGN.md).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scope hotpath|netcorr] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-extras]] [--grad-payload path|netcorr|full]

A "step" is ONE forward + backward pass of the hot path over one batch of synthetic ADE20k-shaped
input (BASELINE.json configs[1]: 256x256 images, batch 8 per GPU, 64x64 feature grid, K = 256,
V = 3 exemplar colours + 151 one-hot labels), inputs already resident in HBM:

    theta/phi 1x1 convs (:272,:282) -> centre + L2-norm (:277-289) -> correlation / T -> softmax ->
    warp of [rgb | ref_seg] (:291-336) -> nearest x4 up-sample (:327) -> loss = <out, G> -> backward
    down to the gradients of the theta/phi weights and of the incoming features
    -> (N > 1) RCCL all-reduce of the parameter gradients.

`value` = images/s summed over all ranks (weak scaling: batch 8 per GPU whatever N), `ms_per_step` = the time of one
timed step.  A plain run does only that: set-up, W warm-up steps, K timed steps (no HIP events in them), the result
line.  `--dump-outputs DIR` then writes what the last timed step computed (see dump_outputs).  With `--full` the same
JSON line also carries, measured in the same process after the headline window: the per-kernel table and the roofline
(HIP events around the dominant kernel in the timed window, the others in a window of their own), the exact-fp32-MFMA
flavour (`flavours.fp32`), a >= 300-step stability window (`stability`), the context configurations, and the CPU
baseline (the reference's torch op sequence on all host cores, plus the numpy port).  `--grad-payload` sizes the gradient exchange of N > 1 runs like BASELINE config 4 (netCorr's
59 M or the full G+Corr 156 M fp32 parameters) — the hot path alone exchanges only theta/phi's 0.8 MB.
`--scope netcorr` times the whole drop-in NoVGGCorrespondence module instead (feature producers on the K16 / K16b
convolutions, K9 / K13 / K17 norms; `COCOS_CONV=f16x3|bf16|torch` picks the convolution flavour, named in
config.workload); it is reported for context in DESIGN.md and is not the headline line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, 256 CUs x 2.4 GHz
F16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA (v_mfma_f32_32x32x16_f16: 32 cycles), no sparsity
F16_MFMA_SUSTAINED_FRAC = 0.655     # measured: tools/mfma_ceiling.sh -> profiles/r06_mfma_ceiling.txt (random operands; zeros reach 0.991)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E ~8 TB/s
BATCH_PER_GPU = 8
IMG = 256
DOWN = 4
SEM_NC = 151
KDIM = 256


def _conv_flavour():
    """How the module scope's nn.Conv2d layers run (COCOS_CONV): 'f16x3' fp32-accurate split (default, parity-safe upstream of
    the softmax at T = 0.01), 'bf16' one term (K16b, the precision of the reference's --amp), 'torch' the framework's MIOpen."""
    from cocosnet_amd import ops
    return ops.CONV_PRECISION


def module_scope_context(device, d, steps=8, warmup=6):
    """ms per forward + backward of the whole NoVGGCorrespondence module (batch 8, 256x256, ADE20k flags) with the convolutions
    on K16c (f16x3, the parity-safe default) and on K16b (bf16): what `--scope netcorr` times, reported beside the headline.
    The bf16 figure carries its END-TO-END deviation: the same module — same parameters, eval mode so that
    spectral norm does not iterate — evaluated in both flavours; `err_vs_f16x3` = max|bf16 - f16x3| / max|f16x3| per output
    (the f16x3 flavour is what tests/test_gpu_conv.py holds to torch-fp64 at 1e-3).  Those convolutions sit upstream of a
    softmax at T = 0.01, so the bf16 timing is NOT a parity-qualified result unless that figure is below 1e-3."""
    from cocosnet_amd import ops
    out = {}
    saved = ops.CONV_PRECISION
    ref_out = {}
    try:
        for flavour in ("f16x3", "bf16"):
            ops.CONV_PRECISION = flavour
            torch.manual_seed(0)
            model, fwd = make_step("netcorr", device)
            params = list(model.parameters())

            def step():
                for p in params:
                    p.grad = None
                o = fwd(d)
                torch.autograd.backward([o["warp_out"], o["warp_mask"]], [d["g_out"], d["g_mask"]])

            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            out[flavour] = {"ms_per_step": round(ms, 3), "images_per_s": round(BATCH_PER_GPU / ms * 1e3, 1), "steps": steps}
            # end-to-end outputs of THIS flavour on identical parameters (fresh seed-0 module, eval: no power iteration)
            torch.manual_seed(0)
            probe, pf = make_step("netcorr", device)
            probe.eval()
            with torch.no_grad():
                o = pf(d)
            cur = {k: o[k].float() for k in ("warp_out", "warp_mask")}
            if flavour == "f16x3":
                ref_out = cur
            else:
                out[flavour]["err_vs_f16x3"] = {k: float((cur[k] - ref_out[k]).abs().max() / ref_out[k].abs().max())
                                                for k in cur}
                out[flavour]["parity_qualified"] = bool(max(out[flavour]["err_vs_f16x3"].values()) < 1e-3)
            del model, params, probe
        out["note"] = ("whole module fwd+bwd (adaptors, ResidualBlocks, SPADE blocks, theta/phi, the path); convolutions f16x3 = "
                       "three-term f16 hi/lo on the NHWC / LDS-DMA kernels (K16c, default), bf16 = one term (K16b, COCOS_CONV=bf16); "
                       "err_vs_f16x3 = end-to-end max-norm deviation of warp_out / warp_mask on identical parameters: bf16 convolutions "
                       "upstream of the T = 0.01 softmax are a timing reference, not a parity-qualified result, unless it is < 1e-3")
        if not out["bf16"].get("parity_qualified", False):      # no bf16 timing beside the qualified ones
            out["unqualified"] = {"bf16": out.pop("bf16")}
    finally:
        ops.CONV_PRECISION = saved
    return out


def config5_context(device, steps=5, warmup=3):
    """BASELINE config 5 as the reference runs it: DeepFashion flags (README.md:69,115: --warp_patch --warp_bilinear, float pose maps,
    no mask loss) on the DEFAULT match_kernel 3 (options/base_options.py:70), 512^2 input at down 4 = 128 x 128 grid, HW = 16384,
    B = 2, forward + backward of the hot path from theta / phi on — the fused match_kernel-3 family on a 128-wide grid (round 4;
    round 3 fell back to three materialised 1 GiB matrices per sample and orientation here).  Context, never part of `value`."""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    B, S, fh = 2, 512, 128
    g = torch.Generator(device=device).manual_seed(4321)
    th = torch.randn(B, KDIM, fh, fh, device=device, generator=g).requires_grad_(True)
    ph = (0.3 * th.detach().roll((3, 11), (2, 3)) + torch.randn(B, KDIM, fh, fh, device=device, generator=g)).requires_grad_(True)
    img = torch.rand(B, 3, S, S, device=device, generator=g) * 2 - 1
    seg = torch.rand(B, 20, S, S, device=device, generator=g)
    gout = torch.randn(B, 3, S, S, device=device, generator=g)
    out = {}
    for mk in (3, 1):
        cfg = HotPathConfig(match_kernel=mk, PONO_C=True, down=4, warp_patch=True, warp_bilinear=True, isTrain=True)

        def step():
            th.grad = ph.grad = None
            o = correspondence_hot_path(th, ph, img, img, seg, seg, cfg)
            o["warp_out"].backward(gout)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()        # (the headline's model and inputs stay resident: the step's OWN peak is reported)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[f"match_kernel_{mk}"] = {"ms_per_step": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1), "steps": steps,
                                     "peak_mem_GiB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)}
    out["note"] = ("DeepFashion 512^2 --warp_patch (Cv = 48), 128x128 grid (HW = 16384), B = 2, hot path fwd+bwd; match_kernel 3 is "
                   "what every README command runs (base_options.py:70): fused family K19 / K20 on a 128-wide grid")
    return out


def config3_hot_path_context(device, steps=8, warmup=3):
    """The correspondence hot path of BASELINE config 3 as the README runs it (README.md:106: CelebA-HQ edge->face, --warp_bilinear
    --warp_cycle_w 1, float edge maps, no mask loss, the DEFAULT match_kernel 3), B = 16, 256^2 at down 4 = 64 x 64 grid: a row pass
    and a column pass over the same correlation (round 4: ONE T read transposed by the column pass, ONE gradient buffer, one box
    adjoint + one GEMM pair).  Forward + backward from theta / phi on; match_kernel 1 beside it.  Context, never part of `value`."""
    from cocosnet_amd.hot_path import HotPathConfig, correspondence_hot_path
    B, S, fh = 16, 256, 64
    g = torch.Generator(device=device).manual_seed(333)
    th = torch.randn(B, KDIM, fh, fh, device=device, generator=g).requires_grad_(True)
    ph = (0.3 * th.detach().roll((2, 7), (2, 3)) + torch.randn(B, KDIM, fh, fh, device=device, generator=g)).requires_grad_(True)
    img = torch.rand(B, 3, S, S, device=device, generator=g) * 2 - 1
    seg = torch.rand(B, 15, S, S, device=device, generator=g)
    out = {}
    for mk in (3, 1):
        cfg = HotPathConfig(match_kernel=mk, PONO_C=True, down=4, warp_bilinear=True, warp_cycle_w=1.0, isTrain=True)
        cot = {}

        def step():
            th.grad = ph.grad = None
            o = correspondence_hot_path(th, ph, img, img, seg, seg, cfg)
            if not cot:
                cot.update({k: torch.randn(v.shape, device=device, generator=g) for k, v in o.items()})
            torch.autograd.backward([o[k] for k in sorted(o)], [cot[k] for k in sorted(o)])
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()        # (the headline's model and inputs stay resident: the step's OWN peak is reported)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[f"match_kernel_{mk}"] = {"ms_per_step": round(ms, 3), "images_per_s": round(B / ms * 1e3, 1), "steps": steps,
                                     "peak_mem_GiB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 2)}
    out["note"] = ("CelebA-HQ edge training flags (--warp_cycle_w 1: row pass + column pass), B = 16, 64x64 grid, hot path fwd+bwd; "
                   "match_kernel 3 is what the README command runs")
    return out


def config3_context(device, steps=4, warmup=3):
    """BASELINE config 3 as written — "CelebA-HQ edge->face 256x256 batch 16, + HIP SPADE generator / PatchGAN conv kernels, bf16
    MFMA" — for the two networks behind the correspondence: cocosnet_amd.translation.SPADEGenerator (generator.py:17-89) and
    MultiscaleDiscriminator (discriminator.py:14-177) with the README's training flags (README.md:106), B = 16, random-init
    weights, synthetic inputs: forward + backward of G (conditioned on [warp_out | edge maps]) and of D on [maps | fake], in the
    fp32-accurate flavour (f16x3) and in the one the config names (bf16), each with its END-TO-END error against an fp64 copy of
    the same module evaluated by the framework (B = 2 of the same inputs).  Context, never part of `value`."""
    import copy
    from cocosnet_amd import ops, translation as tl
    opt = tl.celebahq_edge_train_options()
    B = 16
    g = torch.Generator(device=device).manual_seed(77)
    seg = torch.rand(B, 15, IMG, IMG, device=device, generator=g)
    cbn = torch.cat((torch.rand(B, 3, IMG, IMG, device=device, generator=g) * 2 - 1, seg), 1)
    real = torch.rand(B, 3, IMG, IMG, device=device, generator=g) * 2 - 1
    gimg = torch.randn(B, 3, IMG, IMG, device=device, generator=g)
    out, saved = {}, ops.CONV_PRECISION
    try:
        torch.manual_seed(0)
        G = tl.SPADEGenerator(opt).to(device)
        G.init_weights(opt.init_type, opt.init_variance)
        D = tl.MultiscaleDiscriminator(opt).to(device)
        D.init_weights(opt.init_type, opt.init_variance)
        G.eval(); D.eval()                       # spectral norm does not iterate: every arm sees the same weights
        G64, D64 = copy.deepcopy(G).double(), copy.deepcopy(D).double()
        with torch.no_grad():
            y64 = G64(seg[:2].double(), warp_out=cbn[:2].double())
            d64 = D64(torch.cat((seg[:2].double(), y64), 1))[0]
        rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
        # errors first, in eval mode (in train mode spectral norm iterates and the timed steps below move the weights away from
        # the fp64 copy's)
        for flavour in ("f16x3", "bf16"):
            ops.CONV_PRECISION = flavour
            with torch.no_grad():
                y = G(seg[:2], warp_out=cbn[:2])
                dd = D(torch.cat((seg[:2], y64.float()), 1))[0]
            out[flavour] = {"err_vs_fp64": {"fake_image": rel(y, y64), "D_logits": max(rel(a[-1], b[-1]) for a, b in zip(dd, d64))}}
        del G64, D64
        G.train(); D.train()
        gp, dp = list(G.parameters()), list(D.parameters())
        for flavour in ("f16x3", "bf16"):
            ops.CONV_PRECISION = flavour

            def g_step():
                for p in gp:
                    p.grad = None
                G(seg, warp_out=cbn).backward(gimg)

            def d_step():
                for p in dp:
                    p.grad = None
                res = D(torch.cat((seg, real), 1))[0]
                torch.autograd.backward([r[-1] for r in res], [torch.ones_like(r[-1]) for r in res])

            for name, fn in (("generator", g_step), ("discriminator", d_step)):
                for _ in range(warmup):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / steps * 1e3
                out[flavour][name] = {"ms_fwd_bwd": round(ms, 2), "images_per_s": round(B / ms * 1e3, 1)}
        out["note"] = ("cocosnet_amd.translation.SPADEGenerator / MultiscaleDiscriminator, CelebA-HQ edge training flags, B = 16, 256x256, "
                       "forward + backward each; err_vs_fp64 = max-norm error of the generated image / the PatchGAN logits against an "
                       "fp64 copy of the same module (eval mode, 2 samples): bf16 is the precision BASELINE config 3 names for these two "
                       "networks (behind InstanceNorm / SPADE, NOT upstream of the correlation).  Round 5: the only flavour within "
                       "north_star's 1e-3 of fp64 is f16x3 — one f16 term is at 2.2e-3 on fake_image, two terms (activations split, weights "
                       "one plane) at 1.4e-3 (generator) / 6e-4 (PatchGAN), bf16 at 1.6e-2: profiles/r05_conv_flavour_table.txt, all arms on "
                       "the fp64 copy's branch pattern — so bf16 is listed under `unqualified`")
        out["bf16"]["parity_qualified"] = bool(max(out["bf16"]["err_vs_fp64"].values()) < 1e-3)
        out["f16x3"]["parity_qualified"] = bool(max(out["f16x3"]["err_vs_fp64"].values()) < 1e-3)
        if not out["bf16"]["parity_qualified"]:
            out["unqualified"] = {"bf16": out.pop("bf16")}
    finally:
        ops.CONV_PRECISION = saved
    return out


def build_inputs(device, scope):
    g = torch.Generator(device=device).manual_seed(1234 + (torch.distributed.get_rank()
                                                           if torch.distributed.is_initialized() else 0))
    B, fh = BATCH_PER_GPU, IMG // DOWN
    lab = torch.randint(0, SEM_NC, (B, 1, IMG // 16, IMG // 16), device=device, generator=g)
    lab = lab.repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = torch.zeros(B, SEM_NC, IMG, IMG, device=device).scatter_(1, lab, 1.0)
    lab2 = torch.randint(0, SEM_NC, (B, 1, IMG // 16, IMG // 16), device=device, generator=g)
    lab2 = lab2.repeat_interleave(16, 2).repeat_interleave(16, 3)
    ref_seg = torch.zeros(B, SEM_NC, IMG, IMG, device=device).scatter_(1, lab2, 1.0)
    ref_img = torch.rand(B, 3, IMG, IMG, device=device, generator=g) * 2 - 1
    real_img = torch.rand(B, 3, IMG, IMG, device=device, generator=g) * 2 - 1
    d = dict(seg=seg, ref_seg=ref_seg, ref_img=ref_img, real_img=real_img)
    if scope == "hotpath":
        cl = KDIM + SEM_NC   # 407 channels into theta/phi on ADE20k (--maskmix)
        d["cont_features"] = torch.randn(B, cl, fh, fh, device=device, generator=g).requires_grad_(True)
        d["ref_features"] = (0.3 * d["cont_features"].detach()[:, :, torch.randperm(fh, device=device, generator=g)]
                             + torch.randn(B, cl, fh, fh, device=device, generator=g)).requires_grad_(True)
    d["g_out"] = torch.randn(B, 3, IMG, IMG, device=device, generator=g)
    d["g_mask"] = torch.randn(B, SEM_NC, fh, fh, device=device, generator=g)
    return d


class HotPathStep(torch.nn.Module):
    """theta/phi projections + the HIP hot path (ADE20k flag set, match_kernel 1)."""

    def __init__(self, match_kernel=1):
        super().__init__()
        from cocosnet_amd.hot_path import HotPathConfig
        cl = KDIM + SEM_NC
        self.theta = torch.nn.Conv2d(cl, KDIM, 1)
        self.phi = torch.nn.Conv2d(cl, KDIM, 1)
        self.cfg = HotPathConfig(match_kernel=match_kernel, PONO_C=True, down=DOWN,
                                 warp_mask_losstype="direct")

    def forward(self, d):
        from cocosnet_amd import ops
        from cocosnet_amd.hot_path import correspondence_hot_path
        # :272 / :282 as lazy projections: the match_kernel-1 path fuses them with the centring / normalisation (K23), match_kernel 3
        # asks for the fp32 projections (K0) — exactly what NoVGGCorrespondence.forward hands to the hot path
        theta = ops.LazyProj1x1(d["cont_features"], self.theta.weight, self.theta.bias)
        phi = ops.LazyProj1x1(d["ref_features"], self.phi.weight, self.phi.bias)
        return correspondence_hot_path(theta, phi,
                                       d["ref_img"], d["real_img"], d["seg"], d["ref_seg"], self.cfg)


def make_step(scope, device, match_kernel=1):
    if scope == "hotpath":
        model = HotPathStep(match_kernel).to(device)
        fwd = lambda d: model(d)
    else:
        from cocosnet_amd.correspondence import NoVGGCorrespondence, ade20k_options
        opt = ade20k_options(match_kernel=match_kernel, isTrain=True)
        model = NoVGGCorrespondence(opt).to(device)
        model.init_weights(opt.init_type, opt.init_variance)
        fwd = lambda d: model(d["ref_img"], d["real_img"], d["seg"], d["ref_seg"])
    return model, fwd


#: --dump-outputs writes at most this many fp32 elements in all (60 MiB); larger outputs are sampled
DUMP_BUDGET_ELEMS = 15 << 20


def dump_outputs(out_dir, outputs, model, d):
    """--dump-outputs: what the timed step computed in its last step, each array as `<name>.npy` in float32 — the forward's
    outputs (`warp_out`, `warp_mask`, ...) and the gradients a caller of the step receives: `grad_<parameter>` and
    `grad_cont_features` / `grad_ref_features`.  The budget is shared out smallest array first; an array above its share
    is written as a fixed sample (sorted flat indices from a seed-0 permutation, the same in every run), otherwise whole
    and in its own shape."""
    import numpy as np
    arrays = {k: v for k, v in outputs.items()}
    arrays.update({f"grad_{n}": p.grad for n, p in model.named_parameters() if p.grad is not None})
    arrays.update({f"grad_{k}": d[k].grad for k in ("cont_features", "ref_features") if k in d and d[k].grad is not None})
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BUDGET_ELEMS
    for i, (name, t) in enumerate(sorted(arrays.items(), key=lambda kv: (kv[1].numel(), kv[0]))):
        a = t.detach().float()
        share = left // (len(arrays) - i)
        if a.numel() > share:
            idx = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:share].sort().values
            a = a.reshape(-1)[idx.to(a.device)]
        left -= a.numel()
        np.save(os.path.join(out_dir, name.replace(".", "_") + ".npy"), a.cpu().numpy())


def cpu_baseline_numpy(n_images, seed=0):
    """The numpy oracle (fp32, BLAS threads = host cores) on a bounded sample: forward + backward of the hot path
    from theta/phi on, batch 1 per call."""
    import numpy as np
    from oracle import corr_oracle as co
    # ONE thread policy for both CPU figures: min(host cores, 32) BLAS threads, like the torch baseline below
    used = min(os.cpu_count() or 1, 32)
    limiter = None
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=used)
        cores = used
    except Exception:
        cores = os.cpu_count() or 1
    rs = np.random.RandomState(seed)
    fh = IMG // DOWN
    N = fh * fh
    th = rs.standard_normal((1, KDIM, N)).astype(np.float32)
    ph = rs.standard_normal((1, KDIM, N)).astype(np.float32)
    v = rs.uniform(-1, 1, (1, 3 + SEM_NC, N)).astype(np.float32)
    gout = rs.standard_normal((1, 3 + SEM_NC, N)).astype(np.float32)

    def one():
        qn, kn = co.center_l2norm(th, True), co.center_l2norm(ph, True)
        out = co.corr_softmax_warp(qn, kn, v, np.float32(100.0))
        dqn, dkn, _ = co.corr_softmax_warp_bwd(qn, kn, v, gout, np.float32(100.0))
        return out, co.center_l2norm_bwd(th, dqn, True), co.center_l2norm_bwd(ph, dkn, True)
    one()   # warm-up (BLAS thread pool, page faults)
    t0 = time.perf_counter()
    for _ in range(n_images):
        one()
    dt = time.perf_counter() - t0
    if limiter is not None:
        limiter.restore_original_limits()
    return {"value": n_images / dt, "unit": "images/s", "cores": int(cores), "kind": "port",
            "sample": f"{n_images} images (batch 1 each) through oracle/corr_oracle.py in fp32 numpy: centre+L2norm, "
                      f"correlation, softmax, warp (Cv=154), and their backward; {dt:.1f} s wall"}


def cpu_baseline(runs=10, batch=2, seed=0, budget_s=25.0):
    """The reference's own op sequence for the same workload on the host cores: correspondence.py:272-336 as restated
    on torch CPU tensors by oracle/torch_ref.py (torch matmul / softmax / avg_pool / interpolate, fp32, materialised
    f [B,HW,HW] exactly like the reference), theta/phi 1x1 convs included, forward + autograd backward, batch 2
    (SURVEY §8d).  Reported value: median of `runs` steps after 3 warm-ups at min(cores, 32) threads; `all_cores`
    beside it: the same step with torch.set_num_threads(os.cpu_count()), as many runs (<= runs) as fit in `budget_s`
    seconds after one warm-up — on the 256-thread hosts of the GPU boxes torch's CPU kernels are ~40x SLOWER with every
    thread than with 32 (measured: 10.6 s vs ~0.25 s per step), so the all-core figure alone would flatter the GPU."""
    import statistics
    from oracle import corr_oracle as co
    from oracle import torch_ref as tr
    cores = os.cpu_count() or 1
    prev = torch.get_num_threads()
    g = torch.Generator().manual_seed(seed)
    fh = IMG // DOWN
    cl = KDIM + SEM_NC
    theta, phi = torch.nn.Conv2d(cl, KDIM, 1), torch.nn.Conv2d(cl, KDIM, 1)
    cont = torch.randn(batch, cl, fh, fh, generator=g, requires_grad=True)
    refx = torch.randn(batch, cl, fh, fh, generator=g, requires_grad=True)
    img = torch.rand(batch, 3, IMG, IMG, generator=g) * 2 - 1
    lab = torch.randint(0, SEM_NC, (batch, 1, IMG // 16, IMG // 16), generator=g)
    lab = lab.repeat_interleave(16, 2).repeat_interleave(16, 3)
    seg = torch.zeros(batch, SEM_NC, IMG, IMG).scatter_(1, lab, 1.0)
    g_out = torch.randn(batch, 3, IMG, IMG, generator=g)
    g_mask = torch.randn(batch, SEM_NC, fh, fh, generator=g)
    opt = co.default_opt(match_kernel=1, PONO_C=True, down=DOWN, warp_mask_losstype="direct")

    def one():
        for t in (cont, refx, *theta.parameters(), *phi.parameters()):
            t.grad = None
        out = tr.hot_path(theta(cont), phi(refx), img, img, seg, seg, opt)
        torch.autograd.backward([out["warp_out"], out["warp_mask"]], [g_out, g_mask])

    def timed(threads, warm, n, budget=None):
        torch.set_num_threads(threads)
        for _ in range(warm):
            one()
        ts, t_begin = [], time.perf_counter()
        for _ in range(n):
            t0 = time.perf_counter()
            one()
            ts.append(time.perf_counter() - t0)
            if budget is not None and time.perf_counter() - t_begin > budget:
                break
        return ts
    try:
        used = min(cores, 32)
        ts = timed(used, 3, runs)
        ts_all = timed(cores, 1, runs, budget_s) if cores > used else ts
    finally:
        torch.set_num_threads(prev)
    med, med_all = statistics.median(ts), statistics.median(ts_all)
    return {"value": batch / med, "unit": "images/s", "cores": int(used), "kind": "port",
            "sample": f"median of {len(ts)} steps (after 3 warm-ups) of batch {batch}: the reference's torch op sequence "
                      f"(correspondence.py:272-336 restated in oracle/torch_ref.py, fp32, materialised [B,4096,4096] "
                      f"correlation) incl. the theta/phi 1x1 convs, forward + autograd backward, "
                      f"torch.set_num_threads({used}); {sum(ts):.1f} s of timed CPU work",
            "all_cores": {"value": batch / med_all, "unit": "images/s", "cores": int(cores),
                          "sample": f"same step, torch.set_num_threads({cores}): median of {len(ts_all)} after 1 warm-up, "
                                    f"{sum(ts_all):.1f} s"}}


HOT_TAGS = ("corr_softmax_warp_fwd", "corr_softmax_warp_bwd_query", "corr_softmax_warp_bwd_key_from_ds",
            "corr_softmax_warp_bwd_key", "corr_materialize", "corr_materialize_bwd", "logits_softmax_warp_fwd",
            "logits_softmax_warp_bwd")
SPLIT_TAGS = ("corr_softmax_warp_fwd", "corr_softmax_warp_bwd_query", "corr_softmax_warp_bwd_key_from_ds")
#: parameter counts of BASELINE config 4's exchange: theta/phi only (what the hot path owns),
#: netCorr (59 M), netG + netCorr (156 M)
PAYLOAD_PARAMS = {"path": 0, "netcorr": 59_000_000, "full": 156_000_000}
PMC_FILE = {"f16x3": next((f for f in ("r06_pmc_f16x3.json", "r05_pmc_f16x3.json", "r04_pmc_f16x3.json", "r03_pmc_f16x3.json", "r02_pmc_f16x3.json")
                           if os.path.exists(os.path.join(REPO, "profiles", f))), "r02_pmc_f16x3.json"),
            "fp32": "r01_pmc_final.json"}
# (the counters were taken on the general instantiations <..., 0>; the one that skips exact value blocks moves 8 MB less)
# substrings of the PMC file's kernel names (the training flavours: template arguments after these differ between rounds — value-lo
# skip, device scales — so the entry with the most dispatches among the matches is taken)
PMC_KEY = {"f16x3": {"corr_softmax_warp_fwd": "corr_fwd_f16x3_kernel<5, 1,",
                     "corr_softmax_warp_bwd_query": "corr_bwd_query_f16x3_kernel<5, 1,",
                     "corr_softmax_warp_bwd_key_from_ds": "hgemm_f16x3_kernel<1, 2"},
           "fp32": {"corr_softmax_warp_fwd": "corr_softmax_warp_fwd_kernel<256, 5, true",
                    "corr_softmax_warp_bwd_query": "corr_bwd_query_saved_kernel<256, 5, true",
                    "corr_softmax_warp_bwd_key_from_ds": "sgemm_mfma_kernel<true, true>"}}


def ops_value_lo_skip():
    from cocosnet_amd import ops
    return bool(getattr(ops, "VALUE_LO_SKIP", False))


def kernel_table(kern, precision):
    """Per-kernel algorithmic TFLOP/s from the live HIP-event times (forward 2*HW^2*(K+Cv), backward
    split as query side 2*HW^2*(K+Cv) [dP + dqn] and key side 2*HW^2*K [dkn]; no recompute counted)."""
    N = (IMG // DOWN) ** 2
    cv = 3 + SEM_NC
    B = BATCH_PER_GPU
    alg = {"corr_materialize": 2.0 * N * N * KDIM * B,
           "corr_materialize_bwd": 4.0 * N * N * KDIM * B,
           "logits_softmax_warp_fwd": 2.0 * N * N * cv * B,
           "logits_softmax_warp_bwd": 2.0 * N * N * cv * B,
           "corr_softmax_warp_fwd": 2.0 * N * N * (KDIM + cv) * B,
           "corr_softmax_warp_bwd_query": 2.0 * N * N * (KDIM + cv) * B,
           "corr_softmax_warp_bwd_key_from_ds": 2.0 * N * N * KDIM * B,
           "corr_softmax_warp_bwd_key": 2.0 * N * N * KDIM * B}
    # which matrix instruction the three K2 kernels issue: the split-precision flavour computes every
    # fp32-accurate product with 3 f16 MFMAs (hi*hi + hi*lo + lo*hi), so its roofline is the dense f16 MFMA
    # peak divided by 3; the other entry points (materialised family) stay on fp32 MFMA
    split = precision == "f16x3"
    kernels = {}
    for tag, flops in alg.items():
        if tag in kern:
            ms = kern[tag]["avg_ms"]
            tf = flops / ms / 1e9
            kernels[tag] = {"avg_ms": round(ms, 4), "calls": kern[tag]["calls"], "alg_tflops": round(tf, 2),
                            "frac_fp32_mfma_peak": round(tf / FP32_MFMA_PEAK_TFLOPS, 4)}
            if split and tag in SPLIT_TAGS:
                # MFMA terms per fp32-accurate product: 3 (hi*hi + hi*lo + lo*hi).  The 151 label channels of this
                # workload are one-hot, i.e. exact in f16: their lo plane is all zero, the kernels find that out on the
                # device (cocos_f16_plane_block_mask) and skip the V_lo term for 4 of the 5 value blocks — per 32-key tile
                # and wave 70 MFMAs instead of 78 in the forward and in the query backward (same result).
                terms = 3.0
                if ops_value_lo_skip() and tag in ("corr_softmax_warp_fwd", "corr_softmax_warp_bwd_query"):
                    vsteps, cvb = 2 * (cv // 32 + 1), cv // 32 + 1
                    terms = (3 * 16 + 3 * vsteps - 2 * (cvb - 1)) / (16 + vsteps)
                kernels[tag].update({"mfma": f"v_mfma_f32_32x32x16_f16 x{terms:.2f} per product on average "
                                             "(f16 hi/lo split, fp32 accumulate)",
                                     "issued_tflops": round(terms * tf, 1),
                                     "frac_f16_mfma_peak": round(terms * tf / F16_MFMA_PEAK_TFLOPS, 4)})
            else:
                kernels[tag]["mfma"] = "v_mfma_f32_32x32x2_f32"
    return kernels


def roofline_of(kernels, precision):
    """The `roofline` object of the dominant kernel (longest average launch)."""
    if not kernels:
        return None
    dom = max(kernels, key=lambda k: kernels[k]["avg_ms"])
    split = precision == "f16x3"
    # HBM bytes per launch come from separate rocprofv3 --pmc passes (FETCH_SIZE x2 on gfx950 +
    # WRITE_SIZE, MI355X_MICROARCH.md), committed under profiles/ — they cannot be read live
    traffic, traffic_src = None, None
    pmc_file = os.path.join(REPO, "profiles", PMC_FILE[precision])
    if dom in PMC_KEY[precision] and os.path.exists(pmc_file):
        best = -1
        for name, rec in json.load(open(pmc_file)).items():
            if PMC_KEY[precision][dom] in name and rec.get("dispatches", 0) > best:
                best = rec.get("dispatches", 0)
                traffic = rec["hbm_bytes"]
                traffic_src = f"profiles/{os.path.basename(pmc_file)} (rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE passes)"
    # the same kernel's HBM coordinates (the second roofline north_star names), both ways of counting bytes:
    #   moved       PMC bytes per launch / measured time — what the kernel actually pulls through HBM (saved logits in, dS'' out);
    #   algorithmic SURVEY §8(d)'s fused minimum 4 * (2 K HW + 2 HW Cv) * B per launch / measured time
    # `bound` below follows the contract (ALGORITHMIC flops vs ALGORITHMIC bytes: the matrix roof is the nearer one);
    # `nearer_roof_by_moved_bytes` says which roof the kernel is closer to when its real traffic is counted (VERDICT r3 weak 2:
    # the saved-logits design moves ~11x the algorithmic bytes, and by that count the kernel sits nearer the HBM roof)
    hbm = None
    alg_bytes = 4.0 * (2 * KDIM * (IMG // DOWN) ** 2 + 2 * (IMG // DOWN) ** 2 * (3 + SEM_NC)) * BATCH_PER_GPU
    alg_gbs = alg_bytes / (kernels[dom]["avg_ms"] * 1e-3) / 1e9
    if traffic:
        gbs = traffic / (kernels[dom]["avg_ms"] * 1e-3) / 1e9
        hbm = {"achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 4),
               "algorithmic_bytes": alg_bytes, "achieved_algorithmic": round(alg_gbs, 1),
               "frac_algorithmic": round(alg_gbs / HBM_PEAK_GBS, 4), "moved_over_algorithmic": round(traffic / alg_bytes, 2),
               "note": "moved bytes per launch (PMC, profiles/) / the launch time measured in this run; the kernel streams the "
                       "saved logits in and the dS'' planes out (2 x HW^2 x 4 B per sample) next to its MFMA work — a measured "
                       "design choice (saved logits beat the chunked recompute by 22-40 % at every BASELINE shape: config.context / "
                       "profiles/r05_configs_bench.json); a linear read reaches 4.7-4.9 TB/s on this chip "
                       "(tools/probes/strided_rows.hip)"}
    if split and dom in SPLIT_TAGS:
        peak = F16_MFMA_PEAK_TFLOPS / 3.0
        mfma_frac = kernels[dom]["alg_tflops"] / peak
        return {"bound": "mfma", "nearer_roof_by_moved_bytes": ("hbm" if hbm and hbm["frac"] > mfma_frac else "mfma"),
                "kernel": dom, "hbm": hbm, "achieved": kernels[dom]["alg_tflops"], "peak": round(peak, 1),
                "unit": "TFLOP/s", "frac": round(mfma_frac, 4),
                "frac_kind": "algorithmic FLOPs / (f16 MFMA peak / 3): the utilisation of the matrix pipe by ISSUED "
                             "instructions is frac_issued", "traffic": traffic,
                "traffic_unit": "bytes/launch", "traffic_source": traffic_src,
                "avg_launch_ms": kernels[dom]["avg_ms"], "issued_tflops": kernels[dom]["issued_tflops"],
                "frac_issued": kernels[dom]["frac_f16_mfma_peak"],
                # round 6: on random operands a pure f16 MFMA stream sustains 0.655 of the nominal rate on this
                # chip — the clock drops from 2.39 to ~1.8 GHz at the 1.3 kW it then draws (zeros: 0.991) — profiles/r06_mfma_ceiling.txt
                "frac_of_sustained": round(mfma_frac / F16_MFMA_SUSTAINED_FRAC, 4),
                "sustained_note": f"peak x {F16_MFMA_SUSTAINED_FRAC} = what a pure v_mfma_f32_32x32x16_f16 stream sustains on uniform "
                                  "random operands (DVFS / power: profiles/r06_mfma_ceiling.txt); `frac` stays against the nominal peak",
                "vs_fp32_mfma_peak": kernels[dom]["frac_fp32_mfma_peak"],
                "note": "achieved = ALGORITHMIC fp32 FLOPs per launch / HIP-event time on torch's current stream. Each "
                        "fp32-accurate product is 3 v_mfma_f32_32x32x16_f16 (hi*hi + hi*lo + lo*hi of f16 hi/lo "
                        f"operand planes, fp32 accumulate), so peak = dense f16 MFMA peak {F16_MFMA_PEAK_TFLOPS:.0f} / 3. "
                        f"frac_issued = issued FLOPs / {F16_MFMA_PEAK_TFLOPS:.0f}: equal to frac when all three terms are "
                        "issued; lower here because the V_lo term of the one-hot label blocks (exactly zero) is skipped "
                        "(kernels[...].mfma). vs_fp32_mfma_peak = achieved / "
                        "157.3 (the exact-fp32 MFMA this kernel replaces; flavours.fp32 in this line is that flavour, "
                        "same process, same box)."}
    return {"bound": "mfma", "kernel": dom, "hbm": hbm, "achieved": kernels[dom]["alg_tflops"], "peak": FP32_MFMA_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": kernels[dom]["frac_fp32_mfma_peak"], "traffic": traffic,
            "traffic_unit": "bytes/launch", "traffic_source": traffic_src, "avg_launch_ms": kernels[dom]["avg_ms"],
            "note": "algorithmic FLOPs per launch / HIP-event time on torch's current stream; peak = dense fp32 MFMA "
                    "(v_mfma_f32_32x32x2_f32)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults (round 6): 200 timed steps after 20 warm-up steps — 0.25 s of GPU time.  The 20-step window of earlier rounds started
    # ~10 ms after the GPU left its idle power state and read 3 % slower than the 300-step window that follows it (`stability`)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scope", choices=("hotpath", "netcorr"), default="hotpath")
    ap.add_argument("--match-kernel", type=int, choices=(1, 3), default=1,
                    help="1 = the north-star 64x64x256 correlation (headline); 3 = the reference's shipped "
                         "default (3x3 neighbourhoods, K6/K7 kernels) — reported for context")
    ap.add_argument("--precision", choices=("fp32", "f16x3"), default=None,
                    help="where the K2 products run (default: cocosnet_amd.ops.PRECISION, i.e. $COCOS_PRECISION "
                         "or the package default): fp32 = v_mfma_f32_32x32x2_f32, f16x3 = 3-term split on "
                         "v_mfma_f32_32x32x16_f16 (fp32-class accuracy)")
    ap.add_argument("--grad-payload", choices=tuple(PAYLOAD_PARAMS), default="path",
                    help="N > 1: size of the per-step gradient all-reduce.  path = theta/phi only (0.8 MB, what the hot "
                         "path owns); netcorr / full add fp32 stand-in parameters so that the exchange is netCorr's 237 MB "
                         "or BASELINE config 4's 624 MB (their gradients are written every step, in backward order)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline: per-kernel table and roofline, other flavours, "
                         "stability window, context configurations, CPU baseline, N > 1 exchange probe")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's outputs and gradients to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="--full without the second flavour and the stability window (headline window + roofline only)")
    ap.add_argument("--stability-steps", type=int, default=300)
    ap.add_argument("--cpu-runs", type=int, default=10, help="timed runs of the torch CPU baseline (batch 2 each)")
    ap.add_argument("--cpu-images", type=int, default=10, help="images of the numpy CPU baseline (batch 1 each)")
    args = ap.parse_args()

    from cocosnet_amd import dist as cdist
    from cocosnet_amd import ops
    if args.precision:
        ops.PRECISION = args.precision
        ops.PROJ_PRECISION = args.precision      # K0 follows (COCOS_PROJ_PRECISION overrides it separately)
    rank, local_rank, world = cdist.init_from_env("nccl")
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    torch.manual_seed(0)     # the parameters' initialisation: identical inputs and weights from run to run
    model, fwd = make_step(args.scope, device, args.match_kernel)
    # stand-ins for the rest of the replica's parameters (BASELINE config 4): fp32 tensors whose gradients are written
    # every step by autograd — first in backward order, like the generator's — and exchanged with the real ones
    extra = []
    if world > 1 and PAYLOAD_PARAMS[args.grad_payload]:
        own = sum(p.numel() for p in model.parameters())
        left = max(PAYLOAD_PARAMS[args.grad_payload] - own, 0)
        while left > 0:
            n = min(left, 16 << 20)                      # 64 MiB tensors: one bucket each
            extra.append(torch.nn.Parameter(torch.zeros(n, device=device)))
            left -= n
    params = list(model.parameters()) + extra
    if world > 1:   # identical replicas: broadcast rank 0's parameters once
        for p in model.parameters():
            torch.distributed.broadcast(p.data, 0)
    # N = 1: no exchange, gradients are plain tensors (p.grad = None per step, as the reference's optimizer.zero_grad
    # does); N > 1: flat buckets, p.grad views, hook-driven overlap
    buckets = cdist.GradBuckets(params) if world > 1 else None
    d = build_inputs(device, args.scope)
    ones = [torch.ones((), device=device) for _ in extra]
    fwd_box = [fwd]          # the forward the step runs (the match_kernel-3 context window swaps it)
    last = {}                # --dump-outputs: the latest step's outputs, detached (the autograd graph is not kept alive)

    def step():
        if buckets is not None:
            buckets.zero_grad()
        else:
            for p in params:
                p.grad = None
        for k in ("cont_features", "ref_features"):
            if k in d:
                d[k].grad = None
        out = fwd_box[0](d)
        # backward of the synthetic loss <warp_out, G_out> + <warp_mask, G_mask>: its gradients w.r.t. the two
        # outputs ARE the fixed tensors G, so they are fed to autograd directly (no loss kernels in the timing).
        # Gradient buckets leave for the all-reduce from autograd's hooks, while backward is still running.
        roots = [out["warp_out"], out["warp_mask"]] + [e.sum() for e in extra]
        torch.autograd.backward(roots, [d["g_out"], d["g_mask"]] + ones)
        if buckets is not None:
            buckets.finish(world)
        if args.dump_outputs:
            last.clear()
            last.update((k, v.detach()) for k, v in out.items() if torch.is_tensor(v))

    sync = lambda: (torch.distributed.barrier() if world > 1 else None, torch.cuda.synchronize())

    def window(steps, warmup, tags=HOT_TAGS):
        """W untimed steps, then exactly `steps` timed ones between barrier + synchronize; MAX over ranks."""
        for _ in range(warmup):
            step()
        sync()
        # Live HIP-event timing inside the timed region, but only around the kernels the roofline is about: every
        # event is a marker packet that serialises dispatch (~3.5 us); bracketing all ~40 C-ABI calls of a step
        # costs 8 % of it.  The complete per-call breakdown comes from one extra, untimed step afterwards.
        with ops.KernelTimer(tags=tags) as kt:
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            sync()
            dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt, kt.summary()

    headline_precision = ops.PRECISION
    # set-up, outside the W + K contract: the first calls load every kernel's code object (the K2 kernels exist in two
    # instantiations each), size the caching allocator's pools and the max|x| cell pool — not steady-state work
    SETUP_STEPS = 3
    for _ in range(SETUP_STEPS):
        step()
    sync()
    # A plain run times the steps with no HIP event in them: the per-kernel table and the roofline are --full's.
    timed_tags = ()
    if args.full:
        # Round 5: the timed window carries HIP events around the DOMINANT kernel only (the one `roofline` is about: ④ asks for
        # its launch time measured live over the timed region) — every bracketed call costs two marker packets that serialise
        # dispatch, and six per step were 2-3 % of `value`.  Which kernel that is comes from one fully-bracketed, untimed step;
        # the other hot kernels' live averages come from a second window of the same length right after the headline one.
        # the probe is a steady-state window of its own (30 steps after 5 unbracketed ones, all three MFMA kernels bracketed): on an
        # idle queue an event pair also spans the host's launch latency, and a five-step probe right after a synchronisation ranked
        # the forward above the query backward on some boxes
        _, probe = window(30, 5, tags=HOT_TAGS)
        # (round 6: ONE kernel stays bracketed in the timed window — since the forward's QK loop accumulates in one chain the query
        #  backward is the longest by > 10 %; the second bracket cost another 1.4 % of `value`).  Ranked by the SHORTEST bracket:
        #  the kernel itself
        dom_tags = tuple(sorted(probe, key=lambda t: -probe[t].get("min_ms", probe[t]["avg_ms"]))[:1])
        timed_tags = dom_tags if dom_tags else HOT_TAGS
    dt, kern = window(args.steps, args.warmup, tags=timed_tags)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, model, d)
    kern_all, kern_timed = {}, {}
    if args.full:
        with ops.KernelTimer() as kt_all:
            step()
        kern_all = kt_all.summary()
        _, kern_hot = window(args.steps, 0)              # all hot kernels bracketed: the `kernels` table (never part of `value`)
        kern_timed = dict(kern)                          # what the timed window itself measured: `roofline` is computed from these
        for tag, rec in kern_hot.items():
            kern.setdefault(tag, rec)                    # (the bracketed kernels keep their figures from the headline window)

    # ---- extras, same process / same box, after the headline window (N = 1 only) --------------------------------
    flavours, stability, context = {}, None, None
    if args.full and world == 1 and not args.no_extras and args.scope == "hotpath":
        sdt, _ = window(args.stability_steps, 0, tags=())
        stability = {"steps": args.stability_steps, "ms_per_step": round(sdt / args.stability_steps * 1e3, 4),
                     "images_per_s": round(BATCH_PER_GPU * args.stability_steps / sdt, 1),
                     "note": "untimed-contract window right after the headline one: no HIP events, same step"}
        other = "fp32" if headline_precision == "f16x3" else "f16x3"
        ops.PRECISION = ops.PROJ_PRECISION = other
        odt, okern = window(args.steps, 3)
        ok = kernel_table(okern, other)
        flavours[other] = {"ms_per_step": round(odt / args.steps * 1e3, 4),
                           "images_per_s": round(BATCH_PER_GPU * args.steps / odt, 1), "steps": args.steps,
                           "kernels": ok, "roofline": roofline_of(ok, other)}
        ops.PRECISION = ops.PROJ_PRECISION = headline_precision
        # the same step with the value-lo skipping switched off: what a workload WITHOUT exactly-representable label
        # channels gets (BASELINE configs 3 and 5 carry float label maps) — the headline benefits from ADE20k's one-hot map
        if headline_precision == "f16x3" and ops.VALUE_LO_SKIP:
            ops.VALUE_LO_SKIP = False
            gdt, gkern = window(args.steps, 3)
            gk = kernel_table(gkern, headline_precision)
            flavours["general_v"] = {"ms_per_step": round(gdt / args.steps * 1e3, 4),
                                     "images_per_s": round(BATCH_PER_GPU * args.steps / gdt, 1), "steps": args.steps,
                                     "kernels": gk, "note": "COCOS_VALUE_LO_SKIP=0: every V_lo term issued (78 MFMAs per "
                                                            "32-key wave tile instead of 70)"}
            ops.VALUE_LO_SKIP = True
        # context: the reference's SHIPPED default match_kernel 3 on the same inputs (fused family K19 / K20)
        if args.match_kernel == 1:
            model3, fwd3 = make_step(args.scope, device, 3)
            n_own = len(params)
            params.extend(model3.parameters())            # their gradients are reset by the step like the headline model's
            try:
                fwd_box[0] = fwd3
                mdt, mkern = window(args.steps, 3, tags=())
                with ops.KernelTimer() as kt3:
                    step()
                context = {"match_kernel_3": {"ms_per_step": round(mdt / args.steps * 1e3, 4),
                                              "images_per_s": round(BATCH_PER_GPU * args.steps / mdt, 1),
                                              "abi_calls_ms_per_step": {t: round(r["total_ms"], 4)
                                                                        for t, r in sorted(kt3.summary().items())},
                                              "note": "same step with match_kernel 3 (options/base_options.py:70): x box in "
                                                      "the correlation GEMM's epilogue, y box + softmax + warp in one kernel"}}
            finally:
                fwd_box[0] = fwd
                del params[n_own:]
            del model3
        # context: the whole drop-in module (feature producers + the path) on the same inputs, in its two convolution flavours —
        # never part of `value`, never allowed to cost the line
        if args.scope == "hotpath":
            context = dict(context or {})
            try:
                context["config5"] = config5_context(device)
            except Exception as e:       # noqa: BLE001
                context["config5"] = {"error": repr(e)}
            try:
                context["config3"] = config3_context(device)
                context["config3"]["hot_path"] = config3_hot_path_context(device)
            except Exception as e:       # noqa: BLE001
                context["config3"] = {"error": repr(e)}
            torch.cuda.empty_cache()
            try:
                context["module_scope"] = module_scope_context(device, d)
            except Exception as e:       # noqa: BLE001
                context["module_scope"] = {"error": repr(e)}

    # N > 1: what BASELINE config 4's exchanges cost on this node — timed AFTER the contract window, never part of `value`:
    # one in-place all-reduce (RCCL) of a flat fp32 buffer of netCorr's 59 M and of netG+netCorr's 156 M gradients
    exchange_probe = None
    if args.full and world > 1 and not args.no_extras:
        try:
            exchange_probe = {}
            for name in ("netcorr", "full"):
                buf = torch.zeros(PAYLOAD_PARAMS[name], device=device)
                for _ in range(2):
                    torch.distributed.all_reduce(buf)
                sync()
                t0 = time.perf_counter()
                for _ in range(5):
                    torch.distributed.all_reduce(buf)
                sync()
                ms = (time.perf_counter() - t0) / 5 * 1e3
                nbytes = buf.numel() * 4
                exchange_probe[name] = {"bytes": nbytes, "ms": round(ms, 3),
                                        "bus_GBps": round(nbytes * 2 * (world - 1) / world / (ms * 1e-3) / 1e9, 1)}
                del buf
        except Exception as e:       # noqa: BLE001 — a probe must never cost the bench line
            exchange_probe = {"error": repr(e)}

    if rank == 0:
        split = headline_precision == "f16x3"
        kernels = kernel_table(kern, headline_precision) if args.full else None
        roofline = roofline_of(kernel_table(kern_timed, headline_precision) or kernels, headline_precision) if args.full else None
        # device time of EVERY C-ABI call per step (ms), so the part of the step outside the three big kernels is visible
        per_step = {tag: round(rec["total_ms"], 4) for tag, rec in sorted(kern_all.items())} if args.full else None
        cpu = None
        if args.full and not args.no_cpu_baseline and world == 1:   # reported at N=1 only (bounded sample)
            cpu = cpu_baseline(args.cpu_runs)
            cpu["numpy_port"] = cpu_baseline_numpy(args.cpu_images)
        images = BATCH_PER_GPU * world * args.steps
        line = {
            "metric": "images/sec fwd+bwd ADE20k 256x256 batch-8/GPU (correspondence hot path)",
            "value": round(images / dt, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "setup_steps": SETUP_STEPS, "ms_per_step": round(dt / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32 (K2 products as 3-term f16 hi/lo split on the f16 MFMA, fp32 accumulate)" if split else "f32",
            "data": "synthetic",
            "config": {"workload": f"ADE20k 256x256 batch {BATCH_PER_GPU}/GPU, 64x64 grid (HW=4096), K=256, "
                                   f"Cv=154 (rgb+151 labels), match_kernel {args.match_kernel}, PONO_C, T=0.01; "
                                   f"precision={headline_precision}; scope={args.scope}: "
                                   + ("theta/phi 1x1 conv + centre/L2norm + fused corr-softmax-warp fwd+bwd"
                                      if args.scope == "hotpath" else
                                      "whole NoVGGCorrespondence module fwd+bwd (convolutions K16, norms K9/K13/K17, theta/phi K0); "
                                      f"convolutions={_conv_flavour()}"),
                       "untimed_steps_before_window": SETUP_STEPS + (1 if args.full else 0) + args.warmup,
                       "hip_events_in_timed_window": list(timed_tags),
                       # hygiene: `value` is measured on ADE20k's one-hot label map, whose V_lo MFMA term is
                       # skipped; the same step with every term issued (what configs 3 and 5, with float label maps, get):
                       "value_with_general_v": (flavours.get("general_v") or {}).get("images_per_s"),
                       "step_definition": "bench step = theta/phi 1x1 projections (K0) + centre/L2-norm (K1) + the correspondence "
                                          "kernels, forward and backward; tools/configs_bench.py's step starts at theta/phi (no K0): "
                                          "its match_kernel-3 figure is ~0.2 ms below context.match_kernel_3.ms_per_step",
                       "context": context,
                       "global_batch": BATCH_PER_GPU * world, "parallelism": f"dp{world}",
                       "grad_payload": args.grad_payload,
                       "grad_allreduce_bytes": buckets.nbytes() if buckets is not None else 0,
                       "grad_allreduce": "bucketed (64 MiB), launched from post-accumulate-grad hooks during backward, "
                                         "in place on flat fp32 gradient buffers" if world > 1 else None},
            "roofline": roofline, "kernels": kernels, "abi_calls_ms_per_step": per_step,
            "flavours": flavours, "stability": stability, "cpu_baseline": cpu, "exchange_probe": exchange_probe,
            "full": args.full,
        }
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
