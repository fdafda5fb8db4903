"""K26 (fused parameter-free norm + SPADE modulation + LeakyReLU, ops.norm_spade) against today's route (the norm module, then K17),
as the same-box A/B of the `spade.NORM_FUSED` hook, in ONE process: fwd+bwd ms per step (median of several timed runs after
warm-ups), effective GB/s of the K26 kernels (counted traffic: forward 20 B / element, backward 44 B / element, over their
device time) and peak memory, for
  * one non-PONO SPADEResnetBlock at netG's 256x256 stage ([16, 128, 256, 256] -> 64 channels) with batch, sync-batch (world size 1)
    and instance norm;
  * the whole NoVGGCorrespondence with ade20k_options(PONO=False) at B = 8;
  * translation.SPADEGenerator with the CelebA-HQ edge flags without --PONO at B = 16.
Usage (GPU box): python tools/norm_spade_bench.py [--out FILE.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import torch

import benchlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cocosnet_amd import ops, spade  # noqa: E402

FWD_BYTES, BWD_BYTES = 20, 44


class _Traffic:
    """Counts the elements the K26 passes touch (wrapping the two apply steps the autograd Function calls)."""

    def __init__(self):
        self.fwd = self.bwd = 0
        self._apply, self._bwd_apply = ops.norm_spade_apply, ops.norm_spade_bwd_apply

    def __enter__(self):
        def apply(x, *a, **k):
            self.fwd += x.numel()
            return self._apply(x, *a, **k)

        def bwd_apply(x, *a, **k):
            self.bwd += x.numel()
            return self._bwd_apply(x, *a, **k)
        ops.norm_spade_apply, ops.norm_spade_bwd_apply = apply, bwd_apply
        return self

    def __exit__(self, *exc):
        ops.norm_spade_apply, ops.norm_spade_bwd_apply = self._apply, self._bwd_apply


def _timed_runs(step, warmup, iters, reps):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    runs = [benchlib.time_calls(step, iters) for _ in range(reps)]
    return statistics.median(runs), runs


def _measure(name, step, warmup, iters, reps):
    res = {}
    for fused in (True, False, True, False):           # alternated: the second pair says how much the box moved in between
        spade.NORM_FUSED = fused
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms, runs = _timed_runs(step, warmup, iters, reps)
        peak = torch.cuda.max_memory_allocated() / 2**30
        key = "fused" if fused else "module+K17"
        res.setdefault(key, {"ms": [], "runs": [], "peak_GiB": peak})
        res[key]["ms"].append(ms)
        res[key]["runs"] += runs
    spade.NORM_FUSED = True
    for v in res.values():
        v["median_ms"] = statistics.median(v["runs"])
    with _Traffic() as tr, ops.KernelTimer(tags={"norm_spade_fwd", "norm_spade_bwd"}) as kt:
        step()
        s = kt.summary()
    fwd_ms = s.get("norm_spade_fwd", {}).get("total_ms", 0.0)
    bwd_ms = s.get("norm_spade_bwd", {}).get("total_ms", 0.0)
    res["k26"] = {"fwd_ms": fwd_ms, "bwd_ms": bwd_ms, "fwd_calls": s.get("norm_spade_fwd", {}).get("calls", 0),
                  "fwd_GBps": FWD_BYTES * tr.fwd / (fwd_ms * 1e6) if fwd_ms else None,
                  "bwd_GBps": BWD_BYTES * tr.bwd / (bwd_ms * 1e6) if bwd_ms else None}
    f, m = res["fused"]["median_ms"], res["module+K17"]["median_ms"]
    print(f"{name}: fused {f:.2f} ms ({res['fused']['peak_GiB']:.2f} GiB peak) | module+K17 {m:.2f} ms "
          f"({res['module+K17']['peak_GiB']:.2f} GiB) | speed-up {m / f:.3f}x | K26 fwd {fwd_ms:.2f} ms "
          f"{res['k26']['fwd_GBps'] or 0:.0f} GB/s, bwd {bwd_ms:.2f} ms {res['k26']['bwd_GBps'] or 0:.0f} GB/s", flush=True)
    return res


def block_case(kind, B, fin, fout, hw):
    from cocosnet_amd import correspondence as cc
    from cocosnet_amd.producers import SPADEResnetBlock
    norm = {"batch": "spectralspadebatch3x3", "syncbatch": "spectralspadesyncbatch3x3", "instance": "spectralspadeinstance3x3"}[kind]
    opt = cc.base_options(semantic_nc=15, norm_G=norm, PONO=False, CBN_intype="warp_mask")
    blk = SPADEResnetBlock(fin, fout, opt).cuda().train()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, fin, hw, hw, device="cuda", generator=g).requires_grad_(True)
    seg = torch.rand(B, 18, hw, hw, device="cuda", generator=g)
    gy = torch.randn(B, fout, hw, hw, device="cuda", generator=g)

    def step():
        x.grad = None
        blk.zero_grad(set_to_none=True)
        blk(x, seg).backward(gy)
    return step


def netcorr_case(B):
    from cocosnet_amd import correspondence as cc
    opt = cc.ade20k_options(PONO=False, isTrain=True)
    net = cc.NoVGGCorrespondence(opt).cuda()
    net.init_weights(opt.init_type, opt.init_variance)
    net.train()
    g = torch.Generator(device="cuda").manual_seed(0)
    size, nc = opt.crop_size, opt.semantic_nc
    img = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    real = torch.rand(B, 3, size, size, device="cuda", generator=g) * 2 - 1
    lab = torch.randint(0, nc, (B, 1, size, size), device="cuda", generator=g)
    seg = torch.zeros(B, nc, size, size, device="cuda").scatter_(1, lab, 1.0)
    ref_seg = seg.flip(0).contiguous()

    def step():
        net.zero_grad(set_to_none=True)
        out = net(img, real, seg, ref_seg)
        loss = sum(v.float().mean() for v in out.values() if torch.is_tensor(v) and v.requires_grad)
        loss.backward()
    return step


def generator_case(B):
    from cocosnet_amd import translation as tl
    opt = tl.celebahq_edge_train_options(PONO=False)
    G = tl.SPADEGenerator(opt).cuda()
    G.init_weights(opt.init_type, opt.init_variance)
    G.train()
    g = torch.Generator(device="cuda").manual_seed(0)
    seg = torch.rand(B, 15, 256, 256, device="cuda", generator=g)
    cbn = torch.cat((torch.rand(B, 3, 256, 256, device="cuda", generator=g) * 2 - 1, seg), 1)
    gy = torch.randn(B, 3, 256, 256, device="cuda", generator=g)

    def step():
        G.zero_grad(set_to_none=True)
        G(seg, warp_out=cbn).backward(gy)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal, not a measurement)")
    ap.add_argument("--only", default=None, help="comma list of case names")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("norm_spade_bench: needs the GPU (no CPU timing is reported)")
    q = a.quick
    cases = {}
    for kind in ("batch", "syncbatch", "instance"):
        cases[f"block_{kind}"] = (lambda k=kind: block_case(k, 2 if q else 16, 32 if q else 128, 16 if q else 64, 32 if q else 256),
                                  (1, 2, 3) if q else (2, 3, 5))
    cases["netcorr_B8"] = (lambda: netcorr_case(2 if q else 8), (1, 1, 3) if q else (2, 2, 5))
    cases["generator_B16"] = (lambda: generator_case(2 if q else 16), (1, 1, 3) if q else (2, 2, 5))
    only = set(a.only.split(",")) if a.only else None
    result = {"box": torch.cuda.get_device_name(0), "torch": torch.__version__, "conv_precision": ops.CONV_PRECISION, "cases": {}}
    print("box:", result["box"], flush=True)
    for name, (make, (warmup, iters, reps)) in cases.items():
        if only and name not in only:
            continue
        step = make()
        result["cases"][name] = _measure(name, step, warmup, iters, reps)
        del step
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
