"""The loss block of the generator step (cocosnet_amd.losses.generator_losses + discriminator_losses, forward + backward) on two
arms in ONE process, interleaved round by round:
  unfused   losses.FUSED = False: the framework's ops in the reference's order (what runs without this module)
  fused     the K28 kernels
Shapes: "ade20k" = B 8, 256 x 256, VGG levels r12 ... r52, 2 x 4 PatchGAN feature maps, a [8, 151, 64, 64] warp mask with the
direct mask loss; "celebahq" = the same networks with --warp_cycle_w 1 --two_cycle, warp_self_w > 0 and no mask loss.
Reported per shape and arm: median and min / max ms per step over the timed repetitions (CUDA events around each repetition, warm-up
discarded), C-ABI calls per step, and the peak of max_memory_allocated above the inputs (the step's gradients count).  Also: the rate
of the pair_loss forward and backward at the 256 MB-per-side r12 ... r52 group against a device-to-device copy measured in the
same run.
Usage (GPU box): python tools/loss_bench.py [--out FILE.txt] [--reps 25] [--warmup 5]"""
import argparse
import os
import statistics
import sys

import torch

import benchlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from cocosnet_amd import _lib, losses, ops  # noqa: E402
import loss_case  # noqa: E402


def make_step(shape, dev, B=8, S=256, nc=151):
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    img = lambda hh, ww: torch.rand(B, 3, hh, ww, device=dev, generator=g) * 2 - 1
    feats = [(64, S, S), (128, S // 2, S // 2), (256, S // 4, S // 4), (512, S // 8, S // 8), (512, S // 16, S // 16)]
    # PatchGAN (n_layers_D 4, num_D 2) on a 256 x 256 and a 128 x 128 input: three k4 s2 layers, two k4 s1 layers
    d_shapes = [[(64, 129, 129), (128, 65, 65), (256, 33, 33), (512, 34, 34), (1, 35, 35)],
                [(64, 65, 65), (128, 33, 33), (256, 17, 17), (512, 18, 18), (1, 19, 19)]]
    d_shapes = [d[:3] + d[4:] for d in d_shapes]                       # 2 x (3 intermediate + final): the 2 x 4 maps of the step
    name = "ade20k" if shape == "ade20k" else "celebahq"
    opt = loss_case.options(name)
    lab = lambda: torch.randint(0, nc, (B, 1, S // 8, S // 8), device=dev, generator=g).repeat_interleave(8, 2).repeat_interleave(8, 3)
    inputs = {
        "label": lab(), "ref_label": lab(), "self_ref": (torch.arange(B, device=dev) % 2).float().view(B, 1, 1, 1),
        "real_image": img(S, S), "ref_image": img(S, S), "fake_image": img(S, S),
        "warp_out": img(S, S), "warp_cycle": img(S // 4, S // 4), "warp_i2r2i": img(S // 4, S // 4),
        "warp_mask": torch.softmax(rnd(B, nc, S // 4, S // 4), dim=1),
        "real_features": [rnd(B, *s) for s in feats], "ref_features": [rnd(B, *s) for s in feats[:1]],
        "fake_features": [rnd(B, *s) for s in feats],
        "pred_fake": [[rnd(B, *s) for s in d] for d in d_shapes], "pred_real": [[rnd(B, *s) for s in d] for d in d_shapes],
    }
    loss_case.require_grad(inputs)
    model = loss_case.StubModel(opt, inputs, losses.GANLoss, losses.L1Loss, float_tensor=torch.cuda.FloatTensor)

    def step():
        for _, t in loss_case.leaves(inputs):
            t.grad = None
        G, _ = loss_case.run_generator(losses.compute_generator_loss, model)
        loss_case.total(G).backward()
        D = loss_case.run_discriminator(losses.compute_discriminator_loss, model)
        loss_case.total(D).backward()

    return step, inputs


def stats(ms):
    s = benchlib.summary(ms)
    return f"median {s.median:8.3f} ms  min {s.min:8.3f}  max {s.max:8.3f}  (n = {len(ms)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: needs the GPU")
    dev = torch.device("cuda", 0)
    lines = [f"loss_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, reps {a.reps}, warm-up {a.warmup}"]
    calls, real_call = [0], _lib.call

    def counting(name, *args):
        calls[0] += 1
        return real_call(name, *args)

    def counted(step):
        calls[0], _lib.call = 0, counting
        try:
            step()
        finally:
            _lib.call = real_call

    for shape in ("ade20k", "celebahq"):
        step, inputs = make_step(shape, dev)
        ms, peak, ncalls = {"unfused": [], "fused": []}, {}, {}
        for rep in range(a.warmup + a.reps):
            for arm in ("unfused", "fused"):              # interleaved: both arms see the same clocks and allocator state
                losses.FUSED = arm == "fused"
                t = benchlib.time_calls(step, 1)
                if rep >= a.warmup:
                    ms[arm].append(t)
        for arm in ("unfused", "fused"):
            losses.FUSED = arm == "fused"
            for _, t in loss_case.leaves(inputs):         # the previous step's gradients go first: the peak then counts this step's
                t.grad = None
            peak[arm], ncalls[arm] = benchlib.peak_bytes(lambda: counted(step)) / 2 ** 20, calls[0]
        losses.FUSED = True
        for arm in ("unfused", "fused"):
            lines.append(f"{shape:9s} {arm:8s} {stats(ms[arm])}  C-ABI calls {ncalls[arm]:3d}  peak above the inputs (gradients included) {peak[arm]:9.1f} MiB")
        unfused = benchlib.summary(ms["unfused"])
        lines.append(f"{shape:9s} fused / unfused = {statistics.median(ms['fused']) / unfused.median:.3f}; spread of the unfused arm "
                     f"(max - min) / median = {unfused.spread:.3f}")
        if shape == "ade20k":
            # the fm + perc group on its own against a copy of the same bytes
            fake, realf = inputs["fake_features"], [t.detach() for t in inputs["real_features"]]
            sw = losses._sample_weights(inputs["self_ref"]).detach()
            side = sum(t.numel() * 4 for t in fake)
            segs = [(f, r, sw, w, float(i == 4)) for i, (f, r, w) in enumerate(zip(fake, realf, losses._VGG_LEVEL_WEIGHTS))]
            dst = [torch.empty_like(t) for t in fake]
            out = ops.pair_loss(segs)
            gout = torch.ones_like(out)
            copy = lambda: [d.copy_(t.detach()) for d, t in zip(dst, fake)]
            fwd = lambda: ops.pair_loss(segs)
            bwd = lambda: torch.autograd.grad(out, fake, gout, retain_graph=True)
            t_copy, t_fwd, t_bwd = [], [], []
            for rep in range(a.warmup + a.reps):
                for fn, acc in ((copy, t_copy), (fwd, t_fwd), (bwd, t_bwd)):
                    t = benchlib.time_calls(fn, 1)
                    if rep >= a.warmup:
                        acc.append(t)
            rate = lambda nbytes, t: nbytes / (statistics.median(t) * 1e-3) / 1e12
            r_copy, r_fwd, r_bwd = rate(2 * side, t_copy), rate(2 * side, t_fwd), rate(3 * side, t_bwd)
            lines.append("(every repetition re-reads the same buffers: with a 256 MiB last-level cache on the die part of the traffic of all "
                         "three rows may be served from it; the rates are relative to the copy under the same conditions, not HBM figures)")
            lines.append(f"pair_loss at {side / 1e6:.0f} MB per side: copy {stats(t_copy)} = {r_copy:.2f} TB/s (read + write)")
            lines.append(f"  forward  (2 reads)           {stats(t_fwd)} = {r_fwd:.2f} TB/s = {r_fwd / r_copy:.2f} of the copy rate")
            lines.append(f"  backward (2 reads + 1 write) {stats(t_bwd)} = {r_bwd:.2f} TB/s = {r_bwd / r_copy:.2f} of the copy rate")
        del step, inputs
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
