"""The tail of the reference's training step on this package's kernels (K29): `optimizer_G.step()` / `optimizer_D.step()` and, with
`--use_ema`, the two `EMA.__call__`s of `Pix2PixTrainer.run_generator_one_step` (trainers/pix2pix_trainer.py:52-74).

    trainer = Pix2PixTrainer(opt)              # the reference's, or cocosnet_amd.trainer's DistributedTrainer
    optim.fuse_trainer(trainer)                # Adam of both optimisers and both EMAs: one multi-tensor launch per 64 tensors

`fuse_adam` takes the `torch.optim.Adam` INSTANCE the reference built (Pix2PixModel.create_optimizers, update_fixed_params) and
replaces its `step`; state, `state_dict()` / `load_state_dict()`, `param_groups` and `zero_grad()` stay the framework's, so the
reference's `optimizer.pth` is interchangeable in both directions.  `EMA` is the reference's class (models/networks/generator.py
:259-287) with `__call__` as one multi-tensor launch that updates the shadows in place.  Every route is opt-in and switches back
to the framework's with `FUSED = False`.
"""
from __future__ import annotations

import importlib
import sys

import torch

from . import ops

#: A/B switch, read at call time: False = the framework's Adam step and the reference's EMA expression in torch ops
FUSED = True
#: the kernel route of `fuse_adam` (needs FUSED as well).  Shipped OFF: in tools/optim_bench.py's run on an MI355X
#: (profiles/k29_optim_bench.json) a fused step is bound by this module's per-tensor Python work, not by its kernel - it beats the
#: framework's default route but not torch.optim.Adam(fused=True), the better framework arm.  `optim.ADAM_FUSED = True` turns it on;
#: the GPU tests run with it on.  The EMA route cleared the same rule and follows FUSED alone.
ADAM_FUSED = False

_GROUP_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused", "decoupled_weight_decay")


def _dense_f32(t, device) -> bool:
    return (torch.is_tensor(t) and t.device == device and t.dtype == torch.float32 and t.layout == torch.strided
            and t.is_contiguous() and t.numel() > 0)


def _collect(optimizer):
    """The work of one fused step: (params, grads, exp_avgs, exp_avg_sqs, steps, group of each) over the parameters that have a
    gradient, creating missing state as torch.optim.Adam._init_group does — or None when anything asks for the framework's step."""
    if getattr(optimizer, "grad_scale", None) is not None or getattr(optimizer, "found_inf", None) is not None:
        return None
    P, G, M, V, S, K = [], [], [], [], [], []
    device = None
    for k, group in enumerate(optimizer.param_groups):
        if any(group.get(flag) is True for flag in _GROUP_FLAGS):
            return None
        beta1, beta2 = group["betas"]
        if not all(isinstance(x, (int, float)) for x in (group["lr"], beta1, beta2, group["eps"], group["weight_decay"])):
            return None                                   # tensor hyper-parameters: the framework's business
        for p in group["params"]:
            if device is None:
                device = p.device
                if device.type != "cuda" or device.index != torch.cuda.current_device():
                    return None
            if not _dense_f32(p, device):
                return None                               # every parameter, with a gradient or not: whole optimiser, not per tensor
            g = p.grad
            if g is None:
                continue
            if not _dense_f32(g, device):
                return None
            state = optimizer.state[p]
            if len(state) == 0:
                scalar = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
                state["step"] = torch.tensor(0.0, dtype=scalar)           # on the host, as the framework keeps it
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            step, m, v = state["step"], state["exp_avg"], state["exp_avg_sq"]
            if not (torch.is_tensor(step) and step.device.type == "cpu" and _dense_f32(m, device) and _dense_f32(v, device)
                    and m.numel() == p.numel() == v.numel() == g.numel()):
                return None
            P.append(p); G.append(g); M.append(m); V.append(v); S.append(step); K.append(k)
    return P, G, M, V, S, K


def _group_row(group, t: float):
    """(lr / bc1, sqrt(bc2), beta1, 1 - beta1, beta2, 1 - beta2, eps, weight_decay) at step count t, formed in double; the binding
    rounds each once to fp32"""
    beta1, beta2 = (float(b) for b in group["betas"])
    return (float(group["lr"]) / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5, beta1, 1.0 - beta1, beta2, 1.0 - beta2,
            float(group["eps"]), float(group["weight_decay"]))


def _has_step_hooks(optimizer) -> bool:
    """step pre / post hooks (`register_step_pre_hook`, `register_step_post_hook`, on the instance or global) run inside the
    framework's own `step`; the kernel route does not go through it"""
    import torch.optim.optimizer as _o
    return bool(getattr(optimizer, "_optimizer_step_pre_hooks", None) or getattr(optimizer, "_optimizer_step_post_hooks", None)
                or getattr(_o, "_global_optimizer_pre_hooks", None) or getattr(_o, "_global_optimizer_post_hooks", None))


def fuse_adam(optimizer):
    """Replace `optimizer.step` (a torch.optim.Adam instance) by the multi-tensor kernel step; returns the optimiser.

    The fused step reads `param_groups` (lr, betas, eps, weight_decay), gradients, parameters and state tensors afresh on every
    call, skips parameters without a gradient (their `step` does not advance), and keeps `optimizer.state[p]` = {"step" (CPU fp32
    scalar), "exp_avg", "exp_avg_sq"} exactly as the framework keeps it.  The whole optimiser takes the step it had before
    (`optimizer.step` at the time of this call) when `FUSED` or `ADAM_FUSED` is false, a closure is passed, a parameter,
    gradient or state tensor is not a dense contiguous fp32 tensor on the current GPU, a group sets amsgrad / maximize /
    capturable / differentiable / foreach / fused / decoupled_weight_decay, or a step pre / post hook is registered (on the
    optimiser or globally): hooks run inside the framework's `step`, which the kernel route does not call.  The kernel route
    also leaves no `Optimizer.step#...` record in a torch profiler trace.  `optimizer.cocos_last_launches`: the kernel launches
    of the last fused step, as counted by the library.

    Composes with `cocosnet_amd.trainer.attach_gradient_exchange` in either order: attached afterwards, the exchange wraps this
    step; attached before, this step completes the exchange itself (`optimizer.grad_buckets.finish()`, idempotent) before it
    reads the gradients.  Any OTHER wrapper already around `step` would be bypassed by the fused route, so it is refused."""
    if not isinstance(optimizer, torch.optim.Adam):
        raise TypeError(f"fuse_adam: expected a torch.optim.Adam instance, got {type(optimizer).__name__}")
    if getattr(optimizer, "cocos_fused", False):
        return optimizer
    previous = optimizer.step
    plain = getattr(previous, "__func__", None) is type(optimizer).step
    if not plain and getattr(previous, "cocos_grad_buckets", None) is None:
        raise TypeError("fuse_adam: optimizer.step is already wrapped by something this package does not know (a learning-rate "
                        "scheduler?); the fused route would bypass it - call fuse_adam first")

    def step(closure=None):
        if not (FUSED and ADAM_FUSED) or closure is not None or _has_step_hooks(optimizer):
            return previous(closure) if closure is not None else previous()
        buckets = getattr(optimizer, "grad_buckets", None)
        if buckets is not None:
            buckets.finish()          # what the wrapped step does first (idempotent); it may re-attach p.grad, so before reading it
        work = _collect(optimizer)
        if work is None:
            return previous()
        P, G, M, V, S, K = work
        optimizer.cocos_last_launches = 0
        if not P:
            return None
        counts = torch.stack(S).tolist()                  # CPU tensors: no device read
        rows, index, row_of = [], [], {}
        for k, t in zip(K, counts):
            r = row_of.get((k, t))
            if r is None:                                 # parameters of one group whose step counts differ: different rows
                r = row_of[(k, t)] = len(rows)
                rows.append(_group_row(optimizer.param_groups[k], t + 1.0))
            index.append(r)
        optimizer.cocos_last_launches = ops.adam_multi_step(P, G, M, V, rows, index, validate=False)     # _collect has checked every tensor
        torch._foreach_add_(S, 1.0)
        return None

    step.cocos_fused_adam = True
    optimizer.step = step
    optimizer.cocos_fused = True
    return optimizer


class EMA:
    """The reference's EMA (models/networks/generator.py:259-287), same attributes and methods; `__call__` is one multi-tensor
    launch over all `requires_grad` parameters that updates the shadow tensors IN PLACE (the reference rebinds `shadow[name]` to
    a fresh tensor per parameter and step).  CPU / non-fp32 parameters or `FUSED = False`: the reference's expression in torch
    ops."""

    def __init__(self, mu, shadow=None):
        self.mu = mu
        self.shadow = {} if shadow is None else shadow    # an existing EMA's dictionary is adopted as it is
        self.original = {}

    def register(self, name, val):
        self.shadow[name] = val.clone()

    def __call__(self, model):
        named = [(name, p) for name, p in model.named_parameters() if p.requires_grad]
        for name, _ in named:
            assert name in self.shadow
        if not named:
            return
        shadows = [self.shadow[name] for name, _ in named]
        params = [p.data for _, p in named]
        dev = params[0].device
        if (FUSED and dev.type == "cuda" and dev.index == torch.cuda.current_device()
                and all(_dense_f32(p, dev) and _dense_f32(s, dev) and s.numel() == p.numel() and s.data_ptr() != p.data_ptr()
                        for s, p in zip(shadows, params))):
            self.cocos_last_launches = ops.ema_multi_update(shadows, params, float(self.mu))
            return
        decay = self.mu
        for (name, _), s, p in zip(named, shadows, params):
            self.shadow[name] = ((1.0 - decay) * p + decay * s).clone()

    def assign(self, model):
        for name, param in model.named_parameters():
            if param.requires_grad:
                assert name in self.shadow
                self.original[name] = param.data.clone()
                param.data = self.shadow[name]

    def resume(self, model):
        for name, param in model.named_parameters():
            if param.requires_grad:
                assert name in self.shadow
                param.data = self.original[name]


def fuse_trainer(trainer):
    """An already constructed `Pix2PixTrainer` (or `cocosnet_amd.trainer`'s DistributedTrainer) -> the same object with
    `fuse_adam` on `optimizer_G` / `optimizer_D` where present, with `netG_ema` / `netCorr_ema` replaced by `EMA` objects that
    adopt the existing shadow dictionaries when `opt.use_ema`, and with `update_fixed_params` (which builds a new optimizer_G,
    pix2pix_trainer.py:127-139) followed by `fuse_adam` on the new optimiser."""
    for name in ("optimizer_G", "optimizer_D"):
        optimizer = getattr(trainer, name, None)
        if optimizer is not None:
            fuse_adam(optimizer)
    if getattr(getattr(trainer, "opt", None), "use_ema", False):
        for name in ("netG_ema", "netCorr_ema"):
            old = getattr(trainer, name, None)
            if old is not None and not isinstance(old, EMA):
                new = EMA(old.mu, shadow=old.shadow)
                new.original = old.original
                setattr(trainer, name, new)
    inner = getattr(trainer, "update_fixed_params", None)
    if inner is not None and not getattr(inner, "cocos_fused", False):
        def update_fixed_params(*args, **kwargs):
            out = inner(*args, **kwargs)
            if getattr(trainer, "optimizer_G", None) is not None:
                fuse_adam(trainer.optimizer_G)
            return out

        update_fixed_params.cocos_fused = True
        trainer.update_fixed_params = update_fixed_params
    return trainer


def _ema_holders(module):
    """the modules that hold the reference's `EMA` by name: models.networks.generator, its package when that re-exports the
    class, and, once imported, trainers.pix2pix_trainer (`from models.networks.generator import EMA`, pix2pix_trainer.py:10).
    `module`: the reference's models.networks.generator or its models.networks package."""
    name = module.__name__
    generator = module if name.endswith(".generator") else importlib.import_module(name + ".generator")
    holders = [generator]
    for other in (sys.modules.get(generator.__name__.rsplit(".", 1)[0]), sys.modules.get("trainers.pix2pix_trainer")):
        if other is not None and hasattr(other, "EMA"):
            holders.append(other)
    return holders


def install_optim_into_reference(generator_module):
    """`models.networks.generator.EMA` (and the copies of that name in models.networks and, when already imported, in
    trainers.pix2pix_trainer) -> this module's `EMA`, so a `Pix2PixTrainer` built afterwards owns fused EMAs.
    Returns what it replaced, for `restore_reference_optim`."""
    replaced = {}
    for holder in _ema_holders(generator_module):
        replaced[holder.__name__] = holder.EMA
        holder.EMA = EMA
    return replaced


def restore_reference_optim(generator_module, replaced):
    """Undo `install_optim_into_reference` with the dictionary it returned."""
    for holder in _ema_holders(generator_module):
        if holder.__name__ in replaced:
            holder.EMA = replaced[holder.__name__]
