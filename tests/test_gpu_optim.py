"""K29 on the GPU: the multi-tensor Adam step (`cocosnet_amd.optim.fuse_adam`) and EMA update (`optim.EMA`).

Adam is judged against an arbiter that is not the code under test — torch.optim.Adam on fp64 copies fed the same fp32 gradients —
next to the framework's own fp32 step: err(fused) <= 2 * err(framework) + one fp32 ulp of max|x| for the parameters and both
moments.  Gradients are pre-generated from a seed and never depend on the parameters, so the arms cannot drift apart chaotically:
a difference is rounding or a bug.  EMA is bitwise the reference's expression in torch ops.  Every figure is printed before it
is asserted (tools/gpu_tests.sh keeps the log)."""
import bisect
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POOL_BELOW = 4096           # tensors smaller than this are pooled per case before the maximum is taken
SIZES = [1, 3, 4, 5, 1023, 4096, 407 * 407 * 9, 2 ** 25 + 1]

CASES = {
    # Pix2PixModel.create_optimizers, TTUR: betas (0, 0.9), eps 1e-3, two groups
    "generator": dict(adam=dict(lr=1e-4, betas=(0.0, 0.9), eps=1e-3), group_lr=(2e-4, 5e-5)),
    "discriminator": dict(adam=dict(lr=4e-4, betas=(0.0, 0.9)), group_lr=(None,)),
    "no_TTUR": dict(adam=dict(lr=2e-4, betas=(0.5, 0.999)), group_lr=(None,)),
    "weight_decay": dict(adam=dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-4), group_lr=(None, 1e-3)),
}


@pytest.fixture(autouse=True)
def _adam_route_on(monkeypatch):
    """the kernel route of fuse_adam ships switched off (optim.ADAM_FUSED); every test here exercises it"""
    from cocosnet_amd import optim
    monkeypatch.setattr(optim, "ADAM_FUSED", True)


def _ulp(x: float) -> float:
    """one fp32 ulp of |x| (the form of tests/test_gpu_losses.py)"""
    return float(np.spacing(np.float32(abs(float(x)))))


def _make_optimizer(tensors, case, dtype=torch.float32):
    """parameters (clones of `tensors` in dtype) dealt round-robin over the case's groups + torch.optim.Adam over them"""
    params = [torch.nn.Parameter(t.detach().to(dtype).clone()) for t in tensors]
    lrs = case["group_lr"]
    groups = []
    for k, lr in enumerate(lrs):
        g = {"params": params[k::len(lrs)]}
        if lr is not None:
            g["lr"] = lr
        groups.append(g)
    return params, torch.optim.Adam(groups, **case["adam"])


def _set_grads(params, grads, unaligned=False):
    """p.grad = the pre-generated gradient (cast to p's dtype); `unaligned`: fp32 gradients become views one element into a
    flat buffer: 4-byte, not 16-byte aligned"""
    keep = []
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif unaligned and p.dtype == torch.float32:
            flat = torch.empty(g.numel() + 1, device=g.device, dtype=torch.float32)
            flat[1:].copy_(g.reshape(-1))
            p.grad = flat[1:].view_as(p)
            assert p.grad.data_ptr() % 16 == 4, p.grad.data_ptr()
            keep.append(flat)
        else:
            p.grad = g.to(p.dtype).clone()
    return keep


def _gradients(tensors, steps, seed, special=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for s in range(steps):
        row = []
        for t in tensors:
            x = torch.randn(t.shape, device=DEV, generator=g) * 0.05
            if special and t.numel() >= 5:
                flat = x.view(-1)
                flat[0::7] = 0.0                       # exact zeros
                flat[1::11] = 1e15 if s % 2 == 0 else -1e15      # g * g = 1e30: a normal fp32 number
                flat[2::13] = 1e-15                    # g * g = 1e-30: normal as well
            row.append(x)
        out.append(row)
    return out


def _judge(what, fused, framework, arbiter):
    """the inequality over lists of (name, fused, framework, fp64) tensors; small tensors pooled"""
    pooled = {}
    rows = []
    for (name, a), (_, b), (_, w) in zip(fused, framework, arbiter):
        a64, b64 = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
        w64 = w.detach().reshape(-1)
        # where the framework's arm is inf / NaN the fused arm must be the same class in the same elements
        assert torch.equal(torch.isnan(a64), torch.isnan(b64)), (what, name, "NaN pattern")
        assert torch.equal(torch.isinf(a64), torch.isinf(b64)) and torch.equal(a64[torch.isinf(a64)], b64[torch.isinf(b64)]), (what, name, "inf")
        ok = torch.isfinite(b64) & torch.isfinite(w64)
        if not bool(ok.any()):
            continue
        ef = float((a64 - w64)[ok].abs().max())
        ew = float((b64 - w64)[ok].abs().max())
        mx = float(w64[ok].abs().max())
        if a.numel() < POOL_BELOW:
            p = pooled.setdefault(name.split("/")[0], [0.0, 0.0, 0.0])
            p[0], p[1], p[2] = max(p[0], ef), max(p[1], ew), max(p[2], mx)
        else:
            rows.append((name, ef, ew, mx))
    rows += [(k + "/pooled<%d" % POOL_BELOW, *v) for k, v in pooled.items()]
    worst = None
    for name, ef, ew, mx in rows:
        if worst is None or ef - 2 * ew > worst[1] - 2 * worst[2]:
            worst = (name, ef, ew, mx)
    for name, ef, ew, mx in rows if len(rows) <= 24 else [worst]:
        print(f"{what} {name}: err fused {ef:.3g} framework {ew:.3g} bound {2 * ew + _ulp(mx):.3g} (max|x| {mx:.3g})")
    for name, ef, ew, mx in rows:
        assert ef <= 2 * ew + _ulp(mx), (what, name, ef, ew, mx)


def _state_lists(params, optimizer, prefix):
    p = [(f"{prefix}p/{i}", q) for i, q in enumerate(params)]
    has = [(i, q) for i, q in enumerate(params) if "exp_avg" in optimizer.state.get(q, {})]
    m = [(f"{prefix}m/{i}", optimizer.state[q]["exp_avg"]) for i, q in has]
    v = [(f"{prefix}v/{i}", optimizer.state[q]["exp_avg_sq"]) for i, q in has]
    return p, m, v


def _three_arms(tensors, case, grads, unaligned=False, check_at=None, what=""):
    from cocosnet_amd import optim
    pf, of = _make_optimizer(tensors, case)
    optim.fuse_adam(of)
    pw, ow = _make_optimizer(tensors, case)
    pa, oa = _make_optimizer(tensors, case, torch.float64)
    check_at = check_at or [len(grads)]
    for s, row in enumerate(grads, 1):
        keep = _set_grads(pf, row, unaligned)
        _set_grads(pw, row)
        _set_grads(pa, row)
        of.step(); ow.step(); oa.step()
        del keep
        if s in check_at:
            for lf, lw, la in zip(_state_lists(pf, of, ""), _state_lists(pw, ow, ""), _state_lists(pa, oa, "")):
                _judge(f"{what} step {s}", lf, lw, la)
    assert of.cocos_last_launches >= 1, "the fused route did not run"
    return (pf, of), (pw, ow), (pa, oa)


# ---- 1. Adam against fp64 and against the framework ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("flavour", ["plain", "unaligned_grad", "special_values"])
def test_adam_against_fp64_and_the_framework(case, flavour, hip_lib):
    g = torch.Generator(device=DEV).manual_seed(29)
    tensors = [torch.randn(n, device=DEV, generator=g) * 0.1 for n in SIZES]
    long = flavour in ("plain", "unaligned_grad")      # 50 steps and the 2^25 + 1 tensor (three table entries), also with the 4-byte-aligned gradient
    steps = 50 if long else 2
    sizes = tensors if long else tensors[:-1]
    if long:
        grads = _gradients(sizes[:-1], steps, 7)
        # 50 steps of the largest tensor: one gradient, reused (the arms still see identical inputs)
        big = torch.randn(sizes[-1].shape, device=DEV, generator=g) * 0.05
        grads = [row + [big] for row in grads]
    else:
        grads = _gradients(sizes, steps, 7, special=flavour == "special_values")
    _three_arms(sizes, CASES[case], grads, unaligned=flavour == "unaligned_grad", check_at=[1, 2, steps], what=f"{case}/{flavour}")


# ---- 2. / 5. / 7. the real parameter lists ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_lists():
    from cocosnet_amd import correspondence as cc, translation as tl
    torch.manual_seed(0)
    corr = cc.NoVGGCorrespondence(cc.ade20k_options(isTrain=True)).to(DEV)
    opt = tl.celebahq_edge_train_options()
    netG = tl.SPADEGenerator(opt).to(DEV)
    netD = tl.MultiscaleDiscriminator(opt).to(DEV)
    G = [p.detach() for p in netG.parameters()] + [p.detach() for p in corr.parameters()]
    D = [p.detach() for p in netD.parameters()]
    return {"G": (G, len(list(netG.parameters()))), "D": (D, len(D))}


def _real_optimizer(tensors, n_first, which, dtype=torch.float32):
    """as Pix2PixModel.create_optimizers builds them (opt.lr = 2e-4, TTUR)"""
    params = [torch.nn.Parameter(t.to(dtype).clone()) for t in tensors]
    if which == "G":
        groups = [{"params": params[:n_first], "lr": 2e-4 * 0.5}, {"params": params[n_first:], "lr": 2e-4 * 0.5}]
        return params, torch.optim.Adam(groups, lr=1e-4, betas=(0.0, 0.9), eps=1e-3)
    return params, torch.optim.Adam(params, lr=4e-4, betas=(0.0, 0.9))


def _expected_launches(numels, rows=None):
    """the launch count from the header's constants alone: a tensor takes ceil(n / ENTRY_ELEMS) table entries; a launch is full
    at TABLE_ENTRIES entries or when an entry would name a (TABLE_GROUPS + 1)-th different row (`rows[i]`: the row of tensor i)"""
    c = _header_constants()
    launches, used, seen = 0, 0, set()
    for i, n in enumerate(numels):
        row = 0 if rows is None else rows[i]
        for _ in range(-(-n // c["ENTRY_ELEMS"])):
            if used == c["TABLE_ENTRIES"] or (row not in seen and len(seen) == c["TABLE_GROUPS"]):
                launches, used, seen = launches + 1, 0, set()
            used += 1
            seen.add(row)
    return launches + (1 if used else 0)


def _header_constants():
    from cocosnet_amd import _lib
    return {n: _lib.CONSTANTS["COCOS_OPTIM_" + n] for n in ("TABLE_ENTRIES", "TABLE_GROUPS", "CHUNK_ELEMS", "ENTRY_ELEMS")}


@pytest.mark.parametrize("which", ["G", "D"])
def test_real_parameter_lists(which, real_lists, hip_lib, monkeypatch):
    from cocosnet_amd import _lib, ops, optim
    assert _header_constants() == ops.optim_constants()            # the library was built with the header's values
    tensors, n_first = real_lists[which]
    grads = _gradients(tensors, 3, 101)
    pf, of = _real_optimizer(tensors, n_first, which)
    optim.fuse_adam(of)
    pw, ow = _real_optimizer(tensors, n_first, which)
    pa, oa = _real_optimizer(tensors, n_first, which, torch.float64)
    guard = _TableGuard(monkeypatch)
    for s, row in enumerate(grads, 1):
        _set_grads(pf, row); _set_grads(pw, row); _set_grads(pa, row)
        of.step(); ow.step(); oa.step()
        for lf, lw, la in zip(_state_lists(pf, of, ""), _state_lists(pw, ow, ""), _state_lists(pa, oa, "")):
            _judge(f"real {which} step {s}", lf, lw, la)
    numels = [p.numel() for p in pf]
    # (two groups with one step count each: two rows, far from the row limit) — the count is what the library launched
    want = _expected_launches(numels, [0 if i < n_first else 1 for i in range(len(numels))])
    print(f"real {which}: {sum(numels)} parameters in {len(numels)} tensors, {of.cocos_last_launches} launches per step (expected {want})")
    assert of.cocos_last_launches == want
    guard.check(3, 4 * 3 * len(numels))
    # 5. determinism: the same three steps from the same state, bitwise
    pf2, of2 = _real_optimizer(tensors, n_first, which)
    optim.fuse_adam(of2)
    for row in grads:
        _set_grads(pf2, row)
        of2.step()
    for a, b in zip(pf, pf2):
        assert torch.equal(a, b)
        assert torch.equal(of.state[a]["exp_avg_sq"], of2.state[b]["exp_avg_sq"]) and torch.equal(of.state[a]["exp_avg"], of2.state[b]["exp_avg"])


def test_more_group_rows_than_one_launch_holds(hip_lib):
    """eleven groups of one small tensor: the ninth different row ends the first launch, so two launches — counted by the library"""
    from cocosnet_amd import optim
    g = torch.Generator(device=DEV).manual_seed(41)
    tensors = [torch.randn(n, device=DEV, generator=g) * 0.1 for n in (5, 4096, 1023, 7, 64, 4097, 3, 129, 1, 8192, 33)]
    case = dict(adam=dict(lr=1e-4, betas=(0.5, 0.999)), group_lr=tuple(1e-4 * (k + 1) for k in range(len(tensors))))
    grads = _gradients(tensors, 3, 43)
    (pf, of), _, _ = _three_arms(tensors, case, grads, check_at=[1, 2, 3], what="eleven groups")
    want = _expected_launches([t.numel() for t in tensors], list(range(len(tensors))))
    assert want == 2 and of.cocos_last_launches == want, (of.cocos_last_launches, want)
    # 65 tensors of one group: the 65th entry starts a second launch
    many = [torch.randn(17, device=DEV, generator=g) for _ in range(_header_constants()["TABLE_ENTRIES"] + 1)]
    (pf, of), _, _ = _three_arms(many, CASES["discriminator"], _gradients(many, 1, 44), what="65 tensors")
    assert of.cocos_last_launches == _expected_launches([17] * len(many)) == 2


def _offset_view(t):
    """a copy of t that starts one element into a flat buffer: 4-byte, not 16-byte aligned"""
    flat = torch.zeros(t.numel() + 1, device=t.device, dtype=t.dtype)
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("case", ["generator", "weight_decay"])
def test_dword_route_of_unaligned_parameters_and_moments(case, hip_lib):
    """p, exp_avg, exp_avg_sq (and the gradient) all 4-byte aligned only: the kernel's all-dword route"""
    from cocosnet_amd import optim
    g = torch.Generator(device=DEV).manual_seed(47)
    tensors = [torch.randn(n, device=DEV, generator=g) * 0.1 for n in (1, 3, 5, 1023, 1024, 4096, 3 * 4097, 2 ** 20 + 3)]
    grads = _gradients(tensors, 5, 48)
    pf, of = _make_optimizer(tensors, CASES[case])
    for p in pf:
        p.data = _offset_view(p.data)
        of.state[p] = {"step": torch.tensor(0.0), "exp_avg": _offset_view(torch.zeros_like(p.data)),
                       "exp_avg_sq": _offset_view(torch.zeros_like(p.data))}
    optim.fuse_adam(of)
    pw, ow = _make_optimizer(tensors, CASES[case])
    pa, oa = _make_optimizer(tensors, CASES[case], torch.float64)
    for s, row in enumerate(grads, 1):
        keep = _set_grads(pf, row, unaligned=True)
        _set_grads(pw, row); _set_grads(pa, row)
        for p in pf:
            assert all(t.data_ptr() % 16 == 4 for t in (p, p.grad, of.state[p]["exp_avg"], of.state[p]["exp_avg_sq"]))
        of.step(); ow.step(); oa.step()
        del keep
        for lf, lw, la in zip(_state_lists(pf, of, ""), _state_lists(pw, ow, ""), _state_lists(pa, oa, "")):
            _judge(f"dword route {case} step {s}", lf, lw, la)
    assert of.cocos_last_launches == 1


@pytest.mark.parametrize("unaligned", ["shadow", "parameter", "both"])
def test_ema_dword_route(unaligned, hip_lib):
    from cocosnet_amd import optim
    g = torch.Generator(device=DEV).manual_seed(53)
    tensors = [torch.randn(n, device=DEV, generator=g) for n in (1, 3, 5, 1023, 4096, 3 * 4097, 2 ** 20 + 3)]
    model = _Holder(tensors)
    if unaligned in ("parameter", "both"):
        for p in model.parameters():
            p.data = _offset_view(p.data)
    ema = optim.EMA(0.999)
    for name, p in model.named_parameters():
        ema.register(name, p.data)
        if unaligned in ("shadow", "both"):
            ema.shadow[name] = _offset_view(ema.shadow[name])
    want = {k: v.clone() for k, v in ema.shadow.items()}
    for it in range(2):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, device=DEV, generator=g) * 0.01)
        ema(model)
        assert ema.cocos_last_launches == 1
        for name, p in model.named_parameters():
            want[name] = ((1.0 - 0.999) * p.data + 0.999 * want[name]).clone()
            assert torch.equal(ema.shadow[name], want[name]), (name, it)


# ---- 7. live buffers -------------------------------------------------------------------------------------------------------------
def _live_blocks():
    blocks = []
    for seg in torch.cuda.memory_snapshot():
        addr = seg["address"]
        for b in seg["blocks"]:
            blocks.append((addr, b["size"], b["state"] == "active_allocated"))
            addr += b["size"]
    blocks.sort()
    return blocks


class _TableGuard:
    """`_lib.call` wrapped (the pattern of test_gpu_live_buffers.py): the two multi-tensor entry points take their device pointers
    in HOST tables, so the guard decodes the tables (cocos_adam_entry: words 0-3 of 6, cocos_ema_entry: words 0-1 of 3) and checks
    every pointer against the allocator's ACTIVE blocks at call time."""
    LAYOUT = {"cocos_adam_multi_step": (6, 4), "cocos_ema_multi_update": (3, 2)}

    def __init__(self, monkeypatch):
        from cocosnet_amd import _lib
        self.calls, self.pointers, self.dead = 0, 0, []
        real_call = _lib.call

        def checked_call(name, *args):
            if name in self.LAYOUT:
                words, nptr = self.LAYOUT[name]
                table = (ctypes.c_uint64 * (words * args[1])).from_address(args[0])
                blocks = _live_blocks()
                starts = [b[0] for b in blocks]
                for e in range(args[1]):
                    for k in range(nptr):
                        a = table[e * words + k]
                        j = bisect.bisect_right(starts, a) - 1
                        inside = j >= 0 and a < blocks[j][0] + blocks[j][1]
                        self.pointers += 1
                        if not inside or not blocks[j][2]:
                            self.dead.append((name, e, k, hex(a)))
                self.calls += 1
            return real_call(name, *args)

        monkeypatch.setattr(_lib, "call", checked_call)

    def check(self, min_calls, min_pointers):
        torch.cuda.synchronize()
        assert self.calls >= min_calls and self.pointers >= min_pointers, (self.calls, self.pointers)
        assert not self.dead, f"pointers outside live allocator blocks (entry point, entry, field, address): {self.dead[:8]}"


# ---- 3. semantics ----------------------------------------------------------------------------------------------------------------
def _small_tensors(seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(s, device=DEV, generator=g) * 0.1 for s in ((64, 33, 3, 3), (64,), (5,), (4096, 17), (1,))]


def test_parameters_without_a_gradient_and_a_changed_learning_rate(hip_lib):
    from cocosnet_amd import optim
    tensors = _small_tensors()
    case = CASES["generator"]
    grads = _gradients(tensors, 3, 11)
    for row in grads[:2]:
        row[2] = None                                    # parameter 2 joins at step 3 only: its step count differs inside its group
    pf, of = _make_optimizer(tensors, case)
    optim.fuse_adam(of)
    pw, ow = _make_optimizer(tensors, case)
    pa, oa = _make_optimizer(tensors, case, torch.float64)
    for s, row in enumerate(grads, 1):
        if s == 2:
            for o in (of, ow, oa):
                for grp in o.param_groups:
                    grp["lr"] = grp["lr"] * 10.0         # update_learning_rate rewrites param_group['lr']
        _set_grads(pf, row); _set_grads(pw, row); _set_grads(pa, row)
        of.step(); ow.step(); oa.step()
        if s < 3:
            assert torch.equal(pf[2], tensors[2]) and len(of.state[pf[2]]) == 0
        for lf, lw, la in zip(_state_lists(pf, of, ""), _state_lists(pw, ow, ""), _state_lists(pa, oa, "")):
            _judge(f"semantics step {s}", lf, lw, la)
    assert [float(of.state[p]["step"]) for p in pf] == [3.0, 3.0, 1.0, 3.0, 3.0]
    assert [float(ow.state[p]["step"]) for p in pw] == [3.0, 3.0, 1.0, 3.0, 3.0]
    # the larger learning rate took effect: a step-2 update ten times step 1's would be missed by a cached lr
    assert float((pf[0].detach() - tensors[0]).abs().max()) > 5 * 2e-4


def test_checkpoint_continuation_and_the_switch(hip_lib, monkeypatch):
    from cocosnet_amd import optim
    tensors = _small_tensors(5)
    case = CASES["no_TTUR"]
    grads = _gradients(tensors, 10, 13)

    def run(params, o, rows):
        for row in rows:
            _set_grads(params, row)
            o.step()

    p10, o10 = _make_optimizer(tensors, case)
    optim.fuse_adam(o10)
    run(p10, o10, grads)
    p5, o5 = _make_optimizer(tensors, case)
    optim.fuse_adam(o5)
    run(p5, o5, grads[:5])
    saved = copy.deepcopy(o5.state_dict())
    for k, st in saved["state"].items():
        assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and float(st["step"]) == 5.0
    now = [p.detach().clone() for p in p5]
    # fused -> fused: bitwise
    pff, off = _make_optimizer(now, case)
    optim.fuse_adam(off)
    off.load_state_dict(copy.deepcopy(saved))
    run(pff, off, grads[5:])
    for a, b in zip(pff, p10):
        assert torch.equal(a, b)
    # fused -> framework: the inequality, against fp64 continued from the same checkpoint
    pfw, ofw = _make_optimizer(now, case)
    ofw.load_state_dict(copy.deepcopy(saved))
    run(pfw, ofw, grads[5:])
    pa, oa = _make_optimizer(now, case, torch.float64)
    oa.load_state_dict(copy.deepcopy(saved))
    run(pa, oa, grads[5:])
    for lf, lw, la in zip(_state_lists(p10, o10, ""), _state_lists(pfw, ofw, ""), _state_lists(pa, oa, "")):
        _judge("continuation", lf, lw, la)
    # optim.FUSED = False: the framework's result, bitwise
    monkeypatch.setattr(optim, "FUSED", False)
    ps, os_ = _make_optimizer(tensors, case)
    optim.fuse_adam(os_)
    pw, ow = _make_optimizer(tensors, case)
    run(ps, os_, grads[:3]); run(pw, ow, grads[:3])
    for a, b in zip(ps, pw):
        assert torch.equal(a, b)


def test_step_hooks_send_the_step_to_the_framework(hip_lib):
    """register_step_pre_hook / _post_hook run inside the framework's step: with one registered the fused optimiser takes it"""
    from cocosnet_amd import optim
    tensors = _small_tensors(6)
    grads = _gradients(tensors, 2, 15)
    pf, of = _make_optimizer(tensors, CASES["no_TTUR"])
    optim.fuse_adam(of)
    pw, ow = _make_optimizer(tensors, CASES["no_TTUR"])
    seen = []
    handle = of.register_step_post_hook(lambda *a: seen.append(1))
    _set_grads(pf, grads[0]); _set_grads(pw, grads[0])
    of.step(); ow.step()
    assert seen == [1] and not hasattr(of, "cocos_last_launches")
    for a, b in zip(pf, pw):
        assert torch.equal(a, b)
    handle.remove()
    _set_grads(pf, grads[1])
    of.step()
    assert seen == [1] and of.cocos_last_launches == 1


def test_parameters_reallocated_by_a_host_round_trip(hip_lib):
    """util.save_network: net.cpu(); torch.save; net.cuda() — the parameters are new tensors afterwards"""
    from cocosnet_amd import optim
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).to(DEV)
    o = optim.fuse_adam(torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.0, 0.9)))
    x = torch.randn(8, 40, device=DEV)
    net(x).square().mean().backward()
    o.step()
    before_ptr = [p.data_ptr() for p in net.parameters()]
    net.cpu(); net.cuda()
    o.zero_grad()
    net(x).square().mean().backward()
    before = [p.detach().clone() for p in net.parameters()]
    o.step()
    assert o.cocos_last_launches == 1
    torch.cuda.synchronize()
    for p, b in zip(net.parameters(), before):
        assert not torch.equal(p, b), "the new parameter tensor was not updated"
    print("data_ptr changed by the round trip:", [a != p.data_ptr() for a, p in zip(before_ptr, net.parameters())])


# ---- 4. EMA ----------------------------------------------------------------------------------------------------------------------
class _Holder(torch.nn.Module):
    def __init__(self, tensors, frozen=()):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])
        for i in frozen:
            self.ps[i].requires_grad_(False)


@pytest.mark.parametrize("mu", [0.999, 0.5, 0.0])
@pytest.mark.parametrize("which", ["odd_sizes", "real_G"])
def test_ema_is_bitwise_the_reference_expression(mu, which, real_lists, hip_lib, monkeypatch):
    from cocosnet_amd import optim
    g = torch.Generator(device=DEV).manual_seed(17)
    tensors = [torch.randn(n, device=DEV, generator=g) for n in SIZES] if which == "odd_sizes" else real_lists["G"][0]
    model = _Holder(tensors, frozen=(1,))
    ema = optim.EMA(mu)
    for name, p in model.named_parameters():
        if p.requires_grad:
            ema.register(name, p.data)
    assert "ps.1" not in ema.shadow
    want = {k: v.clone() for k, v in ema.shadow.items()}
    ptrs = {k: v.data_ptr() for k, v in ema.shadow.items()}
    guard = _TableGuard(monkeypatch)
    for it in range(3):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, device=DEV, generator=g) * 0.01)
        ema(model)
        for name, p in model.named_parameters():
            if p.requires_grad:
                want[name] = ((1.0 - mu) * p.data + mu * want[name]).clone()       # the reference's expression, torch ops
        for k in want:
            assert torch.equal(ema.shadow[k], want[k]), (k, it)
            assert ema.shadow[k].data_ptr() == ptrs[k], "the shadow was not updated in place"
    guard.check(3, 2 * 3 * len(want))
    assert ema.cocos_last_launches == _expected_launches([want[k].numel() for k in want])
    before = [p.detach().clone() for p in model.parameters()]
    ema.assign(model)
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.data_ptr() == ema.shadow[name].data_ptr()
    ema.resume(model)
    for p, b in zip(model.parameters(), before):
        assert torch.equal(p, b)


# ---- 6. no host synchronisation, no allocation -----------------------------------------------------------------------------------
def test_no_host_synchronisation_and_no_allocation(hip_lib, monkeypatch):
    from cocosnet_amd import optim
    tensors = _small_tensors(9) + [torch.randn(2 ** 20 + 3, device=DEV)]
    case = CASES["generator"]
    params, o = _make_optimizer(tensors, case)
    optim.fuse_adam(o)
    model = _Holder(tensors)
    ema = optim.EMA(0.999)
    for name, p in model.named_parameters():
        ema.register(name, p.data)
    grads = _gradients(tensors, 1, 21)[0]
    _set_grads(params, grads)
    o.step(); ema(model)                                   # warm-up: state creation, library load
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    mem0, n0 = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            for _ in range(3):
                o.step(); ema(model)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        print("sync debug mode is not honoured on this build: counting the host-reading calls on device tensors instead")
        counts = {}

        def counting(real, name):
            def f(self, *a, **k):
                if torch.is_tensor(self) and self.is_cuda:
                    counts[name] = counts.get(name, 0) + 1
                return real(self, *a, **k)
            return f
        for attr in ("item", "tolist", "cpu", "__bool__", "__float__"):
            monkeypatch.setattr(torch.Tensor, attr, counting(getattr(torch.Tensor, attr), attr))
        for _ in range(3):
            o.step(); ema(model)
        assert not counts, counts
    else:
        print("sync debug mode 'error' is honoured: three fused steps and EMA updates ran under it")
    assert o.cocos_last_launches == 1
    assert torch.cuda.memory_allocated() == mem0, (torch.cuda.memory_allocated(), mem0)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == n0, "a fused step allocated device memory"


# ---- 8. trainer level ------------------------------------------------------------------------------------------------------------
class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(8)
        mk = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 16, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv2d(16, 3, 3, padding=1))
        self.net = torch.nn.ModuleDict({"netG": mk(), "netCorr": mk(), "netD": mk()})

    def create_optimizers(self, opt):
        G = [{"params": self.net["netG"].parameters(), "lr": opt.lr * 0.5}, {"params": self.net["netCorr"].parameters(), "lr": opt.lr * 0.5}]
        return (torch.optim.Adam(G, lr=opt.lr / 2, betas=(0.0, 0.9), eps=1e-3),
                torch.optim.Adam(list(self.net["netD"].parameters()), lr=opt.lr * 2, betas=(0.0, 0.9)))


class _StandInTrainer:
    """the attribute names of the reference's Pix2PixTrainer (trainers/pix2pix_trainer.py); `ema_cls`: its EMA"""

    def __init__(self, opt, ema_cls=None, dtype=torch.float32):
        self.opt = opt
        self.pix2pix_model_on_one_gpu = self.pix2pix_model = _Model().to(DEV, dtype)
        net = self.pix2pix_model_on_one_gpu.net
        if opt.use_ema:
            self.netG_ema, self.netCorr_ema = ema_cls(opt.ema_beta), ema_cls(opt.ema_beta)
            for ema, key in ((self.netG_ema, "netG"), (self.netCorr_ema, "netCorr")):
                for name, p in net[key].named_parameters():
                    if p.requires_grad:
                        ema.register(name, p.data)
        self.optimizer_G, self.optimizer_D = self.pix2pix_model_on_one_gpu.create_optimizers(opt)

    def run_generator_one_step(self, x):
        net = self.pix2pix_model_on_one_gpu.net
        self.optimizer_G.zero_grad()
        self.out = net["netG"](net["netCorr"](x))
        (net["netD"](self.out).mean() + self.out.square().mean()).backward()
        self.optimizer_G.step()
        if self.opt.use_ema:
            self.netG_ema(net["netG"])
            self.netCorr_ema(net["netCorr"])

    def run_discriminator_one_step(self, x):
        net = self.pix2pix_model_on_one_gpu.net
        self.optimizer_D.zero_grad()
        (net["netD"](self.out.detach()).mean() - net["netD"](x).mean()).square().backward()
        self.optimizer_D.step()

    def update_fixed_params(self):
        net = self.pix2pix_model_on_one_gpu.net
        G = [{"params": net["netG"].parameters(), "lr": self.opt.lr * 0.5}, {"params": net["netCorr"].parameters(), "lr": self.opt.lr * 0.5}]
        self.optimizer_G = torch.optim.Adam(G, lr=self.opt.lr / 2, betas=(0.0, 0.9), eps=1e-3)


class _RefEMA:
    """the reference's expression, torch ops (the GPU box has no copy of the reference)"""

    def __init__(self, mu):
        self.mu, self.shadow, self.original = mu, {}, {}

    def register(self, name, val):
        self.shadow[name] = val.clone()

    def __call__(self, model):
        for name, p in model.named_parameters():
            if p.requires_grad:
                self.shadow[name] = ((1.0 - self.mu) * p.data + self.mu * self.shadow[name]).clone()


@pytest.mark.parametrize("distributed", [False, True])
def test_trainer_level(distributed, hip_lib):
    from cocosnet_amd import optim, trainer as tr
    opt = SimpleNamespace(use_ema=True, ema_beta=0.999, lr=2e-4, gpu_ids=[0])
    cls = tr.make_distributed_trainer(_StandInTrainer) if distributed else _StandInTrainer
    fused = optim.fuse_trainer(cls(opt, ema_cls=_RefEMA))
    plain = _StandInTrainer(opt, ema_cls=_RefEMA)
    arbiter = _StandInTrainer(opt, ema_cls=_RefEMA, dtype=torch.float64)      # the same trainer in fp64
    assert isinstance(fused.netG_ema, optim.EMA) and isinstance(fused.netCorr_ema, optim.EMA)
    g = torch.Generator(device=DEV).manual_seed(2)
    for _ in range(2):
        x = torch.randn(2, 3, 16, 16, device=DEV, generator=g)
        for t in (fused, plain, arbiter):
            xt = x.double() if t is arbiter else x
            t.run_generator_one_step(xt)
            t.run_discriminator_one_step(xt)
    assert fused.optimizer_G.cocos_last_launches == 1 and fused.optimizer_D.cocos_last_launches == 1
    nets = lambda t: t.pix2pix_model_on_one_gpu.net
    for key in ("netG", "netCorr", "netD"):
        lists = [[(f"{key}/{i}", p) for i, p in enumerate(nets(t)[key].parameters())] for t in (fused, plain, arbiter)]
        _judge(f"trainer distributed={distributed}", *lists)
    for name in ("netG_ema", "netCorr_ema"):
        lists = [[(f"{name}/{k}", getattr(t, name).shadow[k]) for k in sorted(plain.netG_ema.shadow)] for t in (fused, plain, arbiter)]
        _judge(f"trainer distributed={distributed}", *lists)
    fused.update_fixed_params()
    assert getattr(fused.optimizer_G, "cocos_fused", False), "update_fixed_params left an unfused optimizer_G"
    x = torch.randn(2, 3, 16, 16, device=DEV, generator=g)
    fused.run_generator_one_step(x)
    assert fused.optimizer_G.cocos_last_launches == 1
