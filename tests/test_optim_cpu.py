"""K29 without a GPU: the new translation unit builds for gfx950 with no scratch, header / library / binding agree on its symbols,
the entry points reject bad arguments before any HIP call, and the host side of `cocosnet_amd.optim` (fall-backs, state layout,
the EMA class, the composition with the gradient exchange on gloo) behaves as the framework / the reference does."""
import copy
import ctypes
import os
import re
import socket
import subprocess

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.ref_harness import load_reference, reference_available

needs_ref = pytest.mark.skipif(not reference_available(), reason="the reference checkout is not on this machine")
NEW_SYMBOLS = ("cocos_optim_constant", "cocos_adam_multi_step", "cocos_ema_multi_update")


# ---- 1. build, symbols, scratch ---------------------------------------------------------------------------------------------------
def test_translation_unit_is_built_and_symbols_agree(hip_lib):
    from cocosnet_amd import _lib, build
    assert "optim_step.hip" in build.HIP_SOURCES
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES and name in _lib.EXPORTED_SYMBOLS and hasattr(hip_lib, name), name
    from cocosnet_amd import ops
    for macro, value in ops.optim_constants().items():           # the library's own values against the header's macros
        assert _lib.CONSTANTS["COCOS_OPTIM_" + macro] == value, macro


def test_kernels_use_no_scratch(tmp_path):
    from cocosnet_amd import build
    src = os.path.join(build.CSRC_DIR, "optim_step.hip")
    cmd = [build._hipcc(), *build._flags(), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "optim_step.o")]
    out = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    found = {}
    name = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
    kernels = {k: v for k, v in found.items() if "adam_multi_kernel" in k or "ema_multi_kernel" in k}
    assert len(kernels) == 2, found
    assert all(v == 0 for v in kernels.values()), kernels
    assert "-ffast-math" not in cmd and b"gfx950" in open(tmp_path / "optim_step.o", "rb").read()


# ---- 2. argument checks ----------------------------------------------------------------------------------------------------------
def _adam_entry(p=16, g=32, m=48, v=64, n=4, group=0):
    return (ctypes.c_uint64 * 6)(p, g, m, v, n & 0xffffffffffffffff, group & 0xffffffff)


def _row(step_size=1e-3, bc2_sqrt=0.3, beta1=0.0, beta2=0.9, eps=1e-3, wd=0.0):
    return (ctypes.c_float * 8)(step_size, bc2_sqrt, beta1, 1 - beta1, beta2, 1 - beta2, eps, wd)


def test_argument_validation_needs_no_gpu(hip_lib):
    adam, ema, err = hip_lib.cocos_adam_multi_step, hip_lib.cocos_ema_multi_update, hip_lib.cocos_last_error_string
    A = ctypes.addressof
    e, r = _adam_entry(), _row()
    assert adam(None, 1, A(r), 1, None, None) == -1 and b"null" in err()
    assert adam(A(e), 1, None, 1, None, None) == -1
    assert adam(A(e), 0, A(r), 1, None, None) == -1 and adam(A(e), -3, A(r), 1, None, None) == -1 and adam(A(e), 1, A(r), 0, None, None) == -1
    for bad in (_adam_entry(p=0), _adam_entry(g=0), _adam_entry(m=0), _adam_entry(v=0)):
        assert adam(A(bad), 1, A(r), 1, None, None) == -1 and b"null pointer" in err()
    assert adam(A(_adam_entry(n=0)), 1, A(r), 1, None, None) == -1 and adam(A(_adam_entry(n=-5)), 1, A(r), 1, None, None) == -1
    assert adam(A(_adam_entry(group=1)), 1, A(r), 1, None, None) == -1 and adam(A(_adam_entry(group=-1)), 1, A(r), 1, None, None) == -1
    assert adam(A(_adam_entry(m=16)), 1, A(r), 1, None, None) == -1 and b"aliased" in err()
    for bad in (_row(bc2_sqrt=0.0), _row(beta1=1.0), _row(beta2=-0.1), _row(eps=-1.0)):
        assert adam(A(e), 1, A(bad), 1, None, None) == -2
    s = (ctypes.c_uint64 * 3)(16, 32, 4)
    mu = ctypes.c_double(0.999)
    assert ema(None, 1, mu, None, None) == -1 and b"null" in err()
    assert ema(A(s), 0, mu, None, None) == -1 and ema(A(s), -1, mu, None, None) == -1
    assert ema(A((ctypes.c_uint64 * 3)(0, 32, 4)), 1, mu, None, None) == -1
    assert ema(A((ctypes.c_uint64 * 3)(16, 16, 4)), 1, mu, None, None) == -1 and b"aliased" in err()
    assert ema(A((ctypes.c_uint64 * 3)(16, 32, 0)), 1, mu, None, None) == -1
    assert ema(A(s), 1, ctypes.c_double(float("nan")), None, None) == -1
    # a failed call reports no launch; the counter is optional
    count = ctypes.c_int(7)
    assert adam(A(e), 1, A(_row(eps=-1.0)), 1, A(count), None) == -2 and ema(None, 1, mu, A(count), None) == -1
    const = hip_lib.cocos_optim_constant
    assert [const(k) for k in range(4)] == [64, 8, 4096, 1 << 24] and const(4) == 0 and const(-1) == 0


def test_wrappers_fail_loudly_on_cpu_tensors(hip_lib):
    from cocosnet_amd import _lib, ops
    x = [torch.zeros(4) for _ in range(4)]
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.adam_multi_step(x[:1], x[1:2], x[2:3], x[3:], [(1e-3, 0.3, 0.0, 1.0, 0.9, 0.1, 1e-3, 0.0)], [0])
    with pytest.raises(_lib.CocosHipError, match="no CPU fallback"):
        ops.ema_multi_update(x[:1], x[1:2], 0.999)


# ---- 3. / 5. fuse_adam on the CPU: the framework ------------------------------------------------------------------------------------
def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(5, 7, 1), torch.nn.PReLU(), torch.nn.Conv2d(7, 3, 3, padding=1))


def _adam(net):
    groups = [{"params": net[0].parameters(), "lr": 1e-3}, {"params": list(net[1].parameters()) + list(net[2].parameters())}]
    return torch.optim.Adam(groups, lr=2e-3, betas=(0.0, 0.9), eps=1e-3)


def test_fuse_adam_on_a_cpu_optimiser_is_the_framework_bitwise():
    from cocosnet_amd import optim
    a, b = _net(), _net()
    oa, ob = optim.fuse_adam(_adam(a)), _adam(b)
    assert optim.fuse_adam(oa) is oa
    g = torch.Generator().manual_seed(3)
    for _ in range(20):
        grads = [torch.randn(p.shape, generator=g) for p in a.parameters()]
        for net in (a, b):
            for p, gr in zip(net.parameters(), grads):
                p.grad = gr.clone()
        oa.step(); ob.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.equal(p, q)
    loss = oa.step(lambda: torch.tensor(1.5))            # a closure goes to the framework too
    assert float(loss) == 1.5
    with pytest.raises(TypeError):
        optim.fuse_adam(torch.optim.SGD(a.parameters(), lr=0.1))
    wrapped = _adam(_net())
    inner = wrapped.step
    wrapped.step = lambda closure=None: inner()
    with pytest.raises(TypeError, match="already wrapped"):
        optim.fuse_adam(wrapped)


def test_state_dict_is_interchangeable_with_the_framework():
    from cocosnet_amd import optim
    a, b = _net(), _net()
    oa, ob = optim.fuse_adam(_adam(a)), _adam(b)
    for net, o in ((a, oa), (b, ob)):
        g = torch.Generator().manual_seed(5)
        for _ in range(3):
            for p in net.parameters():
                p.grad = torch.randn(p.shape, generator=g)
            o.step()
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in sa["state"][k]:
            x, y = sa["state"][k][name], sb["state"][k][name]
            assert (x.dtype, x.shape, x.device) == (y.dtype, y.shape, y.device) and torch.equal(x, y), (k, name)
    fresh_fw, fresh_fused = _adam(_net()), optim.fuse_adam(_adam(_net()))
    fresh_fw.load_state_dict(copy.deepcopy(sa))          # fused -> framework
    fresh_fused.load_state_dict(copy.deepcopy(sb))       # framework -> fused
    assert float(fresh_fw.state_dict()["state"][0]["step"]) == 3.0 and float(fresh_fused.state_dict()["state"][0]["step"]) == 3.0


# ---- 4. EMA against the reference's class --------------------------------------------------------------------------------------------
@needs_ref
def test_ema_equals_the_reference_class_on_the_cpu():
    from cocosnet_amd import optim
    ref_cls = load_reference().generator.EMA
    a, b = _net(), _net()
    for net in (a, b):
        net[1].weight.requires_grad_(False)
    mine, ref = optim.EMA(0.999), ref_cls(0.999)
    for net, ema in ((a, mine), (b, ref)):
        for name, p in net.named_parameters():
            if p.requires_grad:
                ema.register(name, p.data)
    assert mine.shadow.keys() == ref.shadow.keys() and "1.weight" not in mine.shadow
    g = torch.Generator().manual_seed(7)

    def same():
        assert mine.shadow.keys() == ref.shadow.keys() and mine.original.keys() == ref.original.keys()
        for k in ref.shadow:
            assert torch.equal(mine.shadow[k], ref.shadow[k]), k
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)

    for _ in range(5):
        with torch.no_grad():
            for p, q in zip(a.parameters(), b.parameters()):
                d = torch.randn(p.shape, generator=g) * 0.1
                p.add_(d); q.add_(d)
        mine(a); ref(b)
        same()
    mine.assign(a); ref.assign(b)
    same()
    for name, p in a.named_parameters():
        if p.requires_grad:
            assert p.data_ptr() == mine.shadow[name].data_ptr()
    mine.resume(a); ref.resume(b)
    same()


@needs_ref
def test_install_and_restore_put_the_class_where_the_trainer_imports_it_from():
    from cocosnet_amd import optim
    networks = load_reference()
    before = networks.generator.EMA
    replaced = optim.install_optim_into_reference(networks)
    try:
        assert networks.generator.EMA is optim.EMA and replaced[networks.generator.__name__] is before
    finally:
        optim.restore_reference_optim(networks, replaced)
    assert networks.generator.EMA is before


def test_fuse_trainer_on_a_cpu_stand_in():
    from types import SimpleNamespace
    from cocosnet_amd import optim

    class Old:
        def __init__(self, mu):
            self.mu, self.shadow, self.original = mu, {"w": torch.ones(2)}, {}

    net = _net()
    t = SimpleNamespace(opt=SimpleNamespace(use_ema=True), optimizer_G=_adam(net), optimizer_D=None, netG_ema=Old(0.9), netCorr_ema=Old(0.8))
    shadow = t.netG_ema.shadow

    def update_fixed_params():
        t.optimizer_G = _adam(net)
    t.update_fixed_params = update_fixed_params
    optim.fuse_trainer(t)
    assert t.optimizer_G.cocos_fused and isinstance(t.netG_ema, optim.EMA) and t.netG_ema.shadow is shadow and t.netCorr_ema.mu == 0.8
    old = t.optimizer_G
    t.update_fixed_params()
    assert t.optimizer_G is not old and t.optimizer_G.cocos_fused


# ---- 6. with the gradient exchange, world size 2 on gloo ------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(global_batch=4):
    g = torch.Generator().manual_seed(1)
    return torch.randn(global_batch, 5, 6, 6, generator=g), torch.randn(global_batch, 3, 6, 6, generator=g)


def _worker(rank, world, port, fuse_first, align, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from cocosnet_amd import dist as cdist, optim, trainer
    cdist.init_from_env("gloo")
    net = _net()
    o = _adam(net)
    if fuse_first:
        optim.fuse_adam(o)
        trainer.attach_gradient_exchange(o, bucket_bytes=256, align_elems=align)
    else:
        trainer.attach_gradient_exchange(o, bucket_bytes=256, align_elems=align)
        optim.fuse_adam(o)
    x, y = _data()
    lo, hi = cdist.shard_batch(x.shape[0], rank, world)
    for _ in range(3):
        o.zero_grad()
        ((net(x[lo:hi]) - y[lo:hi]) ** 2).mean().backward()
        o.step()
    b = o.grad_buckets
    aligned = all(b._offset_of[p] % align == 0 for p in b.params)
    ret[rank] = ([p.detach().clone() for p in net.parameters()], aligned, b.in_flight())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("fuse_first", [True, False])
@pytest.mark.parametrize("align", [1, 4])
def test_fused_step_with_the_gradient_exchange_on_gloo(fuse_first, align):
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, fuse_first, align, ret), nprocs=world, join=True)
    net = _net()
    o = _adam(net)
    x, y = _data()
    for _ in range(3):
        o.zero_grad()
        ((net(x) - y) ** 2).mean().backward()
        o.step()
    for a, b in zip(ret[0][0], ret[1][0]):
        assert torch.equal(a, b)                               # identical replicas
    for rank in range(world):
        params, aligned, in_flight = ret[rank]
        assert aligned and in_flight == 0
        for a, b in zip(params, net.parameters()):
            torch.testing.assert_close(a, b, atol=2e-5, rtol=1e-4)


def test_align_elems_1_is_the_layout_without_the_argument():
    from cocosnet_amd import dist as cdist
    a, b, c = _net(), _net(), _net()
    ba = cdist.GradBuckets(a.parameters(), bucket_bytes=256)
    bb = cdist.GradBuckets(b.parameters(), bucket_bytes=256, align_elems=1)
    bc = cdist.GradBuckets(c.parameters(), bucket_bytes=256, align_elems=4)
    assert [f.numel() for f in ba._flat] == [f.numel() for f in bb._flat]
    off = lambda bk, net: [(bk._bucket_of[p], (p.grad.data_ptr() - bk._flat[bk._bucket_of[p]].data_ptr()) // 4) for p in net.parameters()]
    assert off(ba, a) == off(bb, b)
    assert all(o % 4 == 0 for _, o in off(bc, c)) and any(o % 4 for _, o in off(ba, a))
    for p in c.parameters():
        assert p.grad.shape == p.shape
    # the padding survives zero_grad() re-attaching a dropped view
    first = next(iter(c.parameters()))
    first.grad = None
    bc.zero_grad()
    assert (first.grad.data_ptr() - bc._flat[bc._bucket_of[first]].data_ptr()) // 4 == bc._offset_of[first]
    with pytest.raises(ValueError):
        cdist.GradBuckets(_net().parameters(), align_elems=0)
