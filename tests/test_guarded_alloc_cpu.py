"""tests/guarded_alloc.py checked on the host (`guarded(device_type="cpu")`), no kernel involved: the damage is done with plain torch
indexing into the registry's own flat buffers."""
import os
import sys
import threading

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as ga  # noqa: E402
from guarded_alloc import G, guarded  # noqa: E402

PATCHED = [(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "full")] + [(torch.Tensor, "new_empty"), (torch.Tensor, "new_zeros")]
THIS = os.path.join("tests", os.path.basename(__file__))


def _line():
    return sys._getframe(1).f_lineno


def test_carved_tensors_have_the_asked_shape_dtype_strides_and_alignment():
    with guarded("cpu") as g:
        src = torch.arange(24.0).reshape(2, 3, 4).permute(2, 0, 1)          # dense, non-overlapping, not contiguous
        got = {
            "empty": (torch.empty(3, 5, dtype=torch.float16), (3, 5), torch.float16, (5, 1)),
            "empty_tuple": (torch.empty((2, 0, 3)), (2, 0, 3), torch.float32, (3, 3, 1)),
            "empty_size_kw": (torch.empty(size=(7,), dtype=torch.float64, device="cpu"), (7,), torch.float64, (1,)),
            "scalar": (torch.empty((), dtype=torch.int32), (), torch.int32, ()),
            "zeros": (torch.zeros(4, 1, 3, dtype=torch.int64), (4, 1, 3), torch.int64, (3, 3, 1)),
            "full": (torch.full((2, 3), 1.5), (2, 3), torch.float32, (3, 1)),
            "full_int": (torch.full((3,), 7), (3,), torch.int64, (1,)),
            "empty_like": (torch.empty_like(src), (4, 2, 3), torch.float32, src.stride()),
            "empty_like_contig": (torch.empty_like(src, memory_format=torch.contiguous_format), (4, 2, 3), torch.float32, (6, 3, 1)),
            "zeros_like": (torch.zeros_like(src, dtype=torch.bfloat16), (4, 2, 3), torch.bfloat16, src.stride()),
            "empty_like_slice": (torch.empty_like(src[:, :, ::2]), (4, 2, 2), torch.float32, torch.empty_like(src[:, :, ::2].to("meta")).stride()),
            "new_empty": (src.new_empty((5, 2)), (5, 2), torch.float32, (2, 1)),
            "new_zeros": (src.new_zeros(3, dtype=torch.uint8), (3,), torch.uint8, (1,)),
            "place": (g.place(src), (4, 2, 3), torch.float32, (6, 3, 1)),
        }
        for name, (t, shape, dtype, stride) in got.items():
            assert tuple(t.shape) == shape and t.dtype == dtype and t.stride() == tuple(stride), (name, t.shape, t.dtype, t.stride())
            assert t.data_ptr() % 512 == 0, name
            assert t.storage_offset() * t.element_size() >= G, name
        assert bool((got["zeros"][0] == 0).all()) and bool((got["zeros_like"][0] == 0).all()) and bool((got["new_zeros"][0] == 0).all())
        assert bool((got["full"][0] == 1.5).all()) and bool((got["full_int"][0] == 7).all())
        assert torch.equal(got["place"][0], src)
        assert bool(torch.isnan(got["empty"][0]).all()) and bool(torch.isnan(got["empty_size_kw"][0]).all())       # 0xFF.. is NaN
        assert bool((got["scalar"][0] == -1).all())
        assert torch.empty(2, requires_grad=True).requires_grad and g.place(src.clone().requires_grad_()).requires_grad
        assert g.guarded_count == len(got) + 2 and not g.passthroughs
        for a in g.allocations:
            assert a.flat.numel() == G + a.nbytes + G and a.flat.data_ptr() % 512 == 0
        assert g.check() == []
        # the interiors can be written to their last byte without touching a guard
        for t, *_ in got.values():
            t.fill_(1)
        assert g.check() == [] and g.violations == []


def test_attributes_are_restored_after_normal_exit_and_after_an_exception():
    from cocosnet_amd import _lib
    before = [getattr(o, n) for o, n in PATCHED] + [_lib.call]
    with guarded("cpu"):
        assert all(getattr(o, n) is not f for (o, n), f in zip(PATCHED, before)) and _lib.call is not before[-1]
    assert [getattr(o, n) for o, n in PATCHED] + [_lib.call] == before
    with pytest.raises(ZeroDivisionError):
        with guarded("cpu"):
            1 / 0
    assert [getattr(o, n) for o, n in PATCHED] + [_lib.call] == before


def test_other_devices_pass_through_uncounted():
    with guarded("cuda") as g:
        t = torch.zeros(3)
        assert t.storage_offset() == 0 and g.guarded_count == 0 and not g.passthroughs


@pytest.mark.parametrize("side,at,count", [("before", -1, 1), ("after", 0, 1), ("before", -G, 3), ("after", G - 2, 2)])
def test_one_damaged_byte_is_reported_with_site_side_offset_and_count(side, at, count):
    with guarded("cpu") as g:
        torch.empty(5)
        t = torch.empty(3, 7, dtype=torch.float16); line = _line()        # 42 bytes: the guard behind it starts unaligned
        torch.zeros(2)
        assert g.check() == []
        a = g.allocations[1]
        assert a.nbytes == 42 and a.site == f"{THIS}:{line}" and not a.in_pkg
        first = G + at if side == "before" else G + a.nbytes + at
        a.flat[first:first + count] = 0
        found = g.check()
        assert found == [ga.Violation(None, f"{THIS}:{line}", side, at if side == "before" else a.nbytes + at, count)], found
        assert "byte(s) damaged " + side in str(found[0])
        assert g.check() == [] and g.violations == found          # a damaged guard is reported once
        assert bool(torch.isnan(t).all())                          # the interior was not touched


def test_a_stub_entry_point_that_damages_a_guard_is_named(monkeypatch):
    from cocosnet_amd import _lib
    box = {}

    def stub(name, *args):
        if name == "cocos_overruns":
            box["a"].flat[G + box["a"].nbytes] = 0
        return 0
    monkeypatch.setattr(_lib, "call", stub)
    with guarded("cpu") as g:
        torch.empty(4); line = _line()
        box["a"] = g.allocations[0]
        _lib.call("cocos_fine", 1, 2)
        assert g.violations == []
        _lib.call("cocos_overruns")
        _lib.call("cocos_fine")
        assert g.violations == [ga.Violation("cocos_overruns", f"{THIS}:{line}", "after", 16, 1)]
        assert g.entries == {"cocos_fine", "cocos_overruns"} and g.calls == 3
        assert g.check() == []
    assert _lib.call is stub


def test_passthroughs_are_counted_with_their_site():
    with guarded("cpu") as g:
        out = torch.ones(3)
        torch.zeros(3, out=out); l0 = _line()
        for _ in range(2):
            torch.empty(2, 3, 4, 5, memory_format=torch.channels_last); l1 = _line()
        torch.empty_like(torch.ones(3, 1).expand(3, 4)); l2 = _line()
        assert g.guarded_count == 0
        assert dict(g.passthroughs) == {(f"{THIS}:{l0}", False, "out="): 1, (f"{THIS}:{l1}", False, "memory format"): 2,
                                        (f"{THIS}:{l2}", False, "overlapping source"): 1}
        assert g.passthroughs_inside_package() == {}


def test_the_site_is_the_first_frame_inside_the_package():
    # (no function of the package allocates on the host: code compiled under a file name inside cocosnet_amd/ stands in for one)
    ns = {"torch": torch}
    src = "def inner():\n    return torch.empty(3)\n\n\ndef outer(helper):\n    return helper(inner)\n"
    exec(compile(src, os.path.join(ga._PKG, "pretend.py"), "exec"), ns)
    with guarded("cpu") as g:
        ns["outer"](lambda f: f())                                        # package -> test -> package -> torch.empty
        ns["outer"](lambda f: torch.empty(2, 2, 2, 2, memory_format=torch.channels_last))
        a = g.allocations[0]
        assert a.in_pkg and a.site == os.path.join("cocosnet_amd", "pretend.py") + ":2", a.site
        assert list(g.passthroughs_inside_package()) == [(os.path.join("cocosnet_amd", "pretend.py") + ":6", True, "memory format")]


def test_two_threads_allocating_concurrently_lose_no_records():
    n = 300
    with guarded("cpu") as g:
        def work(k):
            for i in range(n):
                torch.empty(i % 7 + k)
        threads = [threading.Thread(target=work, args=(k,)) for k in (1, 2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert g.guarded_count == 2 * n
        assert sorted(a.nbytes for a in g.allocations) == sorted(4 * (i % 7 + k) for k in (1, 2) for i in range(n))
        assert g.check() == []
