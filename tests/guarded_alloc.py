"""Red zones around every buffer a kernel is handed: `guarded()` makes torch's allocation functions carve each tensor out of a flat byte
buffer `guard | interior | guard`, all of it filled with 0xFF, and `check()` reports every guard byte that is no longer 0xFF.

0xFF..FF is NaN in fp32, fp64, f16 and bf16 and -1 in the integer types: a kernel that WRITES outside its buffer damages a guard (up to
G bytes either side; further out it lands where it lands today), one that READS outside it, or reads an interior nobody wrote, carries
a NaN into whatever it computes.  The carved tensor sits at a storage offset of at least G bytes, so `untyped_storage().data_ptr()`
handed over where `data_ptr()` is meant points into the guard in front.

    with guarded() as g:                   # device_type="cuda"; "cpu" exercises the helper itself
        x = g.place(x)                     # inputs, parameters, optimiser state: copied into a guarded buffer
        y = op(x)                          # every torch.empty / empty_like / zeros / zeros_like / full / new_empty / new_zeros inside is carved
        bad = g.check()                    # [Violation(entry, site, side, offset, nbytes)]

While the context is active `cocosnet_amd._lib.call` is wrapped: after each call the guards that were intact before it are compared
again and what is newly damaged is stamped with the entry point's name; `g.entries` is the set of names reached.

What cannot be carved (out=, pinned memory, a layout or memory format other than the default, an `empty_like` source that overlaps
itself) goes to the real function and is counted in `g.passthroughs` with its call site; other devices pass through uncounted.

G is a design constant (64 KiB, a multiple of the 512 B the caching allocator aligns to), not a measurement."""
import collections
import os
import sys
import threading

import torch

G = 64 * 1024
ALIGN = 512
FILL = 0xFF

_HERE = os.path.abspath(__file__)
_REPO = os.path.dirname(os.path.dirname(_HERE))
_PKG = os.path.join(_REPO, "cocosnet_amd") + os.sep

Violation = collections.namedtuple("Violation", "entry site side offset nbytes")
Violation.__str__ = lambda v: (f"{v.entry or '<no entry point>'}: {v.nbytes} byte(s) damaged {v.side} the buffer allocated at {v.site}, first at "
                               f"offset {v.offset:+d} from the interior")


class Allocation:
    __slots__ = ("flat", "nbytes", "site", "in_pkg", "intact")

    def __init__(self, flat, nbytes, site, in_pkg):
        self.flat, self.nbytes, self.site, self.in_pkg = flat, nbytes, site, in_pkg
        self.intact = {"before": True, "after": True}

    def guard(self, side):
        return self.flat[:G] if side == "before" else self.flat[G + self.nbytes:]


def _site(depth=2):
    """(file:line, inside cocosnet_amd/) of the first frame inside the package, else of the caller of the patched function"""
    f = sys._getframe(depth)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    caller, g = f, f
    while g is not None:
        if os.path.abspath(g.f_code.co_filename).startswith(_PKG):
            return f"{os.path.relpath(g.f_code.co_filename, _REPO)}:{g.f_lineno}", True
        g = g.f_back
    if caller is None:
        return "<unknown>", False
    name = caller.f_code.co_filename
    name = os.path.relpath(name, _REPO) if os.path.abspath(name).startswith(_REPO + os.sep) else name
    return f"{name}:{caller.f_lineno}", False


def _size_of(args, kwargs):
    if "size" in kwargs:
        size = kwargs.pop("size")
    elif len(args) == 1 and not isinstance(args[0], int) and not (torch.is_tensor(args[0]) and args[0].dim() == 0):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


def _contiguous_strides(size):
    st, acc = [], 1
    for s in reversed(size):
        st.append(acc)
        acc *= max(int(s), 1)
    return tuple(reversed(st))


class guarded:
    def __init__(self, device_type="cuda"):
        self.device_type = device_type
        self.allocations = []
        self.passthroughs = collections.Counter()          # (site, inside cocosnet_amd/, why) -> count
        self.violations = []
        self.entries = set()
        self.calls = 0
        self._lock = threading.RLock()
        self._saved = None

    # ---- the context -----------------------------------------------------------------------------------------------------------
    def __enter__(self):
        from cocosnet_amd import _lib
        T = torch.Tensor
        self._saved = [(torch, n, getattr(torch, n)) for n in ("empty", "empty_like", "zeros", "zeros_like", "full")]
        self._saved += [(T, "new_empty", T.new_empty), (T, "new_zeros", T.new_zeros), (_lib, "call", _lib.call)]
        real = {(o, n): f for o, n, f in self._saved}
        self._empty = real[(torch, "empty")]
        try:
            torch.empty = self._factory(real[(torch, "empty")], fill=None)
            torch.zeros = self._factory(real[(torch, "zeros")], fill=0)
            torch.full = self._factory(real[(torch, "full")], fill="arg")
            torch.empty_like = self._like(real[(torch, "empty_like")], fill=None)
            torch.zeros_like = self._like(real[(torch, "zeros_like")], fill=0)
            T.new_empty = self._new(real[(T, "new_empty")], fill=None)
            T.new_zeros = self._new(real[(T, "new_zeros")], fill=0)
            _lib.call = self._wrap_call(real[(_lib, "call")])
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc):
        self._restore()
        with self._lock:
            for a in self.allocations:      # the flat buffers were held until here
                a.flat = None
        return False

    def _restore(self):
        for obj, name, fn in self._saved or ():
            setattr(obj, name, fn)
        self._saved = None

    # ---- carving ---------------------------------------------------------------------------------------------------------------
    def _mine(self, device):
        return torch.device(device).type == self.device_type

    @staticmethod
    def _device(device):
        if device is None:
            return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
        if isinstance(device, int):
            return torch.device("cuda", device)
        return torch.device(device)

    def _carve(self, size, stride, dtype, device, site, in_pkg):
        size = tuple(int(s) for s in size)
        stride = _contiguous_strides(size) if stride is None else tuple(int(s) for s in stride)
        item = torch._utils._element_size(dtype)
        numel = 1
        for s in size:
            numel *= s
        extent = 0 if numel == 0 else 1 + sum((s - 1) * st for s, st in zip(size, stride))
        nbytes = extent * item
        raw = self._empty(G + nbytes + G + ALIGN - 1, dtype=torch.uint8, device=device)
        off = -raw.data_ptr() % ALIGN                       # 0 on the device (512-byte blocks); the host allocator aligns to 64
        flat = raw[off:off + G + nbytes + G]
        flat.fill_(FILL)
        t = self._empty(0, dtype=dtype, device=device)
        t.set_(flat.untyped_storage(), (flat.storage_offset() + G) // item, size, stride)
        with self._lock:
            self.allocations.append(Allocation(flat, nbytes, site, in_pkg))
        return t

    def _pass(self, real, args, kwargs, site, in_pkg, why):
        with self._lock:
            self.passthroughs[(site, in_pkg, why)] += 1
        return real(*args, **kwargs)

    @staticmethod
    def _uncarvable(kwargs, like=False):
        if kwargs.get("out") is not None:
            return "out="
        if kwargs.get("pin_memory"):
            return "pinned memory"
        if kwargs.get("layout") not in (None, torch.strided):
            return "layout"
        ok = (None, torch.contiguous_format) + ((torch.preserve_format,) if like else ())
        if kwargs.get("memory_format") not in ok:
            return "memory format"
        if kwargs.get("names") is not None:
            return "named tensor"
        return None

    def _finish(self, t, fill, kwargs):
        if fill is not None:
            t.fill_(fill)
        if kwargs.get("requires_grad"):
            t.requires_grad_(True)
        return t

    def _factory(self, real, fill):
        def patched(*args, **kwargs):
            device = self._device(kwargs.get("device"))
            if not self._mine(device):
                return real(*args, **kwargs)
            site, in_pkg = _site()
            why = self._uncarvable(kwargs)
            if why:
                return self._pass(real, args, kwargs, site, in_pkg, why)
            kw, value, rest = dict(kwargs), fill, args
            if fill == "arg":                                   # torch.full(size, fill_value, ...)
                if "fill_value" in kw:
                    value = kw.pop("fill_value")
                else:
                    value, rest = args[-1], args[:-1]
                if torch.is_tensor(value):
                    value = value.item()
            size = _size_of(rest, kw)
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = torch.get_default_dtype()
                if fill == "arg":
                    dtype = (torch.bool if isinstance(value, bool) else torch.int64 if isinstance(value, int) else
                             torch.complex64 if isinstance(value, complex) else dtype)
            return self._finish(self._carve(size, None, dtype, device, site, in_pkg), value, kw)
        return patched

    def _like(self, real, fill):
        def patched(src, *args, **kwargs):
            device = self._device(kwargs.get("device")) if kwargs.get("device") is not None else src.device
            if not self._mine(device):
                return real(src, *args, **kwargs)
            site, in_pkg = _site()
            why = self._uncarvable(kwargs, like=True) or ("positional arguments" if args else None)
            if not why and src.layout != torch.strided:
                why = "layout"
            if not why and any(st == 0 and s > 1 for s, st in zip(src.shape, src.stride())):
                why = "overlapping source"
            if why:
                return self._pass(real, (src,) + args, kwargs, site, in_pkg, why)
            dtype = kwargs.get("dtype") or src.dtype
            # the strides the real function would give (a dense, non-overlapping source keeps its own), asked of a meta tensor
            meta = torch.empty_strided(tuple(src.shape), src.stride(), dtype=src.dtype, device="meta")
            fmt = kwargs.get("memory_format") or torch.preserve_format
            stride = real(meta, memory_format=fmt).stride()
            return self._finish(self._carve(src.shape, stride, dtype, device, site, in_pkg), fill, kwargs)
        return patched

    def _new(self, real, fill):
        def patched(src, *args, **kwargs):
            device = self._device(kwargs.get("device")) if kwargs.get("device") is not None else src.device
            if not self._mine(device):
                return real(src, *args, **kwargs)
            site, in_pkg = _site()
            why = self._uncarvable(kwargs)
            if why:
                return self._pass(real, (src,) + args, kwargs, site, in_pkg, why)
            kw = dict(kwargs)
            size = _size_of(args, kw)
            return self._finish(self._carve(size, None, kw.get("dtype") or src.dtype, device, site, in_pkg), fill, kw)
        return patched

    def place(self, t, device=None):
        """a copy of `t` (values, shape, dtype, requires_grad; contiguous) inside a guarded buffer on `device` (default: t's own if it
        is of the guarded type, else the guarded type)"""
        if device is None:
            device = t.device if t.device.type == self.device_type else torch.device(self.device_type)
        site, in_pkg = _site()
        out = self._carve(t.shape, None, t.dtype, self._device(device), site, in_pkg)
        with torch.no_grad():
            out.copy_(t.detach())
        return out.requires_grad_(t.requires_grad)

    # ---- the registry ----------------------------------------------------------------------------------------------------------
    @property
    def guarded_count(self):
        return len(self.allocations)

    def passthroughs_inside_package(self):
        return {k: n for k, n in self.passthroughs.items() if k[1]}

    def _synchronise(self):
        if self.device_type == "cuda":
            if torch.cuda.is_current_stream_capturing():
                return False
            torch.cuda.synchronize()
        return True

    def check(self, entry=None):
        """Compare every guard that was intact at the last check with 0xFF; return (and append to self.violations) what is newly damaged."""
        with self._lock:
            if not self._synchronise():
                return []
            todo = [(a, side) for a in self.allocations if a.flat is not None for side in ("before", "after") if a.intact[side]]
            found = []
            by_device = collections.defaultdict(list)
            for a, side in todo:
                by_device[a.flat.device].append((a, side))
            for items in by_device.values():
                both = torch.cat([a.guard(side) for a, side in items]).view(len(items), G)
                damaged = (both != FILL).any(dim=1).cpu().tolist()
                for (a, side), bad in zip(items, damaged):
                    if not bad:
                        continue
                    a.intact[side] = False
                    where = (a.guard(side) != FILL).nonzero().flatten().cpu()
                    first = int(where[0])
                    offset = first - G if side == "before" else a.nbytes + first
                    found.append(Violation(entry, a.site, side, offset, int(where.numel())))
            self.violations += found
            return found

    def _wrap_call(self, real):
        def call(name, *args):
            with self._lock:
                self.entries.add(name)
                self.calls += 1
            try:
                return real(name, *args)
            finally:
                self.check(entry=name)
        return call

    def report(self):
        return "\n".join(str(v) for v in self.violations)
