"""Audit of the version-keyed caches of cocosnet_amd.ops: the max|x| cells (`_remember_amax` / `_recall_amax`) and the row dot D that
warp_head's backward leaves for the next softmax backward (`_rowdot_cached`).

`audit(monkeypatch)` replaces the three functions by checking wrappers and returns the `Audit` that collects what they saw:

  * a SITE is a line of ops.py / inference.py that calls `_remember_amax` (producer) or `_recall_amax` (consumer), named after the
    function or method that contains it.  The full set comes from the SOURCE (ast), so a site added later is known — and uncovered
    until a workload reaches it;
  * at remember time the cell must hold EXACTLY max|tensor| (the contract in the docstring of test_gpu_amax_epilogues.py);
  * at every recall that returns a cell the same equality must hold against the tensor as it is THEN, and the (producer, consumer)
    pair is recorded;
  * when `_rowdot_cached` returns the cached D, D is compared with the fp64 row dot rounded to fp32.  Both sides accumulate in fp64
    and round once, so they differ by one rounding flip at most: one fp32 ulp at the size of sum_c |dout * out|.  This is the only
    tolerance of the file.

There is no allow-list: a cell that is not exact is an AssertionError at the site that left (or found) it.

`caches_off(monkeypatch)`: the other arm — every consumer takes its own pass (no recall returns a cell, D is always recomputed).
warp_head's backward leaves D in the SAME backward that consumes it, so clearing `known_rowdot` in front of a backward would not
switch it off: `_rowdot_cached` itself is replaced."""
import ast
import os
import sys

import torch

NAMES = ("_remember_amax", "_recall_amax")


def _sites_of(path):
    """{name: {(file, first line, last line): qualified name of the enclosing def / class}} of the calls of NAMES in `path`"""
    with open(path) as fh:
        tree = ast.parse(fh.read())
    found = {n: {} for n in NAMES}
    base = os.path.basename(path)

    def walk(node, scope):
        for child in ast.iter_child_nodes(node):
            sub = scope
            if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                sub = scope + [child.name]
            if isinstance(child, ast.Call):
                f = child.func
                name = f.id if isinstance(f, ast.Name) else (f.attr if isinstance(f, ast.Attribute) else None)
                if name in NAMES:
                    found[name][(base, child.lineno, child.end_lineno)] = ".".join(scope) or "<module>"
            walk(child, sub)
    walk(tree, [])
    return found


class Audit:
    def __init__(self, ops, inference):
        self.ops = ops
        self.producers, self.consumers = {}, {}        # (file, line) -> qualified name
        self._span = {}                                # (file, line within a call) -> (file, first line)
        for mod in (ops, inference):
            got = _sites_of(mod.__file__)
            for name, table in ((NAMES[0], self.producers), (NAMES[1], self.consumers)):
                for (base, l0, l1), qual in got[name].items():
                    table[(base, l0)] = qual
                    for ln in range(l0, l1 + 1):
                        self._span[(name, base, ln)] = (base, l0)
        self.reached_producers, self.reached_consumers = set(), set()
        self.pairs = set()                             # (producer site, consumer site)
        self.hits = 0                                  # recalls that returned a verified cell + cached D's returned
        self.rowdot_hits = 0
        self._made_by = {}                             # id(cell) -> (cell, producer site): the cell is held, its id stays its own

    # ---- who is calling ------------------------------------------------------------------------------------------------------
    def _site(self, name, frame):
        key = (name, os.path.basename(frame.f_code.co_filename), frame.f_lineno)
        site = self._span.get(key)
        assert site is not None, f"{name} called from {key[1]}:{key[2]}, which the source scan does not know as a call site"
        return site

    def label(self, site):
        qual = self.producers.get(site) or self.consumers.get(site)
        return f"{site[0]}:{site[1]} ({qual})"

    @staticmethod
    def _exact(cell, t):
        return float(cell) == float(t.detach().abs().max())

    # ---- the wrappers --------------------------------------------------------------------------------------------------------
    def install(self, monkeypatch):
        ops, real_remember, real_recall, real_rowdot = self.ops, self.ops._remember_amax, self.ops._recall_amax, self.ops._rowdot_cached

        def remember(t, cell, weak=False):
            site = self._site(NAMES[0], sys._getframe(1))
            assert cell.numel() == 1 and self._exact(cell, t), (
                f"{self.label(site)} remembers {float(cell)!r} for a tensor {tuple(t.shape)} whose max|.| is {float(t.detach().abs().max())!r}")
            self.reached_producers.add(site)
            self._made_by[id(cell)] = (cell, site)
            return real_remember(t, cell, weak)

        def recall(t, consume=True):
            site = self._site(NAMES[1], sys._getframe(1))
            cell = real_recall(t, consume)
            if cell is not None:
                made = self._made_by.get(id(cell))
                src = self.label(made[1]) if made is not None else "a producer outside the audit"
                assert self._exact(cell, t), (
                    f"{self.label(site)} recalls {float(cell)!r} (left by {src}) for a tensor {tuple(t.shape)} whose max|.| is now "
                    f"{float(t.detach().abs().max())!r}")
                self.reached_consumers.add(site)
                self.hits += 1
                if made is not None:
                    self.pairs.add((made[1], site))
            return cell

        def rowdot_cached(dout, out):
            ent = ops._tls.known_rowdot
            d = real_rowdot(dout, out)
            if ent is not None and d is ent[3]:
                prod = dout.double() * out.double()
                ref = prod.sum(1).float()
                size = prod.abs().sum(1).float()
                ulp = torch.nextafter(size, torch.full_like(size, float("inf"))) - size
                worst = float(((d - ref).abs() / ulp).max())
                assert bool(((d - ref).abs() <= ulp).all()), f"the cached row dot D is {worst:.3g} ulp(sum|dout * out|) from the fp64 row dot"
                self.hits += 1
                self.rowdot_hits += 1
            return d

        monkeypatch.setattr(ops, "_remember_amax", remember)
        monkeypatch.setattr(ops, "_recall_amax", recall)
        monkeypatch.setattr(ops, "_rowdot_cached", rowdot_cached)
        return self

    # ---- the report ----------------------------------------------------------------------------------------------------------
    def uncovered_producers(self):
        return sorted(set(self.producers) - self.reached_producers)

    def uncovered_consumers(self):
        return sorted(set(self.consumers) - self.reached_consumers)

    def report(self):
        line = (f"CACHE_AUDIT producers {len(self.reached_producers)}/{len(self.producers)} consumers "
                f"{len(self.reached_consumers)}/{len(self.consumers)} hits {self.hits}")
        print(line)
        return line


def audit(monkeypatch) -> Audit:
    from cocosnet_amd import inference, ops
    return Audit(ops, inference).install(monkeypatch)


def caches_off(monkeypatch):
    from cocosnet_amd import ops

    def rowdot(dout, out):
        ops._tls.known_rowdot = None
        return ops._rowdot(dout, out)
    monkeypatch.setattr(ops, "_recall_amax", lambda t, consume=True: None)
    monkeypatch.setattr(ops, "_rowdot_cached", rowdot)


def clear_caches():
    """an empty table, as at the start of a thread: every arm of a comparison starts from the same state"""
    from cocosnet_amd import ops
    ops._tls.known_amax.clear()
    ops._tls.known_rowdot = None
