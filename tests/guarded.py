"""Guarded device allocations for the GPU tests (a helper module: no test, no conftest).

The parity tests compare the tensor they own; the caching allocator places live tensors back to back, so a kernel that stores one tile row
past its output, or loads past the end of an input row, damages or reads some OTHER live tensor and no assertion looks there.  While a
``Guard`` is active every device tensor the package's host layer creates (``torch.empty`` / ``zeros`` / ``full`` and their ``*_like`` forms
inside ``MODULES``) aliases the middle of a buffer of its own:

    [ margin bytes 0xFF | the tensor, rounded up to 512 bytes | margin bytes 0xFF ]

The tensor handed back is not a torch view of that buffer but an alias of the bytes from MARGIN on with a storage of its own (through DLPack):
storage_offset() == 0 and no view relation, as a fresh allocation has.  The host layer keys on both (``Guard._alloc`` says where).

0xFF.. is a NaN in float32, bfloat16 and float64 and 255 in uint8: a load past an extent that reaches a result makes it NaN, ``empty``
buffers read before they are written give NaN (also the ones block_routes.poison cannot reach), and ``check()`` finds every byte a kernel
stored into a margin and names the buffer, its allocating line and the damaged offsets.  MARGIN = 256 KiB is twice the largest block one
workgroup stores (128 rows x 256 channels x 4 B) -- a design condition -- and a multiple of 512, so the tensors keep the alignment the caching
allocator gives and no aligned16 dispatch of the library changes.  A test whose tensors are wider states its own condition and passes
``Guard(margin=...)`` (tests/test_wide_channels_gpu.py: 512 channels, 512 KiB); MARGIN stays the default.

Not covered: an overrun longer than a margin that skips it; a stray store of 0xFF bytes (a packed sign-image or dropout-mask byte with all
eight bits set, an all-ones NaN: the margin's own fill, so the damage test ``byte != 0xFF`` cannot see it); a stray load whose value is
discarded; tensors autograd allocates in C++; allocations inside a graph capture (they pass through); and integer tensors (labels, CSR arrays,
gather indices, frame maps) -- those pass through unguarded on purpose: a poisoned index could become an address, and this harness must never
turn a value bug into a stray access.

Memory: every guarded allocation stays alive until ``check()`` and carries 512 KiB of margin, so a model-level test with thousands of host-layer
allocations holds several GB until its teardown.  An out-of-memory error that appears only under the guard is that, not a finding.

The interception swaps the ``torch`` global of each module in ``MODULES`` for a forwarding proxy that overrides the allocation functions
only; ``torch`` itself is untouched and everything is restored on exit.  ``INTERCEPTED`` is the table of idioms the guard knows;
tests/test_guarded.py scans the host layer and fails on an allocation idiom that is not in it.

For the test modules: the fixtures ``guarded_allocations`` (every test of a module) and ``guarded_gpu_tests`` (a module that mixes host and
device tests: only the tests marked ``gpu``), and two module-level functions that place test inputs through the ACTIVE guard, so that helpers
need no fixture argument: ``put(t, dtype, device)``, a contiguous guarded copy, and ``to(obj, device)``, which is ``obj.to(device)`` with a host
tensor of a guarded dtype landing in a guarded buffer.  Without an active guard (a helper shared with a module that runs without one) both are
the plain copy."""
from __future__ import annotations

import importlib
import os
import sys
from typing import List, Optional

import pytest
import torch

MARGIN = 256 * 1024
ALIGN = 512
FILL = 0xFF
GUARDED_DTYPES = (torch.float32, torch.bfloat16, torch.float64, torch.uint8)

# the modules of the host layer that create device tensors (test_guarded.py: no other module of the package does)
MODULES = tuple("fusion_gcn_amd." + m for m in (
    "ops", "block", "fops", "packing", "optim", "loss", "metrics", "data", "dp", "models.agcn.agcn", "models.mmargcn.agcn",
    "models.mmargcn.graph_convolution", "models.msg3d.ms_gcn", "models.msg3d.ms_tcn"))

# idiom -> what the body holds: "fill" = left 0xFF, "zero", "value" = the call's fill value
INTERCEPTED = {"empty": "fill", "empty_like": "fill", "zeros": "zero", "zeros_like": "zero", "full": "value", "full_like": "value"}

_TESTS = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_TESTS)
_SITE_DIRS = (os.path.join(_ROOT, "fusion_gcn_amd") + os.sep, _TESTS + os.sep)
_THIS = os.path.abspath(__file__)
_active: Optional["Guard"] = None


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _call_site() -> str:
    """file:line of the first frame inside fusion_gcn_amd/ or tests/ (this module excepted)"""
    f = sys._getframe(2)
    while f is not None:
        name = f.f_code.co_filename
        if name.startswith(_SITE_DIRS) and name != _THIS:
            return f"{os.path.relpath(name, _ROOT)}:{f.f_lineno}"
        f = f.f_back
    return "?"


class _Buffer:
    __slots__ = ("raw", "nbytes", "shape", "dtype", "site", "margin")

    def __init__(self, raw, nbytes, shape, dtype, site, margin=MARGIN):
        self.raw, self.nbytes, self.shape, self.dtype, self.site, self.margin = raw, nbytes, shape, dtype, site, margin

    def margins(self):
        """(side, bytes of that margin, offset of its first byte relative to the tensor's start / end)"""
        back = self.margin + self.nbytes                  # (the rounding bytes behind the tensor belong to the back margin)
        return (("front", self.raw[:self.margin], -self.margin), ("back", self.raw[back:], 0))


class _TorchProxy:
    """stands in for the ``torch`` global of one module: the allocation functions of ``INTERCEPTED`` go through the guard, all else forwards"""

    def __init__(self, guard: "Guard"):
        for name in INTERCEPTED:
            setattr(self, name, guard._wrap(name))

    def __getattr__(self, name):            # (only reached for what the instance does not define)
        return getattr(torch, name)


class Guard:
    """Context manager: guarded allocations inside ``MODULES`` (+ ``modules``) on ``device``'s type; ``check()`` verifies every margin.

    Not re-entrant, single-threaded.  ``trace=True`` additionally verifies the margins after every C-ABI entry point (the ``check`` that
    ops passes each return code through) and names the entry point: slow, for locating a finding.  ``margin``: bytes of 0xFF on each side of
    every tensor, a multiple of 512; MARGIN unless a test's tensors are wider than its design condition (the module docstring)."""

    def __init__(self, device="cuda", trace: bool = False, modules=(), margin: int = MARGIN):
        if margin <= 0 or margin % ALIGN:
            raise ValueError(f"margin = {margin}: a positive multiple of {ALIGN} bytes keeps the allocator's alignment")
        self.margin = margin
        self.device_type = torch.device(device).type
        self.trace = trace
        self.extra = tuple(modules)
        self.buffers: List[_Buffer] = []
        self.handed_out = 0
        self._saved: list = []

    # ---- activation ----------------------------------------------------------------------------------------------------------------------
    def __enter__(self) -> "Guard":
        global _active
        if _active is not None:
            raise RuntimeError("a Guard is already active: it is not re-entrant")
        _active = self
        try:
            proxy = _TorchProxy(self)
            for mod in [importlib.import_module(m) for m in MODULES] + list(self.extra):
                if vars(mod).get("torch") is not torch:
                    raise RuntimeError(f"{mod.__name__} has no plain `torch` global to intercept")
                self._saved.append((mod, "torch", torch))
                mod.torch = proxy
            if self.trace:
                lib = importlib.import_module("fusion_gcn_amd._lib")
                real = lib.check

                def traced_check(rc, what):
                    real(rc, what)
                    self._verify(f"after entry point {what}")
                for mod in (lib, importlib.import_module("fusion_gcn_amd.ops")):      # (ops imports it by name; optim and packing call _lib.check)
                    self._saved.append((mod, "check", real))
                    mod.check = traced_check
        except BaseException:
            self._restore()
            raise
        return self

    def __exit__(self, *exc) -> bool:
        self._restore()
        return False

    def _restore(self) -> None:
        global _active
        for mod, name, value in reversed(self._saved):
            setattr(mod, name, value)
        self._saved = []
        _active = None

    # ---- allocation ----------------------------------------------------------------------------------------------------------------------
    def _alloc(self, shape, strides, dtype, device, site: str) -> torch.Tensor:
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * dtype.itemsize
        margin = self.margin
        raw = torch.full((margin + round_up(nbytes, ALIGN) + margin,), FILL, dtype=torch.uint8, device=device)
        self.buffers.append(_Buffer(raw, nbytes, tuple(shape), dtype, site, margin))
        self.handed_out += 1
        if not nbytes:
            return torch.empty_strided(tuple(shape), tuple(strides), dtype=dtype, device=device)      # no element: nothing to alias
        # an alias of the bytes from ``margin`` on with a storage of its own: storage_offset() == 0 and no view relation, as a fresh allocation
        # has -- the host layer keys on both (FlatOptimizer finds a parameter's place in its flat buffers by the storage offset of the
        # gradient view; autograd refuses an in-place op on a custom Function's output that is a view).  The storage keeps ``raw`` alive
        alias = torch.from_dlpack(raw[margin:margin + nbytes])
        return torch.empty(0, dtype=dtype, device=device).set_(alias.untyped_storage(), 0, tuple(shape), tuple(strides))

    def _wrap(self, name: str):
        real, body = getattr(torch, name), INTERCEPTED[name]

        def alloc(*args, **kwargs):
            if kwargs.get("pin_memory") or kwargs.get("out") is not None:
                return real(*args, **kwargs)
            meta = real(*args, **{**kwargs, "device": "meta"})            # shape, strides and dtype exactly as torch would give them
            device = kwargs.get("device")
            if device is None:
                device = args[0].device if name.endswith("_like") else torch.get_default_device()
            device = torch.device(device)
            if device.type != self.device_type or meta.dtype not in GUARDED_DTYPES or meta.layout != torch.strided:
                return real(*args, **kwargs)
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                return real(*args, **kwargs)            # inside a graph capture the allocations are the capture pool's own: not guarded
            out = self._alloc(meta.shape, meta.stride(), meta.dtype, device, _call_site())
            if body == "zero":
                out.zero_()
            elif body == "value":
                out.fill_(kwargs["fill_value"] if "fill_value" in kwargs else args[1])
            if kwargs.get("requires_grad"):
                out.requires_grad_(True)
            return out
        alloc.__name__ = name
        return alloc

    def put(self, cpu_tensor: torch.Tensor, dtype: Optional[torch.dtype] = None, device=None) -> torch.Tensor:
        """a guarded device copy of a test input (contiguous): NaN in front of its first and behind its last element"""
        src = cpu_tensor.detach()
        dtype = src.dtype if dtype is None else dtype
        device = torch.device(device if device is not None else ("cuda:0" if self.device_type == "cuda" else "cpu"))
        if dtype not in GUARDED_DTYPES:
            return src.to(device=device, dtype=dtype).contiguous()
        out = self._alloc(src.shape, torch.empty(src.shape, device="meta").stride(), dtype, device, _call_site())
        out.copy_(src)
        return out

    # ---- verification --------------------------------------------------------------------------------------------------------------------
    def _damaged(self, buffers) -> bool:
        """whether any margin holds a changed byte: one minimum per margin, gathered on the device, one synchronisation per device"""
        lows = {}
        for b in buffers:
            for _, m, _ in b.margins():
                lows.setdefault(m.device, []).append(m.amin())
        return any(int(torch.stack(v).amin()) != FILL for v in lows.values())

    def _report(self, buffers, when: str) -> str:
        lines = []
        for b in buffers:
            for side, m, base in b.margins():
                idx = (m != FILL).nonzero().flatten()
                if idx.numel():
                    first, last = int(idx[0]) + base, int(idx[-1]) + base
                    rel = "the tensor's start" if side == "front" else "the tensor's end"
                    lines.append(f"{tuple(b.shape)} {b.dtype} allocated at {b.site}: {side} margin damaged, {idx.numel()} bytes, "
                                 f"offsets {first}..{last} relative to {rel}")
        return f"stores outside a guarded tensor ({when}):\n  " + "\n  ".join(lines)

    def _verify(self, when: str) -> None:
        if self._damaged(self.buffers):
            raise AssertionError(self._report(self.buffers, when))

    def check(self) -> None:
        """Verify every margin of every buffer handed out since activation (or the last check) and drop the references"""
        try:
            self._verify("found by Guard.check")
        finally:
            self.buffers = []


@pytest.fixture
def guarded_allocations():
    """the test runs under a Guard; its margins are verified at teardown"""
    with Guard() as guard:
        yield guard
    guard.check()


@pytest.fixture
def guarded_gpu_tests(request):
    """for a module that mixes host and device tests: the tests marked ``gpu`` run under a Guard, the others as they are"""
    if request.node.get_closest_marker("gpu") is None:
        yield None
        return
    with Guard() as guard:
        yield guard
    guard.check()


def active() -> Optional[Guard]:
    return _active


def to(obj, device):
    """``obj.to(device)``; a host tensor of a guarded dtype lands in a guarded buffer of the active guard, with the strides ``.to`` would give
    it.  Everything else is torch's own ``.to``: modules (their parameters are not guarded), integer tensors, tensors that are on a device
    already or that require grad (the copy is part of the graph), and any call without an active guard."""
    g, dev = _active, torch.device(device)
    if (g is None or not isinstance(obj, torch.Tensor) or obj.device.type != "cpu" or dev.type != g.device_type or obj.dtype not in GUARDED_DTYPES
            or obj.requires_grad or obj.layout != torch.strided or (dev.type == "cuda" and torch.cuda.is_current_stream_capturing())):
        return obj.to(device)
    meta = torch.empty_like(obj, device="meta")
    out = g._alloc(meta.shape, meta.stride(), obj.dtype, dev, _call_site())
    out.copy_(obj)
    return out


def put(t: torch.Tensor, dtype: Optional[torch.dtype] = None, device=None) -> torch.Tensor:
    """``Guard.put`` of the active guard; a plain device copy where none is active (a helper shared with a module that runs without the guard)"""
    if _active is not None:
        return _active.put(t, dtype, device)
    t = t.detach().to(device=device if device is not None else "cuda:0")
    return (t if dtype is None else t.to(dtype)).contiguous()
