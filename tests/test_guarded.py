"""tests/guarded.py checks itself: margins, contents, interception scope and restoration on the host (``Guard(device="cpu")``), the closure of
its idiom table over the host layer's source, and one margin check on the device."""
import ast
import importlib
import os
import sys

import pytest
import torch

import guarded
from guarded import MARGIN, Guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TORCH = torch                        # (the real one: inside ``cpu_guard`` the name ``torch`` of this module is the guard's proxy)
ME = sys.modules[__name__]           # this module's ``torch`` global is swapped too (``modules=``): the allocations below are the guard's
HERE = os.path.join("tests", "test_guarded.py")


def cpu_guard(**kw):
    return Guard(device="cpu", modules=(ME,), **kw)


def line_of(marker: str) -> int:
    with open(os.path.join(ROOT, HERE)) as f:
        return next(i for i, line in enumerate(f, 1) if line.rstrip().endswith("# " + marker))


@pytest.mark.parametrize("side", ["front", "back"])
def test_a_changed_margin_byte_is_reported_with_side_offset_and_call_site(side):
    with cpu_guard() as g:
        torch.zeros(8, device="cpu")                                                     # a clean neighbour: not in the report
        t = torch.empty((3, 5), device="cpu", dtype=torch.float32)                       # SITE
        raw = g.buffers[-1].raw
        assert raw.dtype == torch.uint8 and raw.numel() == MARGIN + 512 + MARGIN
        raw[MARGIN - 1 if side == "front" else MARGIN + t.numel() * 4] = 7               # ordinary indexing through the raw buffer
        with pytest.raises(AssertionError) as exc:
            g.check()
    msg = str(exc.value)
    assert f"(3, 5) torch.float32 allocated at {HERE}:{line_of('SITE')}: {side} margin damaged, 1 bytes" in msg
    assert ("offsets -1..-1 relative to the tensor's start" if side == "front" else "offsets 0..0 relative to the tensor's end") in msg
    assert "(8,)" not in msg and msg.count("margin damaged") == 1
    assert g.buffers == []                  # references dropped, also after a failure


def test_a_wider_margin_is_laid_out_checked_and_reported_like_the_default_one():
    """``Guard(margin=)``: the tensor starts ``margin`` bytes into its buffer, both margins are that long and 0xFF, damage at their far ends (beyond
    where the default margin would stop) is found and reported relative to the tensor; the default stays MARGIN; a margin that would break the
    512-byte alignment is refused"""
    wide = 2 * MARGIN
    with cpu_guard(margin=wide) as g:
        t = torch.empty((3, 5), device="cpu", dtype=torch.float32)
        b = g.buffers[-1]
        assert b.raw.numel() == wide + 512 + wide and t.data_ptr() - b.raw.data_ptr() == wide and t.data_ptr() % 512 == b.raw.data_ptr() % 512
        assert bool(t.isnan().all()) and bool((b.raw[:wide] == 255).all()) and bool((b.raw[wide + 60:] == 255).all())
        (front, fm, fbase), (back, bm, bbase) = b.margins()
        assert (front, fm.numel(), fbase, back, bm.numel(), bbase) == ("front", wide, -wide, "back", 512 - 60 + wide, 0)
        t.fill_(1.0)
        p = g.put(TORCH.arange(6.0))
        assert p.data_ptr() - g.buffers[-1].raw.data_ptr() == wide and g.buffers[-1].margin == wide
        g.check()                                            # clean, and the tensor's own bytes are not margin
        torch.zeros(4, device="cpu")
        g.buffers[-1].raw[0] = 1                             # the first byte of the front margin ...
        g.buffers[-1].raw[-1] = 1                            # ... and the last of the back one
        with pytest.raises(AssertionError) as exc:
            g.check()
    msg = str(exc.value)
    assert f"front margin damaged, 1 bytes, offsets {-wide}..{-wide} relative to the tensor's start" in msg
    assert f"back margin damaged, 1 bytes, offsets {512 - 16 + wide - 1}..{512 - 16 + wide - 1} relative to the tensor's end" in msg
    with cpu_guard() as g:
        torch.empty(4, device="cpu")
        assert g.margin == MARGIN and g.buffers[-1].margin == MARGIN and g.buffers[-1].raw.numel() == MARGIN + 512 + MARGIN
        g.check()
    for bad in (0, -512, MARGIN + 4):
        with pytest.raises(ValueError, match="multiple of 512"):
            Guard(device="cpu", margin=bad)
    assert guarded.active() is None


def test_first_last_and_count_of_a_damaged_range():
    with cpu_guard() as g:
        torch.zeros((2, 3), device="cpu", dtype=torch.bfloat16)
        g.buffers[-1].raw[MARGIN + 12 + 100:MARGIN + 12 + 164:2] = 0
        with pytest.raises(AssertionError, match=r"back margin damaged, 32 bytes, offsets 100\.\.162 relative to the tensor's end"):
            g.check()


def test_a_byte_changed_inside_the_body_is_not_reported():
    with cpu_guard() as g:
        t = torch.empty(100, device="cpu")
        g.buffers[-1].raw[MARGIN] = 0
        g.buffers[-1].raw[MARGIN + 399] = 0
        t[50] = 1.0
        g.check()


def test_contents_by_call_and_unguarded_pass_through():
    with cpu_guard() as g:
        assert bool(torch.empty((4, 4), device="cpu").isnan().all())
        assert bool(torch.empty(9, device="cpu", dtype=torch.bfloat16).isnan().all())
        assert bool(torch.empty(3, device="cpu", dtype=torch.float64).isnan().all())
        assert bool((torch.empty(11, device="cpu", dtype=torch.uint8) == 255).all())
        like = torch.empty_like(torch.ones((2, 3), dtype=torch.float64))
        assert like.dtype == torch.float64 and bool(like.isnan().all())
        z = torch.zeros((2, 7), device="cpu", dtype=torch.bfloat16)
        assert bool((z == 0).all()) and not bool(torch.signbit(z).any())
        assert bool((torch.zeros_like(like) == 0).all())
        assert bool((torch.full_like(like, 1e-6) == 1e-6).all())
        assert bool((torch.full((5,), 2.5, device="cpu") == 2.5).all())
        assert g.handed_out == 9
        # integer tensors and pinned / other-device allocations are torch's own: untouched, not counted
        idx = torch.zeros(6, dtype=torch.int64, device="cpu")
        assert idx.dtype == torch.int64 and bool((idx == 0).all()) and idx.untyped_storage().nbytes() == 48
        assert torch.full((3,), -1, dtype=torch.int32, device="cpu").untyped_storage().nbytes() == 12
        assert torch.empty(5, dtype=torch.float32, pin_memory=False, device="meta").device.type == "meta"
        assert g.handed_out == 9
        g.check()
    with Guard(modules=(ME,)) as g:          # the default guard is the device's: host allocations (data.py's staging buffers) pass through
        assert torch.empty(5, dtype=torch.float32, device="cpu").untyped_storage().nbytes() == 20
        assert torch.zeros(5, dtype=torch.float32).untyped_storage().nbytes() == 20
        assert g.handed_out == 0


def test_views_are_contiguous_and_aligned():
    with cpu_guard() as g:
        for shape, dt in (((3, 5), torch.float32), ((1,), torch.uint8), ((7, 1, 9), torch.bfloat16), ((129,), torch.float64), ((0,), torch.float32)):
            t = torch.empty(shape, device="cpu", dtype=dt)
            b = g.buffers[-1]
            nbytes = t.numel() * t.element_size()
            assert t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shape and t.storage_offset() == 0
            assert not t._is_view()                  # (autograd refuses in-place ops on a custom Function's output that is a view)
            assert b.raw.numel() == MARGIN + (nbytes + 511) // 512 * 512 + MARGIN and MARGIN % 512 == 0
            if nbytes:
                assert t.data_ptr() - b.raw.data_ptr() == MARGIN and (t.data_ptr() - b.raw.data_ptr()) % 512 == 0
        src = torch.arange(12.0).reshape(3, 4).t()           # put: a contiguous copy of a strided input, NaN on both sides
        p = g.put(src)
        assert p.is_contiguous() and torch.equal(p, src) and p.data_ptr() - g.buffers[-1].raw.data_ptr() == MARGIN
        assert g.put(src, dtype=torch.bfloat16).dtype == torch.bfloat16
        assert g.put(torch.arange(4)).dtype == torch.int64 and len(g.buffers) == 7
        like = torch.empty_like(p.t())                       # empty_like keeps a dense input's strides, as torch's does
        assert like.stride() == p.t().stride()
        del t, p, like
        g.check()


def test_module_globals_are_restored_and_a_second_activation_is_refused():
    mods = [importlib.import_module(m) for m in guarded.MODULES]
    ops = importlib.import_module("fusion_gcn_amd.ops")
    real_check = ops.check
    with cpu_guard(trace=True) as g:
        assert all(m.torch is not TORCH for m in mods) and ME.torch is not TORCH and ops.check is not real_check
        assert ops.torch.float32 is TORCH.float32 and ops.torch.nn is TORCH.nn          # everything else forwards
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with Guard(device="cpu"):
                pass
        assert all(m.torch is not TORCH for m in mods)         # the refused activation undid nothing
        assert guarded.active() is g
    assert all(m.torch is TORCH for m in mods) and ME.torch is TORCH and ops.check is real_check
    with pytest.raises(KeyError):
        with cpu_guard():
            raise KeyError("inside")
    assert all(m.torch is TORCH for m in mods) and ME.torch is TORCH and guarded.active() is None
    with cpu_guard():                            # and the guard can be activated again
        pass


def test_trace_names_the_entry_point_called_last():
    ops = importlib.import_module("fusion_gcn_amd.ops")
    with cpu_guard(trace=True) as g:
        t = torch.empty(16, device="cpu")
        ops.check(0, "fgcn_first")               # (a zero return code: the library is not touched)
        g.buffers[-1].raw[MARGIN + 64] = 0
        with pytest.raises(AssertionError, match="after entry point fgcn_second"):
            ops.check(0, "fgcn_second")
        del t
        g.buffers.clear()


def test_module_level_to_places_host_floats_in_guarded_buffers_and_is_torchs_own_otherwise():
    x = torch.arange(12.0).reshape(3, 4)
    assert guarded.to(x, "cpu") is x and guarded.put(x, device="cpu").untyped_storage().nbytes() == 48          # no guard active: plain
    with cpu_guard() as g:
        a = guarded.to(x, "cpu")
        b = g.buffers[-1]
        assert torch.equal(a, x) and a.data_ptr() - b.raw.data_ptr() == MARGIN and not a._is_view() and tuple(b.shape) == (3, 4)
        assert b.site.startswith(HERE + ":")
        t = guarded.to(x.t(), "cpu")                         # a dense strided source keeps its strides, as ``.to`` keeps them
        assert t.stride() == x.t().stride() and torch.equal(t, x.t())
        n = g.handed_out
        idx = torch.arange(5)
        assert guarded.to(idx, "cpu") is idx                 # integer tensors, modules, leaves that require grad, other devices: torch's own
        lin = TORCH.nn.Linear(2, 2)
        assert guarded.to(lin, "cpu") is lin
        leaf = torch.ones(3, requires_grad=True)
        assert guarded.to(leaf, "cpu") is leaf and guarded.to(x, "meta").device.type == "meta" and g.handed_out == n
        g.check()


# ---- closure: every allocation idiom of the host layer is one the guard intercepts -----------------------------------------------------------
CREATORS = ("empty", "zeros", "ones", "full", "empty_strided")
METHODS = ("new_empty", "new_zeros", "new_full", "new_ones", "new_tensor")


def package_sources():
    top = os.path.join(ROOT, "fusion_gcn_amd")
    for d, _, files in os.walk(top):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(d, f)
                yield os.path.relpath(path, ROOT)[:-3].replace(os.sep, "."), path


def allocation_calls(path: str):
    """(idiom, line, names a device, zero-size literal): the tensor-creating ``torch.<name>(`` calls and ``.new_*(`` method calls of a file.
    A device is named by ``device=``, by a ``**`` dictionary (``**f32``), or implicitly by a ``*_like`` function / ``new_*`` method"""
    with open(path) as f:
        tree = ast.parse(f.read(), path)
    for node in ast.walk(tree):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        name, on_torch = node.func.attr, isinstance(node.func.value, ast.Name) and node.func.value.id == "torch"
        if on_torch and (name in CREATORS or name.endswith("_like")):
            kws = [k.arg for k in node.keywords]
            yield name, node.lineno, ("device" in kws or None in kws or name.endswith("_like")), False
        elif name in METHODS:
            zero = len(node.args) == 1 and isinstance(node.args[0], ast.Constant) and node.args[0].value == 0
            yield "." + name, node.lineno, True, zero


def unintercepted(table) -> list:
    bad = []
    for mod, path in package_sources():
        for idiom, line, device, zero in allocation_calls(path):
            if not device:
                continue                    # a host tensor (CSR arrays, pinned staging buffers, module parameters before .to())
            if idiom.startswith("."):
                if not zero:                # a tensor method cannot be reached through a module's ``torch`` global: only the zero-element
                    bad.append(f"{mod}:{line} {idiom}(...) allocates through a tensor method")       # placeholder (nothing to guard) may
            elif idiom not in table:
                bad.append(f"{mod}:{line} torch.{idiom} is not an idiom the guard intercepts")
            elif mod not in guarded.MODULES:
                bad.append(f"{mod}:{line} torch.{idiom}: the module is not in guarded.MODULES")
    return bad


def test_every_allocation_idiom_of_the_host_layer_is_intercepted():
    found = {(mod, idiom) for mod, path in package_sources() for idiom, _, device, _ in allocation_calls(path) if device}
    assert len(found) > 20 and ("fusion_gcn_amd.ops", "empty") in found and ("fusion_gcn_amd.metrics", "full") in found       # the scan sees them
    bad = unintercepted(guarded.INTERCEPTED)
    assert not bad, "\n".join(bad)
    for m in guarded.MODULES:                # a plain ``import torch`` in each: what the proxy replaces
        assert vars(importlib.import_module(m)).get("torch") is TORCH, m
    # the modules the guard was specified for are all in its list
    for m in ("ops", "block", "fops", "packing", "optim", "loss", "metrics", "data", "dp", "models.mmargcn.agcn", "models.mmargcn.graph_convolution",
              "models.msg3d.ms_gcn", "models.msg3d.ms_tcn"):
        assert "fusion_gcn_amd." + m in guarded.MODULES


def test_the_closure_scan_fails_on_an_idiom_the_guard_does_not_know():
    for missing in ("full", "empty_like", "zeros"):
        table = {k: v for k, v in guarded.INTERCEPTED.items() if k != missing}
        assert any(f"torch.{missing} is not" in line for line in unintercepted(table)), missing


# ---- the same margin check on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_store_past_the_end_is_reported_on_the_device():
    """One element written behind a guarded tensor through the RAW buffer with torch indexing (the write stays inside the test's own
    allocation; no kernel overruns anything): check() reports it, and with trace=True the report names the entry point called just before."""
    from fusion_gcn_amd import ops
    with Guard(trace=True) as g:
        x = g.put(torch.arange(2 * 33 * 5, dtype=torch.float32).reshape(2, 33, 5))
        assert x.is_cuda and x.is_contiguous() and x.data_ptr() % 512 == 0
        out = ops.transpose(x, 64)                           # margins verified after the entry point: clean
        raw = g.buffers[-1].raw
        assert tuple(g.buffers[-1].shape) == (2, 5, 64) and out.data_ptr() - raw.data_ptr() == MARGIN
        assert bool(torch.isnan(raw[:MARGIN].view(torch.float32)).all()) and bool(torch.isnan(raw[MARGIN + out.numel() * 4:].view(torch.float32)).all())
        raw[MARGIN + out.numel() * 4:MARGIN + out.numel() * 4 + 4] = 0          # "out.flatten()[numel] = 0.0"
        with pytest.raises(AssertionError) as exc:
            ops.transpose_into(out, 33)
        msg = str(exc.value)
        assert "after entry point fgcn_transpose" in msg and "(2, 5, 64) torch.float32 allocated at fusion_gcn_amd/ops.py:" in msg
        assert "back margin damaged, 4 bytes, offsets 0..3 relative to the tensor's end" in msg
        with pytest.raises(AssertionError, match="found by Guard.check"):
            g.check()
    with Guard() as g:                                       # without trace: found at check()
        e = ops.torch.empty((4, 4), device=x.device, dtype=torch.bfloat16)
        assert bool(e.isnan().all())
        g.buffers[-1].raw[MARGIN - 2:MARGIN] = 0
        with pytest.raises(AssertionError, match=r"front margin damaged, 2 bytes, offsets -2\.\.-1 relative to the tensor's start"):
            g.check()
