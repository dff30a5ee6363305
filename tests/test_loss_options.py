"""torch's CrossEntropyLoss arguments on fusion_gcn_amd.loss, the part that needs no GPU: what the constructor and the functional
form accept and refuse, the weight buffer, the host-side argument checks of fgcn_ce_fwd / fgcn_ce_bwd (they precede any launch),
the workspace query and the class-weight helper.  The values are in tests/test_loss_options_gpu.py."""
import ctypes as C
import math

import pytest
import torch

from fusion_gcn_amd import _lib, build
from fusion_gcn_amd.loss import CrossEntropyLoss, balanced_class_weights, cross_entropy


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_constructor_takes_torchs_arguments():
    """(`CrossEntropyLoss(label_smoothing=0.1)` was a TypeError before the options existed.)"""
    loss = CrossEntropyLoss(label_smoothing=0.1)
    assert (loss.weight, loss.ignore_index, loss.reduction, loss.label_smoothing) == (None, -100, "mean", 0.1)
    w = torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)
    loss = CrossEntropyLoss(w, 2, "sum", 1.0)                      # torch's positional order
    assert loss.weight.dtype == torch.float32 and loss.weight.tolist() == [0.5, 2.0, 1.0]
    assert (loss.ignore_index, loss.reduction, loss.label_smoothing) == (2, "sum", 1.0)
    assert CrossEntropyLoss(reduction="none", label_smoothing=0).reduction == "none"
    plain = CrossEntropyLoss()
    assert (plain.weight, plain.ignore_index, plain.reduction, plain.label_smoothing) == (None, -100, "mean", 0.0)


def test_weight_is_a_buffer():
    w = torch.tensor([0.25, 4.0])
    loss = CrossEntropyLoss(weight=w)
    assert list(loss.state_dict()) == ["weight"] and torch.equal(loss.state_dict()["weight"], w)
    assert dict(loss.named_buffers())["weight"] is loss.weight and not list(loss.parameters())
    assert loss.to(torch.float64).weight.dtype == torch.float64      # it moves with .to(), as a buffer does
    other = CrossEntropyLoss(weight=torch.ones(2))
    other.load_state_dict(loss.state_dict())
    assert other.weight.tolist() == [0.25, 4.0]
    assert list(CrossEntropyLoss().state_dict()) == []


@pytest.mark.parametrize("eps", [-0.01, 1.01, float("nan"), float("inf")])
def test_label_smoothing_outside_the_unit_interval(eps):
    with pytest.raises(ValueError, match="label_smoothing"):
        CrossEntropyLoss(label_smoothing=eps)
    with pytest.raises(ValueError, match="label_smoothing"):
        cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), label_smoothing=eps)


def test_errors_that_need_no_gpu():
    z, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    for bad in ("Mean", "batchmean", "", None):
        with pytest.raises(ValueError, match="reduction"):
            CrossEntropyLoss(reduction=bad)
        with pytest.raises(ValueError, match="reduction"):
            cross_entropy(z, y, reduction=bad)
    for bad in (torch.ones(3, 1), torch.ones(()), torch.ones(3, dtype=torch.int64), [1.0, 1.0, 1.0]):
        with pytest.raises(ValueError, match="weight"):
            CrossEntropyLoss(weight=bad)
        with pytest.raises(ValueError, match="weight"):
            cross_entropy(z, y, weight=bad)
    with pytest.raises(ValueError, match="weight"):                  # one entry per class: known at the call
        CrossEntropyLoss(weight=torch.ones(4))(z, y)
    with pytest.raises(ValueError, match="weight"):
        cross_entropy(z, y, torch.ones(2))
    with pytest.raises(ValueError, match="ignore_index"):            # class probabilities have no row to ignore
        cross_entropy(z, torch.full((4, 3), 1 / 3), ignore_index=1)
    with pytest.raises(ValueError, match="ignore_index"):
        CrossEntropyLoss(ignore_index=0)(z, torch.full((4, 3), 1 / 3))
    for name in ("size_average", "reduce"):                          # deprecated in torch, not built
        with pytest.raises(TypeError):
            CrossEntropyLoss(**{name: True})
        with pytest.raises(TypeError):
            cross_entropy(z, y, **{name: True})


def test_options_have_no_fallback():
    """Without a GPU a forward with options raises, like every other libfgcn path: nothing is computed by torch instead."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    z, y = torch.randn(4, 3, requires_grad=True), torch.tensor([0, 1, 2, 1])
    for loss in (CrossEntropyLoss(label_smoothing=0.1), CrossEntropyLoss(weight=torch.ones(3)), CrossEntropyLoss(reduction="none"),
                 CrossEntropyLoss(ignore_index=1), CrossEntropyLoss()):
        with pytest.raises(_lib.FgcnError):
            loss(z, y)
    with pytest.raises(_lib.FgcnError):
        cross_entropy(z, torch.full((4, 3), 1 / 3))
    from fusion_gcn_amd import ops
    with pytest.raises(_lib.FgcnError):
        ops.cross_entropy_opts_fwd(z.detach(), y, label_smoothing=0.1)
    with pytest.raises(_lib.FgcnError):
        ops.cross_entropy_opts_bwd(torch.zeros(4, 3), y, None, torch.zeros(4), torch.zeros(2), torch.zeros(1))


def test_workspace_bytes(lib):
    assert lib.fgcn_ce_workspace_bytes(0) == 0 and lib.fgcn_ce_workspace_bytes(-5) == 0
    sizes = [lib.fgcn_ce_workspace_bytes(r) for r in (1, 16, 17, 64, 517, 4096)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)       # float64 pairs, more rows never need fewer
    assert sizes[0] == sizes[1] < sizes[2]                                            # a fixed number of rows per workgroup


def test_host_side_validation(lib):
    """Every bad argument of include/fgcn.h's list is FGCN_E_BADARG before any launch (no device is touched: this runs without one)."""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    MEAN, SUM, NONE = (_lib.CE_REDUCTIONS[k] for k in ("mean", "sum", "none"))
    assert (MEAN, SUM, NONE) == (0, 1, 2)

    def fwd(logits=p, labels=p, target=None, weight=None, probs=p, row_loss=p, row_scale=p, loss=p, work=p, rows=4, classes=3, ld=4,
            ld_t=0, ignore=-100, eps=0.0, red=MEAN):
        return lib.fgcn_ce_fwd(logits, labels, target, weight, probs, row_loss, row_scale, loss, work, rows, classes, ld, ld_t, ignore,
                               eps, red, None)

    def bwd(probs=p, labels=p, target=None, weight=None, row_scale=p, loss=p, dloss=p, dlogits=p, rows=4, classes=3, ld_t=0, ld_out=4,
            ignore=-100, eps=0.0, red=MEAN):
        return lib.fgcn_ce_bwd(probs, labels, target, weight, row_scale, loss, dloss, dlogits, rows, classes, ld_t, ld_out, ignore, eps,
                               red, None)

    for name in ("logits", "row_loss", "row_scale", "loss", "work"):                 # (probs may be NULL: no backward follows)
        assert fwd(**{name: None}) == -1, name
        assert b"null pointer" in lib.fgcn_last_error()
    for name in ("probs", "row_scale", "loss", "dloss", "dlogits"):
        assert bwd(**{name: None}) == -1, name
    for call in (fwd, bwd):
        assert call(labels=None) == -1 and b"exactly one" in lib.fgcn_last_error()                 # neither
        assert call(target=p, ld_t=3) == -1 and b"exactly one" in lib.fgcn_last_error()            # both
        assert call(rows=0) == -1 and call(rows=-1) == -1 and call(classes=0) == -1 and call(classes=-3) == -1
        assert call(labels=None, target=p, ld_t=2) == -1                                           # the target's row stride < classes
        for eps in (-0.1, 1.5, math.nan, math.inf):
            assert call(eps=eps) == -1 and b"label_smoothing" in lib.fgcn_last_error()
        for red in (-1, 3, 7):
            assert call(red=red) == -1 and b"reduction" in lib.fgcn_last_error()
    assert fwd(ld=2) == -1 and bwd(ld_out=2) == -1
    assert fwd(work=p + 4) == -2 and b"aligned" in lib.fgcn_last_error()


def test_balanced_class_weights():
    # n = 8 samples, C = 4 classes, counts (4, 1, 0, 3): n / (C count) = 0.5, 2, (empty: 0), 2 / 3
    w = balanced_class_weights([0, 3, 0, 1, 3, 0, 3, 0], 4)
    assert w.dtype == torch.float32 and w.shape == (4,)
    assert w.tolist() == pytest.approx([0.5, 2.0, 0.0, 2.0 / 3.0], rel=1e-7)
    import numpy as np
    assert torch.equal(balanced_class_weights(np.array([0, 3, 0, 1, 3, 0, 3, 0], dtype=np.int32), 4), w)     # what labels_data is
    assert torch.equal(balanced_class_weights(torch.tensor([[1, 1], [1, 1]]), 2), torch.tensor([0.0, 0.5]))
    assert balanced_class_weights([], 3).tolist() == [0.0, 0.0, 0.0]
    for bad in ([0, 4], [-1, 0]):
        with pytest.raises(ValueError):
            balanced_class_weights(bad, 4)
    # a balanced set weighs every class 1: the weighted mean is the plain mean
    assert balanced_class_weights([0, 1, 2, 0, 1, 2], 3).tolist() == [1.0, 1.0, 1.0]
