"""torch's CrossEntropyLoss arguments on fusion_gcn_amd.loss (fgcn_ce_fwd / fgcn_ce_bwd, include/fgcn.h): every
value against torch.nn.functional.cross_entropy on the CPU in float64 over the same float32 values cast up, at the bounds
tests/test_kernels_gpu.py::test_cross_entropy_matches_torch holds the plain loss to.  The cross-row sums are float64, so the bounds
do not loosen with the row count."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
REDUCTIONS = ("mean", "sum", "none")
# 16 rows per workgroup: (1000, 3) runs on 63 workgroups with 8 rows in the last, (517, 1030) on 33 with 5 in the last
SHAPES = [(1, 5), (2, 27), (7, 35), (64, 60), (130, 60), (16, 200), (1000, 3), (517, 1030)]
# (weight, label_smoothing, ignore_index)
OPTIONS = {"weight": (True, 0.0, -100), "smooth": (False, 0.1, -100), "weight_smooth": (True, 0.1, -100), "ignore2": (True, 0.1, 2),
           "smooth1": (False, 1.0, -100)}
# 8 shapes x 5 option sets, the reduction rotating: every option set runs in all three reductions, every shape too (40 cases)
INDEX_CASES = [(rows, classes, name, REDUCTIONS[(si + oi) % 3]) for si, (rows, classes) in enumerate(SHAPES)
               for oi, name in enumerate(OPTIONS)]


def close(got, want):
    return abs(got - want) < 2e-6 * max(1.0, abs(want))


@functools.lru_cache(maxsize=None)
def inputs(rows, classes, ignore_index=-100):
    """Seeded inputs, float32 values held in float64 (shared by the cases of a shape, never modified): logits = 3 * randn in a padded
    matrix (the loss sees the column window [:, :classes], row stride > classes), labels with ``ignore_index`` in two rows (rows 1
    and rows - 2; one row of a two-row batch, none of a single row: a batch of ignored rows only is an edge case below, not parity),
    weights in [0.1, 1.1] with one class at 0, softmax targets in a padded matrix whose row 0 sums to 0.6, an upstream vector."""
    g = torch.Generator().manual_seed(1000 * rows + classes)
    npad = classes // 4 * 4 + 4
    z = (torch.randn(rows, npad, generator=g) * 3).double()
    y = torch.randint(0, classes, (rows,), generator=g)
    if rows <= 2 and ignore_index >= 0:
        y[0] = (ignore_index + 1) % classes
    for i in ([1, rows - 2] if rows > 4 else [1] if rows == 2 else []):
        y[i] = ignore_index
    w = torch.rand(classes, generator=g) + 0.1
    w[classes // 2] = 0.0
    t = torch.zeros(rows, npad)
    t[:, :classes] = torch.softmax(torch.randn(rows, classes, generator=g) * 2, dim=1)
    t[0] *= 0.6
    up = torch.randn(rows, generator=g)
    return z, y, w.double(), t.double(), up.double()


def reference(z, target, classes, weight, ignore_index, reduction, eps, up):
    """float64 on the CPU -> (loss, d loss / d logits) of (loss * upstream).sum()"""
    zr = z[:, :classes].clone().requires_grad_(True)
    want = F.cross_entropy(zr, target, weight=weight, ignore_index=ignore_index, reduction=reduction, label_smoothing=eps)
    (want * (up if reduction == "none" else 1.7)).sum().backward()
    return want.detach(), zr.grad


def run(z, target, classes, weight, ignore_index, reduction, eps, up):
    from fusion_gcn_amd.loss import CrossEntropyLoss
    base = guarded.to(z.float(), DEV).requires_grad_(True)
    loss_fn = guarded.to(CrossEntropyLoss(None if weight is None else weight.float(), ignore_index, reduction, eps), DEV)
    got = loss_fn(base[:, :classes], target)
    (got * (guarded.to(up.float(), DEV) if reduction == "none" else 1.7)).sum().backward()
    torch.cuda.synchronize()
    return got.detach().cpu(), base.grad.cpu()


def compare(got, grad, want, want_grad, classes, reduction):
    if reduction == "none":
        assert got.shape == want.shape and got.dtype == torch.float32
        err = rel_l2(got.numpy(), want.numpy())
        print(f"row_loss rel_l2 {err:.3e}")
        assert err < 2e-6
    else:
        assert got.dim() == 0
        print(f"loss {float(got):.9g} want {float(want):.9g} err {abs(float(got) - float(want)) / max(1.0, abs(float(want))):.3e}")
        assert close(float(got), float(want))
    err = rel_l2(grad[:, :classes].numpy(), want_grad.numpy())
    print(f"grad rel_l2 {err:.3e}")
    assert err < 2e-6
    assert float(grad[:, classes:].abs().max()) == 0.0            # the pad columns of the matrix the logits are a window of


@pytest.mark.parametrize("rows,classes,name,reduction", INDEX_CASES)
def test_index_targets_match_torch(rows, classes, name, reduction):
    use_w, eps, ignore_index = OPTIONS[name]
    z, y, w, _, up = inputs(rows, classes, ignore_index)
    w = w if use_w else None
    want, want_grad = reference(z, y, classes, w, ignore_index, reduction, eps, up)
    got, grad = run(z, guarded.to(y, DEV), classes, w, ignore_index, reduction, eps, up)
    compare(got, grad, want, want_grad, classes, reduction)
    ignored = (y == ignore_index).nonzero().flatten()
    assert ignored.numel() >= min(2, rows - 1)
    assert float(grad[ignored].abs().max() if ignored.numel() else 0.0) == 0.0           # exactly 0, not small


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("use_w,eps", [(False, 0.0), (True, 0.0), (False, 0.1), (True, 0.1)])
@pytest.mark.parametrize("rows,classes", [(7, 35), (64, 60), (517, 1030)])
def test_probability_targets_match_torch(rows, classes, use_w, eps, reduction):
    z, _, w, t, up = inputs(rows, classes)
    w = w if use_w else None
    assert abs(float(t[0].sum()) - 0.6) < 1e-6 and abs(float(t[1].sum()) - 1.0) < 1e-6
    want, want_grad = reference(z, t[:, :classes], classes, w, -100, reduction, eps, up)
    got, grad = run(z, guarded.to(t.float(), DEV)[:, :classes], classes, w, -100, reduction, eps, up)       # a window: its own row stride
    compare(got, grad, want, want_grad, classes, reduction)


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_every_row_ignored_and_zero_weights(reduction):
    """A zero denominator: the mean is NaN as in torch, the sum 0, the vector zeros; the gradients are what torch gives (0 for an
    ignored row whatever the reduction; NaN under the mean for rows whose classes all weigh 0)."""
    rows, classes = 20, 7
    z, _, w, _, up = inputs(rows, classes)
    for y, weight, eps in ((torch.full((rows,), -100), None, 0.0), (torch.full((rows,), -100), w, 0.1),
                           (torch.tensor([classes // 2] * (rows - 1) + [-100]), w, 0.0),           # every present class at weight 0
                           (torch.tensor([classes // 2] * (rows - 1) + [-100]), w, 0.1)):
        want, want_grad = reference(z, y, classes, weight, -100, reduction, eps, up)
        got, grad = run(z, guarded.to(y, DEV), classes, weight, -100, reduction, eps, up)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isnan(grad[:, :classes]), torch.isnan(want_grad))
        if reduction == "mean":
            assert torch.isnan(got)
        elif eps == 0.0:
            assert float(got.abs().max()) == 0.0
        if reduction == "none":
            assert rel_l2(got.numpy(), want.numpy()) < 2e-6
        else:
            assert torch.isnan(got) or close(float(got), float(want))
        ignored = y == -100
        assert float(grad[ignored].abs().max()) == 0.0
        assert rel_l2(grad[:, :classes].nan_to_num(7.0).numpy(), want_grad.nan_to_num(7.0).numpy()) < 2e-6


@pytest.mark.parametrize("reduction", REDUCTIONS)
def test_invalid_label_is_nan_in_its_row(reduction):
    """A label outside [0, classes) that is not ignore_index (torch: a device assert): that row's loss and gradient are NaN, and so
    are the mean and the sum; with reduction none only that row."""
    rows, classes = 37, 11
    z, y, w, _, up = inputs(rows, classes)
    for bad_label in (classes, -1, 2 ** 40):
        bad = y.clone()
        bad[5] = bad_label
        got, grad = run(z, guarded.to(bad, DEV), classes, w, -100, reduction, 0.1, up)
        other = torch.arange(rows) != 5
        assert torch.isnan(grad[5, :classes]).all() and not torch.isnan(grad[other]).any() and float(grad[:, classes:].abs().max()) == 0.0
        if reduction == "none":
            assert torch.isnan(got[5]) and not torch.isnan(got[other]).any()
            want, _ = reference(z, y, classes, w, -100, reduction, 0.1, up)
            assert rel_l2(got[other].numpy(), want[other].numpy()) < 2e-6
        else:
            assert torch.isnan(got)


@pytest.mark.parametrize("rows,classes", [(64, 60), (130, 60)])
def test_default_arguments_are_the_plain_path(rows, classes):
    """CrossEntropyLoss() and CrossEntropyLoss(None, -100, "mean", 0.0) ARE block.cross_entropy (the plain kernels), bit for bit;
    the options kernels with neutral options forced (weight = ones) agree with it to the tolerance of the parity tests."""
    from fusion_gcn_amd import block
    from fusion_gcn_amd.loss import CrossEntropyLoss, cross_entropy
    z, y, _, _, _ = inputs(rows, classes)
    y = guarded.to(y, DEV)

    def both(fn):
        base = guarded.to(z.float(), DEV).requires_grad_(True)
        loss = fn(base[:, :classes], y)
        (loss * 1.7).backward()
        return loss.detach(), base.grad

    want, want_grad = both(block.cross_entropy)
    for fn in (CrossEntropyLoss(), CrossEntropyLoss(None, -100, "mean", 0.0), cross_entropy,
               lambda a, b: cross_entropy(a, b, None, -100, "mean", 0.0)):
        got, grad = both(fn)
        assert torch.equal(got, want) and torch.equal(grad, want_grad)
    got, grad = both(guarded.to(CrossEntropyLoss(weight=torch.ones(classes)), DEV))
    assert close(float(got), float(want)) and rel_l2(grad.cpu().numpy(), want_grad.cpu().numpy()) < 2e-6
    assert float(grad[:, classes:].abs().max()) == 0.0


def test_two_runs_leave_the_same_bits():
    """(517, 1030) with weight and label_smoothing 0.1: 33 workgroups' partials, added in index order."""
    from fusion_gcn_amd import ops
    rows, classes = 517, 1030
    z, y, w, _, _ = inputs(rows, classes)
    zd, yd, wd = guarded.to(z.float(), DEV)[:, :classes], guarded.to(y, DEV), guarded.to(w.float(), DEV)
    runs = []
    for _ in range(2):
        loss, row_loss, row_scale, probs = ops.cross_entropy_opts_fwd(zd, yd, wd, label_smoothing=0.1)
        grad = ops.cross_entropy_opts_bwd(probs, yd, wd, row_scale, loss, torch.full((1,), 1.7, device=DEV), label_smoothing=0.1)
        runs.append((loss, row_loss, grad))
        torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert not torch.isnan(runs[0][2]).any() and float(runs[0][0][1]) > 0


def test_forward_without_autograd_returns_the_same_bits():
    """Under torch.no_grad() (validation) the softmax is not stored; the loss is the one the training forward returns."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.loss import CrossEntropyLoss
    rows, classes = 64, 60
    z, y, w, _, _ = inputs(rows, classes)
    yd = guarded.to(y, DEV)
    for reduction in REDUCTIONS:
        loss_fn = guarded.to(CrossEntropyLoss(w.float(), reduction=reduction, label_smoothing=0.1), DEV)
        base = guarded.to(z.float(), DEV).requires_grad_(True)
        with_grad = loss_fn(base[:, :classes], yd)
        assert with_grad.requires_grad
        with torch.no_grad():
            without = loss_fn(base[:, :classes], yd)
        assert not without.requires_grad and torch.equal(without, with_grad.detach())
    assert ops.cross_entropy_opts_fwd(base.detach()[:, :classes], yd, need_probs=False)[3] is None


def test_graph_step_replays_a_loss_with_options():
    """GraphStep records the step with CrossEntropyLoss(weight=, label_smoothing=) once and replays it for other labels: every
    replay is the eager step at the bounds of GraphStep's own verification (loss 1e-6, flat gradient 1e-5 rel-L2)."""
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.loss import CrossEntropyLoss, balanced_class_weights
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.session.procedures import GraphStep
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    shape, classes, clips = (1, 16, 20, 3), 27, 4
    model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
    filler.fill_state_dict(model.state_dict())
    model = guarded.to(model, DEV).train()
    twin = copy.deepcopy(model)
    g = torch.Generator().manual_seed(11)
    x = guarded.to(torch.randn(clips, *shape, generator=g), DEV)
    w = balanced_class_weights(torch.randint(0, classes, (200,), generator=g), classes) + 0.05
    loss_fn = guarded.to(CrossEntropyLoss(weight=w, label_smoothing=0.1), DEV)
    step = GraphStep()
    for k in range(3):
        y = guarded.to(torch.randint(0, classes, (clips,), generator=g), DEV)
        model.zero_grad()
        _, loss = step.forward(model, loss_fn, x, y)
        step.backward(loss)
        torch.cuda.synchronize()
        got = torch.cat([v.reshape(-1) for v in step.grads.views]).clone()
        twin.zero_grad()
        want_loss = loss_fn(twin(x), y)
        want_loss.backward()
        want = torch.cat([p.grad.reshape(-1) for p in twin.parameters()])
        assert abs(float(loss) - float(want_loss.detach())) <= 1e-6 * abs(float(want_loss.detach())), k
        assert rel_l2(got.cpu().numpy(), want.cpu().numpy()) < 1e-5, k
    assert step.replays == 3 and len(step._recorded) == 1
