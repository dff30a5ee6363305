"""fusion_gcn_amd.metrics on the device: the golden streams of tests/golden/metrics.npz through ``fgcn_classify_update``, the
kernel's stated rules on constructed rows with guard words around everything it may write, the prediction store, strided logits,
the container inside ``Session.train_epoch`` / ``validate_epoch`` with ``GraphStep``, and the no-host-wait contract of
``update_*`` + ``format_*``."""
import threading

import numpy as np
import pytest
import torch

import metrics_golden as MG
from fusion_gcn_amd import _lib
from fusion_gcn_amd import metrics as M

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def d():
    return MG.load()


def _dev(batch):
    z, y, loss, idx = batch
    return guarded.to(torch.from_numpy(z), DEV), guarded.to(torch.from_numpy(y), DEV), guarded.to(torch.tensor(float(loss), dtype=torch.float32), DEV), torch.from_numpy(idx)


def _feed(container, d, s, step):
    for ctx, update in (("train", container.update_training), ("val", container.update_validation)):
        z, y, loss, idx = _dev(MG.batches(d, s, ctx)[step])
        update(loss, (z, y), None, idx)


def _assert_state(container, d, s, step):
    for ctx, long in MG.CONTEXTS:
        snap, want = container.state_snapshot(ctx), MG.expected_state(d, s, step, long)
        assert (snap["counts"] == want["counts"]).all(), (s, step, ctx, snap["counts"], want["counts"])
        assert (snap["confusion"] == want["confusion"]).all(), (s, step, ctx)
        assert abs(snap["loss_sum"] - want["loss_sum"]) <= 1e-12 * abs(want["loss_sum"])


@pytest.mark.parametrize("s", MG.STREAMS)
def test_golden_streams_through_the_kernel(d, s):
    classes, k, rows = MG.spec(d, s)
    first, second = MG.build_container(classes, k), MG.build_container(classes, k)
    for step in range(len(rows)):
        _feed(first, d, s, step)
        _assert_state(first, d, s, step)
        MG.check_values(first, d, s, step, k)            # loss mean, every ratio, MisclassifiedSamplesList.value
        torch.cuda.synchronize()
        for which in ("training", "validation", "all"):   # everything has arrived: the progress line is the reference's
            assert getattr(first, f"format_{which}")() == str(d[f"{s}_step{step}_format_{which}"])
    for step in range(len(rows)):
        _feed(second, d, s, step)
    for ctx, _ in MG.CONTEXTS:                            # a second container fed the same stream: bit-identical state
        torch.cuda.synchronize()
        a, b = first._states[ctx].dev.cpu().numpy(), second._states[ctx].dev.cpu().numpy()
        assert a.tobytes() == b.tobytes()
    first.reset_all()
    assert first.get_value_history()["training_accuracy"] == [float(d[f"{s}_step{len(rows) - 1}_training_accuracy"])]
    assert int(first._states["train"].dev.abs().sum()) == 0
    _feed(first, d, s, 0)                                 # and the next epoch starts from zero
    _assert_state(first, d, s, 0)


def _guarded_state(classes):
    from fusion_gcn_amd import ops
    words = ops.classify_state_bytes(classes) // 8
    buf = torch.full((words + 32,), GUARD, dtype=torch.int64, device=DEV)
    buf[16:16 + words] = 0
    return buf, buf[16:16 + words], words


def _guards_intact(buf, words):
    host = buf.cpu().numpy()
    return (host[:16] == GUARD).all() and (host[16 + words:] == GUARD).all()


def _parse(state, classes):
    raw = state.cpu().numpy()
    return raw[:7], raw[7:8].view(np.float64)[0], raw[8:].view(np.int32)[:classes * classes].reshape(classes, classes)


def test_stated_rules_on_constructed_rows():
    from fusion_gcn_amd import ops
    nan, classes, k = float("nan"), 6, 2
    tied, with_nan = [1., 5., 5., 2., 5., 0.], [1., 2., 3., nan, 9., nan]
    rows = [(tied, 2),            # maximum at 1, 2 and 4: pred = 1 (the first); one equal logit below the label: rank 1 < k
            (tied, 4),            # two equal logits below the label: rank 2, NOT a hit -- the tie at the k boundary
            (with_nan, 4),        # a NaN is the maximum (pred = 3, the first NaN) and ranks above every number: rank 2
            (with_nan, 5),        # the label's logit is NaN: only the NaN below it ranks above: rank 1
            ([9., 0., 0., 0., 0., 1.], -100),
            ([9., 0., 0., 0., 0., 1.], classes), ([9., 0., 0., 0., 0., 1.], -1), ([9., 0., 0., 0., 0., 1.], 2 ** 40),
            ([0., 1., 2., 3., 4., 5.], 5)]
    z = torch.tensor([r for r, _ in rows], dtype=torch.float32, device=DEV)
    y = torch.tensor([lab for _, lab in rows], dtype=torch.int64, device=DEV)
    want_pred = [1, 1, 3, 3, -1, -1, -1, -1, 5]
    assert torch.argmax(z, dim=1).tolist() == [1, 1, 3, 3, 0, 0, 0, 0, 5]          # torch's rule, at test time
    buf, state, words = _guarded_state(classes)
    pred_buf = torch.full((len(rows) + 8,), -7, dtype=torch.int32, device=DEV)
    loss = torch.tensor(0.75, device=DEV)
    for call in range(2):
        ops.classify_update(z, y, state, k=k, loss=loss, pred_out=pred_buf[:len(rows)])
        counts, loss_sum, confusion = _parse(state, classes)
        n = call + 1
        assert counts.tolist() == [5 * n, 1 * n, 3 * n, 1 * n, 3 * n, 0, len(rows) * n], counts
        assert loss_sum == 0.75 * len(rows) * n
        want = np.zeros((classes, classes), np.int32)
        for lab, p in ((2, 1), (4, 1), (4, 3), (5, 3), (5, 5)):
            want[lab, p] = n
        assert (confusion == want).all()                  # untouched by the ignored and the invalid rows
        assert pred_buf.tolist() == want_pred + [-7] * 8
        assert _guards_intact(buf, words)
    # k = 1: a top-k hit is pred == label, ties and NaN included
    buf, state, words = _guarded_state(classes)
    ops.classify_update(z, y, state, k=1)
    counts, loss_sum, _ = _parse(state, classes)
    assert counts.tolist() == [5, 1, 1, 1, 3, 0, 0] and loss_sum == 0.0 and _guards_intact(buf, words)
    # the wrapper refuses what the kernel could not take
    with pytest.raises(_lib.FgcnError, match="state"):
        ops.classify_update(z, y, state[:-1], k=1)
    with pytest.raises(_lib.FgcnError, match="bad k"):
        ops.classify_update(z, y, state, k=classes + 1)
    with pytest.raises(_lib.FgcnError):
        ops.classify_update(z.cpu(), y.cpu(), state, k=1)


def test_pred_out_capacity_and_strided_logits(d):
    from fusion_gcn_amd import ops
    s = "a27"
    classes, k, rows = MG.spec(d, s)
    total, cap = sum(rows), 10
    buf, state, words = _guarded_state(classes)
    pred_buf = torch.full((cap + 8,), -7, dtype=torch.int32, device=DEV)
    offset = 0
    for z, y, loss, idx in map(_dev, MG.batches(d, s, "train")):
        padded = torch.full((z.shape[0], 64), 1e30, device=DEV)          # ld = 64 > classes: the padding must never be read as a class
        padded[:, :classes] = z
        view = padded[:, :classes]
        assert view.stride(0) == 64
        ops.classify_update(view, y, state, k=k, loss=loss, pred_out=pred_buf[:cap], pred_offset=offset)
        offset += z.shape[0]
    counts, loss_sum, confusion = _parse(state, classes)
    want = MG.expected_state(d, s, len(rows) - 1, "training")
    want["counts"][_lib.CLS_DROPPED] = total - cap
    assert (counts == want["counts"]).all() and (confusion == want["confusion"]).all()
    assert abs(loss_sum - want["loss_sum"]) <= 1e-12 * abs(want["loss_sum"])
    argmax = d[f"{s}_train_logits"].astype(np.float32).argmax(axis=1)
    assert pred_buf.tolist() == argmax[:cap].tolist() + [-7] * 8 and _guards_intact(buf, words)
    # the same through the container: the stored prefix, the rest counted as dropped
    container = MG.build_container(classes, k, capacity=cap)
    for step in range(len(rows)):
        _feed(container, d, s, step)
    lst = container["training_misclassified"]
    assert lst.dropped == total - cap
    idx, lab = d[f"{s}_train_indices"][:cap], d[f"{s}_train_labels"][:cap]
    wrong = argmax[:cap] != lab
    assert lst.value == sorted(zip(idx[wrong].tolist(), argmax[:cap][wrong].tolist(), lab[wrong].tolist()))
    assert float(container["training_accuracy"].value) == float(d[f"{s}_step{len(rows) - 1}_training_accuracy"])


# ---- in the loop --------------------------------------------------------------------------------------------------------------------
def _agcn(shape, classes):
    from oracle import filler
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    model = Model(shape, classes, Graph(utd.skeleton_edges, center_joint=utd.center_joint))
    filler.fill_state_dict(model.state_dict())
    return guarded.to(model, DEV)


def _batches(sizes, shape, classes, seed=5):
    g = torch.Generator().manual_seed(seed)
    out, first = [], 0
    for n in sizes:
        out.append((guarded.to(torch.randn(n, *shape, generator=g), DEV), guarded.to(torch.randint(0, classes, (n,), generator=g), DEV), first + torch.arange(n)))
        first += n
    return out


class _Hooked:
    """The container behind the test's own hook: keeps what every update was handed."""

    def __init__(self, container):
        self.container, self.seen = container, {"train": [], "val": []}

    def update_training(self, loss, pair, model, indices):
        self.seen["train"].append((loss.detach().clone(), pair[0].detach().clone(), pair[1].clone(), indices.clone()))
        self.container.update_training(loss, pair, model, indices)

    def update_validation(self, loss, pair, model, indices):
        self.seen["val"].append((loss.detach().clone(), pair[0].detach().clone(), pair[1].clone(), indices.clone()))
        self.container.update_validation(loss, pair, model, indices)

    def format_training(self):
        return self.container.format_training()

    def format_all(self):
        return self.container.format_all()


def _after_the_fact(seen, classes, k):
    """Plain torch, float64, from the captured per-batch logits and losses (the reference's formulas)."""
    z = torch.cat([s[1] for s in seen]).double().cpu()
    y = torch.cat([s[2] for s in seen]).cpu()
    idx = torch.cat([s[3] for s in seen])
    pred = z.argmax(dim=1)
    n = sum(len(s[2]) for s in seen)
    loss = sum(float(s[0].double()) * len(s[2]) for s in seen) / n
    top = (torch.topk(z, k, dim=1)[1] == y[:, None]).any(dim=1).double().mean().item()
    cm = torch.bincount(classes * y + pred, minlength=classes ** 2).reshape(classes, classes)
    wrong = sorted((int(i), int(p), int(t)) for i, p, t in zip(idx, pred, y) if p != t)
    return {"loss": loss, "accuracy": (pred == y).double().mean().item(), f"top{k}_accuracy": top, "confusion": cm.numpy(), "wrong": wrong}


def _assert_epoch(container, seen, long, classes, k):
    want = _after_the_fact(seen, classes, k)
    for name in ("loss", "accuracy", f"top{k}_accuracy"):
        got = container[f"{long}_{name}"].value
        assert abs(got - want[name]) <= 1e-12 * abs(want[name]), (long, name, got, want[name])
    assert (container[f"{long}_confusion"].value.numpy() == want["confusion"]).all()
    assert container[f"{long}_misclassified"].value == want["wrong"]


def test_container_in_the_session_loops():
    from fusion_gcn_amd.loss import CrossEntropyLoss
    from fusion_gcn_amd.optim import FlatOptimizer
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, GradientAccumulationBatchProcessor, GraphStep
    from fusion_gcn_amd.session.session import Session
    shape, classes, k = (1, 24, 20, 3), 27, 5
    data = _batches([4, 4, 4, 3], shape, classes)
    model = _agcn(shape, classes)
    opt = FlatOptimizer(model.parameters(), "SGD", 0.01, momentum=0.9)
    loss_fn = CrossEntropyLoss()
    step = GraphStep()
    hooked = _Hooked(MG.build_container(classes, k))
    lines = []

    class Progress:
        def update_epoch_mode(self, mode, metrics=None):
            lines.append(metrics)
    Session.train_epoch(DefaultBatchProcessor(step), model, loss_fn, data, opt, Progress(), hooked)
    assert step.replays == 4 and len(hooked.seen["train"]) == 4 and len(lines) == 4
    assert all(line.startswith("training_loss: ") for line in lines)
    _assert_epoch(hooked.container, hooked.seen["train"], "training", classes, k)
    Session.validate_epoch(DefaultBatchProcessor(step), model, loss_fn, data[:3], Progress(), hooked)
    assert len(hooked.seen["val"]) == 3 and lines[-1].startswith("training_loss: ") and "validation_loss: " in lines[-1]
    _assert_epoch(hooked.container, hooked.seen["val"], "validation", classes, k)
    _assert_epoch(hooked.container, hooked.seen["train"], "training", classes, k)        # untouched by the validation updates
    torch.cuda.synchronize()
    want = _after_the_fact(hooked.seen["train"], classes, k)
    assert hooked.container.format_training().startswith(f"training_loss: {want['loss']:.4f}, training_accuracy: {want['accuracy']:.4f}")
    # gradient accumulation: every micro-batch's loss arrives divided by its size and is weighted with its rows, as in the reference
    hooked.container.reset_all()
    hooked.seen = {"train": [], "val": []}
    data = _batches([4, 4], shape, classes, seed=9)
    Session.train_epoch(GradientAccumulationBatchProcessor(step, 4, 2), model, loss_fn, data, opt, None, hooked)
    seen = hooked.seen["train"]
    assert len(seen) == 4 and all(len(s[2]) == 2 for s in seen)
    _assert_epoch(hooked.container, seen, "training", classes, k)
    for loss, z, y, _ in seen:
        ce = torch.nn.functional.cross_entropy(z.double(), y).item()
        assert abs(float(loss) - ce / 2) <= 1e-5 * ce
    mean_ce = sum(torch.nn.functional.cross_entropy(s[1].double(), s[2]).item() for s in seen) / 4
    assert abs(hooked.container["training_loss"].value - mean_ce / 2) <= 1e-5 * mean_ce


def test_update_and_format_never_wait_for_the_device(d):
    """``torch.cuda.set_sync_debug_mode("error")`` makes torch raise on every synchronising call it knows of; it is checked first that
    this torch build honours it (an ``.item()`` must raise).  Independently of it: the progress line comes back while a long
    kernel queue enqueued BEFORE the updates is still running, and shows zeros, the values of the newest snapshot that has arrived."""
    s = "b60"
    classes, k, rows = MG.spec(d, s)
    container = MG.build_container(classes, k, snapshot_every=2)
    staged = [_dev(b) for b in MG.batches(d, s, "train")]
    a = torch.randn(8192, 8192, device=DEV)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            probe.item()
        except RuntimeError:
            honoured = True
        for _ in range(60):                               # >= 60 * 1.1 TFLOP of float32 GEMM in front of the updates
            a @ a
        busy = torch.cuda.Event()
        busy.record()
        lines = []
        for z, y, loss, idx in staged:
            container.update_training(loss, (z, y), None, idx)
            lines.append(container.format_training())
        still_running = not busy.query()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert honoured, "this torch build does not raise on .item() under set_sync_debug_mode('error')"
    assert still_running, "the GEMM queue finished before the host came back: the check shows nothing"
    assert all(line.startswith("training_loss: 0.0000, training_accuracy: 0.0000") for line in lines), lines
    last = len(rows) - 1
    assert container["training_accuracy"].value == float(d[f"{s}_step{last}_training_accuracy"])      # .value waits
    assert container.format_training() == str(d[f"{s}_step{last}_format_training"])
    # snapshot_every = 2: of the three updates only the second enqueued a copy; the value above came from the waiting path
    state = container._states["train"]
    assert state.seq == 3 and state.snap_seq == 2


def test_two_containers_on_two_streams_and_threads(d):
    s = "b60"
    classes, k, rows = MG.spec(d, s)
    staged = {ctx: [_dev(b) for b in MG.batches(d, s, ctx)] for ctx, _ in MG.CONTEXTS}
    torch.cuda.synchronize()
    containers = [MG.build_container(classes, k) for _ in range(2)]
    errors = []

    def run(container):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                for _ in range(3):                        # three epochs each, reset in between
                    container.reset_all(save_history=False)
                    for step in range(len(rows)):
                        for ctx, update in (("train", container.update_training), ("val", container.update_validation)):
                            z, y, loss, idx = staged[ctx][step]
                            update(loss, (z, y), None, idx)
                stream.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=run, args=(c,)) for c in containers]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for container in containers:
        _assert_state(container, d, s, len(rows) - 1)
        MG.check_values(container, d, s, len(rows) - 1, k)
