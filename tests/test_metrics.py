"""fusion_gcn_amd.metrics without a device: every derived value against the values the reference's own classes reported
(tests/golden/metrics.npz, tools/gen_golden_metrics.py), the container's behaviour, the C ABI's host-side validation, the
data-parallel sum over gloo."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import metrics_golden as MG
from conftest import ROOT
from fusion_gcn_amd import _lib, build
from fusion_gcn_amd import metrics as M


@pytest.fixture(scope="module")
def d():
    return MG.load()


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _install(container, d, s, step):
    rows = MG.spec(d, s)[2]
    for ctx, long in MG.CONTEXTS:
        arrays = MG.expected_state(d, s, step, long)
        arrays["indices"], arrays["pred"], arrays["labels"] = MG.reference_predictions(d, s, ctx, sum(rows[:step + 1]))
        container.load_state(ctx, arrays)


def test_golden_inputs_have_no_ties(d):
    for s in MG.STREAMS:
        for ctx, _ in MG.CONTEXTS:
            z = d[f"{s}_{ctx}_logits"].astype(np.float32)
            assert all(len(set(row.tolist())) == z.shape[1] for row in z)
    assert MG.spec(d, "a27") == (27, 5, [8, 8, 5]) and MG.spec(d, "b60") == (60, 5, [64, 64, 64]) and MG.spec(d, "c5")[:2] == (5, 5)


@pytest.mark.parametrize("s", MG.STREAMS)
def test_derived_values_match_the_reference(d, s):
    classes, k, rows = MG.spec(d, s)
    container = MG.build_container(classes, k)
    for step in range(len(rows)):
        _install(container, d, s, step)
        MG.check_values(container, d, s, step, k)
        for which in ("training", "validation", "all"):
            assert getattr(container, f"format_{which}")() == str(d[f"{s}_step{step}_format_{which}"]), (s, step, which)
        snap = container.state_snapshot("val")
        want = MG.expected_state(d, s, step, "validation")
        assert (snap["counts"] == want["counts"]).all() and (snap["confusion"] == want["confusion"]).all()
        assert snap["counts"].dtype == np.int64 and snap["confusion"].dtype == np.int32 and snap["loss_sum"] == want["loss_sum"]


def test_history_and_reset(d):
    s = "a27"
    classes, k, rows = MG.spec(d, s)
    container = MG.build_container(classes, k)
    for epoch in range(2):
        _install(container, d, s, len(rows) - 1)
        container.reset_all(save_history=True)
    history = container.get_value_history()
    assert set(history) == {m.name for m in container.get_metrics()}
    for name, values in history.items():
        assert len(values) == 2
        key = f"{s}_history_{name}"
        if key in d.files:
            assert abs(values[0] - float(d[key][0])) <= 1e-12 * abs(float(d[key][0])) and values[1] == values[0], name
    # after the reset: empty again -- progress lines show zeros, values divide by zero as the reference's do
    assert container.format_training().startswith("training_loss: 0.0000, training_accuracy: 0.0000")
    with pytest.raises(ZeroDivisionError):
        container["training_accuracy"].value
    assert int(container["training_confusion"].value.sum()) == 0 and container["training_misclassified"].value == []
    container.reset_all(save_history=False)
    assert all(len(v) == 2 for v in history.values())
    # the consistency assertion: a metric that joins the history late
    container._metrics_dict["late"] = M.SimpleMetric("late")
    _install(container, d, s, 0)
    with pytest.raises(AssertionError, match="Inconsistency in history length"):
        container.reset_all(save_history=True)
    with pytest.raises(RuntimeError, match="reset_all"):
        container["training_accuracy"].reset()


class _Probe(M.Metric):
    def __init__(self, name):
        super().__init__(name)
        self.calls = []

    def update(self, val=None, **kwargs):
        self.calls.append((val, kwargs))

    @property
    def value(self):
        return len(self.calls)

    def reset(self):
        self.calls = []

    def _to_summary(self, summary, epoch):
        summary.add_scalar(self.name, self.value, epoch)


class _HostMean(M.ScalarMetric):
    """A user's loss metric: receives (loss, num_items=)."""

    def __init__(self, name):
        super().__init__(name)
        self.seen = []

    def update(self, val=None, **kwargs):
        self.seen.append((val, kwargs))

    @property
    def value(self):
        return float(len(self.seen))

    def reset(self):
        self.seen = []


def test_split_by_name_and_pass_through():
    probe_t, probe_v, both, neither = _Probe("train_probe"), _Probe("val_probe"), _Probe("train_val_probe"), _Probe("other")
    lr, loss_t = M.SimpleMetric("lr"), _HostMean("training_loss")
    bars = M.AccuracyBarChart(4, "train_val_diff")
    container = M.MetricsContainer([loss_t, M.Mean("validation_loss"), M.MultiClassAccuracy("validation_accuracy"), probe_t, probe_v,
                                    both, neither, lr, bars])
    assert container.training_loss is loss_t and container.validation_loss.name == "validation_loss"
    assert container._training_metrics == [probe_t, both, bars] and container._validation_metrics[1:] == [probe_v, both, bars]
    assert container["lr"] is lr and container.get_metrics()[0] is loss_t
    model, indices, out = object(), torch.arange(3), (torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))
    # no state-backed TRAINING metric other than the bar chart would be touched by a host-only update; with it a launch is due
    with pytest.raises(_lib.FgcnError):
        container.update_training(torch.tensor(0.5), out, model, indices)
    plain = M.MetricsContainer([loss_t, probe_t, both, neither, lr])
    loss_t.reset()
    plain.update_training(torch.tensor(0.5), out, model, indices)
    assert loss_t.seen == [(torch.tensor(0.5), {"num_items": 3})]
    (val, kw), = probe_t.calls
    assert val is out and kw == {"context": "train", "model": model, "indices": indices}
    assert len(both.calls) == 1 and not neither.calls and not probe_v.calls
    plain.update_validation(torch.tensor(0.5), out, model, indices)
    assert both.calls[1][1]["context"] == "val"
    lr.update(0.1)
    assert plain.format_all() == "training_loss: 1.0000, lr: 0.1000" and plain.format_training() == "training_loss: 1.0000"
    # bar chart: both contexts' per-class accuracy, NaN for a class without samples
    cm = np.array([[2, 1, 0, 0], [0, 3, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1]], np.int32)
    counts = np.zeros(7, np.int64)
    counts[0], counts[1] = cm.sum(), np.trace(cm)
    container.load_state("train", {"counts": counts, "loss_sum": 0.0, "confusion": cm})
    container.load_state("val", {"counts": counts, "loss_sum": 0.0, "confusion": cm.T.copy()})
    v = container["train_val_diff"].value
    assert v["train"].dtype == torch.float64 and v["train"][[0, 1, 3]].tolist() == [2 / 3, 1.0, 0.5] and torch.isnan(v["train"][2])
    assert v["val"][[0, 1, 3]].tolist() == [2 / 3, 0.75, 1.0]
    with pytest.raises(ValueError, match="both contexts"):
        M.MetricsContainer([M.MultiClassAccuracy("train_val_accuracy")])
    with pytest.raises(ValueError, match="names no context"):
        M.MetricsContainer([M.Mean("loss")])
    with pytest.raises(ValueError, match="one k per context"):
        M.MetricsContainer([M.TopKAccuracy("training_top3", k=3), M.TopKAccuracy("training_top5", k=5)])


def test_build_metrics_list_and_summary(d):
    names = lambda c: [m.name for m in c.get_metrics()]      # noqa: E731
    assert names(M.build_metrics(27)) == ["training_loss", "validation_loss", "training_accuracy", "validation_accuracy",
                                          "training_confusion", "validation_confusion", "training_top5_accuracy",
                                          "validation_top5_accuracy", "lr"]
    extra = [_Probe("val_extra")]
    ev = M.build_metrics(27, k=1, additional_metrics=extra, is_eval=True)
    assert names(ev) == ["validation_loss", "validation_accuracy", "validation_confusion", "val_extra"]
    assert ev["validation_confusion"].write_to_summary_interval == 1 and M.build_metrics(27)["training_confusion"].write_to_summary_interval == 5
    assert M.build_metrics(27, k=3)["training_top3_accuracy"]._k == 3 and M.build_metrics(27, k=3)._states["train"].k == 3

    class Writer:
        def __init__(self):
            self.scalars, self.texts, self.figures = [], [], []

        def add_scalar(self, *a):
            self.scalars.append(a)

        def add_text(self, *a):
            self.texts.append(a)

        def add_figure(self, *a, **k):
            self.figures.append(a)

    classes, k, rows = MG.spec(d, "c5")
    container = MG.build_container(classes, k)
    _install(container, d, "c5", len(rows) - 1)
    w = Writer()
    container.to_summary(w, 5)
    got = dict((n, v) for n, v, e in w.scalars)
    assert all(e == 5 for _, _, e in w.scalars) and not w.figures
    assert set(got) == {m.name for m in container.get_metrics() if isinstance(m, M.ScalarMetric)}
    assert got["validation_top5_accuracy"] == 1.0 and got["training_loss"] == float(d["c5_step1_training_loss"])
    assert [t[0] for t in w.texts] == ["training_misclassified", "validation_misclassified"]
    assert w.texts[0][1].startswith("| Sample | Prediction | Ground Truth |  \n| --- | --- | --- |  \n| ")
    container["training_accuracy"].write_to_summary_interval = 2
    w = Writer()
    container.to_summary(w, 3)
    assert "training_accuracy" not in dict((n, v) for n, v, e in w.scalars)


def test_no_fallback_on_host_tensors():
    container = M.build_metrics(5)
    out = (torch.randn(4, 5), torch.randint(0, 5, (4,)))
    with pytest.raises(_lib.FgcnError):
        container.update_training(torch.tensor(1.0), out, None, torch.arange(4))
    with pytest.raises(_lib.FgcnError):
        container.update_validation(torch.tensor(1.0), out, None, torch.arange(4))
    with pytest.raises(RuntimeError, match="MetricsContainer"):         # a state-backed metric lives in a container
        M.MultiClassAccuracy().update(out)
    with pytest.raises(RuntimeError, match="register it"):
        M.MultiClassAccuracy().value
    assert container.format_all().count("0.0000") == 7          # nothing was counted


def test_module_imports_without_tensorboard_or_matplotlib():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('tensorboard', 'matplotlib', 'oracle') or name == 'torch.utils.tensorboard':\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "import fusion_gcn_amd.metrics as m\n"
            "assert not any(n.split('.')[0] in ('tensorboard', 'matplotlib', 'oracle') for n in sys.modules), 'imported'\n"
            "assert 'torch.utils.tensorboard' not in sys.modules\n"
            "print(m.build_metrics(3).format_all())\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("training_loss: 0.0000")


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_state_bytes_sweep(lib):
    for c in list(range(1, 130)) + [255, 256, 400, 1023, 1024]:
        want = (64 + 4 * c * c + 7) // 8 * 8
        assert lib.fgcn_classify_state_bytes(c) == want, c
        st = M._State()
        st._set_classes(c)
        assert st._words() * 8 == want
    for c in (0, -1, 1025, 1 << 20):
        assert lib.fgcn_classify_state_bytes(c) == 0
    assert (_lib.CLS_EXAMPLES, _lib.CLS_TOP1, _lib.CLS_TOPK, _lib.CLS_IGNORED, _lib.CLS_INVALID, _lib.CLS_DROPPED, _lib.CLS_LOSS_ITEMS,
            _lib.CLS_LOSS_SUM, _lib.CLS_WORDS) == tuple(range(9))
    header = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    for i, word in enumerate(("EXAMPLES", "TOP1", "TOPK", "IGNORED", "INVALID", "DROPPED", "LOSS_ITEMS", "LOSS_SUM", "WORDS")):
        assert f"FGCN_CLS_{word} = {i}" in header
    assert f"#define FGCN_CLS_MAX_CLASSES {_lib.CLS_MAX_CLASSES}" in header


def test_classify_update_rejects_bad_arguments_before_any_launch(lib):
    p = C.c_void_p(64)                # never dereferenced: validation precedes HIP
    ok = dict(logits=p, labels=p, loss=None, state=p, pred_out=None, pred_offset=0, pred_capacity=0, rows=8, classes=27, ld=27, k=5)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.fgcn_classify_update(a["logits"], a["labels"], a["loss"], a["state"], a["pred_out"], a["pred_offset"], a["pred_capacity"],
                                      a["rows"], a["classes"], a["ld"], a["k"], None)
        return rc, lib.fgcn_last_error()

    for bad, text in ((dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(state=None), b"null pointer"),
                      (dict(rows=0), b"rows=0"), (dict(rows=-3), b"rows=-3"), (dict(classes=0, ld=0, k=0), b"classes=0"),
                      (dict(classes=1025, ld=1025), b"classes=1025"), (dict(ld=26), b"ld=26"), (dict(k=0), b"k=0"),
                      (dict(k=28), b"k=28"), (dict(pred_offset=-1), b"pred_offset=-1"), (dict(pred_capacity=-1), b"pred_capacity=-1")):
        rc, msg = call(**bad)
        assert rc == -1 and text in msg and msg.startswith(b"classify_update"), (bad, rc, msg)
    rc, msg = call(state=C.c_void_p(68))
    assert rc == -2 and b"8-byte aligned" in msg


# ---- data parallelism -------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def _half_states(d, s, long, ctx):
    """The golden stream's last state split in two: rank 0 holds the state after the first batch, rank 1 the rest."""
    last = len(MG.spec(d, s)[2]) - 1
    first, whole = MG.expected_state(d, s, 0, long), MG.expected_state(d, s, last, long)
    rest = {key: whole[key] - first[key] for key in whole}
    rest["confusion"] = rest["confusion"].astype(np.int32)
    return first, rest


def _all_reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        d, s = MG.load(), "b60"
        classes, k, rows = MG.spec(d, s)
        container = M.build_metrics(classes, k=k, additional_metrics=[M.F1MeasureMetric("training_f1"), M.F1MeasureMetric("validation_f1")])
        for ctx, long in MG.CONTEXTS:
            container.load_state(ctx, _half_states(d, s, long, ctx)[rank])
        container.all_reduce()
        out = {}
        for ctx, long in MG.CONTEXTS:
            snap = container.state_snapshot(ctx)
            out[long] = (snap["counts"], snap["loss_sum"], snap["confusion"],
                         {n: container[f"{long}_{n}"].value for n in ("loss", "accuracy", f"top{k}_accuracy", "f1")})
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_all_reduce_over_gloo_gives_the_whole_stream(d):
    import torch.multiprocessing as mp
    world, s = 2, "b60"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_all_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    classes, k, rows = MG.spec(d, s)
    last = len(rows) - 1
    for rank in range(world):
        for _, long in MG.CONTEXTS:
            counts, loss_sum, confusion, values = got[rank][long]
            want = MG.expected_state(d, s, last, long)
            assert (counts == want["counts"]).all() and counts.dtype == np.int64
            assert (confusion == want["confusion"]).all() and confusion.dtype == np.int32
            assert abs(loss_sum - want["loss_sum"]) <= 1e-12 * abs(want["loss_sum"])
            for name, v in values.items():
                g = float(d[f"{s}_step{last}_{long}_{name}"])
                assert abs(v - g) <= 1e-12 * abs(g), (rank, long, name)
    # without a process group: a no-op
    container = M.build_metrics(classes, k=k)
    container.load_state("train", MG.expected_state(d, s, 0, "training"))
    container.all_reduce()
    assert (container.state_snapshot("train")["confusion"] == d[f"{s}_step0_training_confusion"]).all()
