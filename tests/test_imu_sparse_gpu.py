"""The sparse aggregation route of the static-adjacency IMU graph convolution on the GPU: fgcn_graph_spmm against the float64 dense
product, its determinism, and ``sparse=True`` models against the float64 oracle with the tolerances of tests/test_imu_gcn.py.

Kernel tolerance (derived, not tuned).  A row with n entries is a chain of n float32 FMAs; its forward error is bounded by
n * u * S with u = 2^-24 and S = sum_j |val_j| * |in_j|.  The bound asserted is 2 * (n + 1) * u * S elementwise: one more operation for the
store-side arithmetic and a factor 2 of slack.  With a residual the epilogue adds the terms ``b`` (identity) or ``b * scale`` and
``shift`` (affine) to the sum, each rounded once more, so S gains their magnitudes (|b|, or |b * scale| + |shift|): without them an
empty row (S = 0) would have to reproduce ``b * scale + shift`` exactly, which a float32 FMA cannot.  ReLU does not increase an error."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import imu_gcn_oracle as O
from test_imu_gcn import CASES, GOLD, build, fmt, inputs, late_build, late_inputs, late_loss_and_grads, late_oracle

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
U = 2.0 ** -24
MODES = ("f32", "bf16x3", "f16x2")


def dev():
    return torch.device("cuda:0")


def config_adj(inter=False, back=1, frames=326):
    from fusion_gcn_amd.models.mmargcn.imu_feature_models import build_imu_graph_adjacency
    return build_imu_graph_adjacency((frames, 6), 0, "stgcn", False, "column", back, inter)


def random_adj(V, seed, max_nnz=40):
    """0 .. max_nnz non-zeros per row (at most V), every fifth row empty, random values of both signs."""
    g = torch.Generator().manual_seed(seed)
    a = torch.zeros(V, V)
    for v in range(V):
        n = 0 if v % 5 == 3 else int(torch.randint(0, min(max_nnz, V) + 1, (1,), generator=g))
        cols = torch.randperm(V, generator=g)[:n]
        a[v, cols] = torch.randn(n, generator=g)
    return a


def check_forms(adj, B, C, seed, ld_extra=0, forms=("plain", "relu", "identity", "affine")):
    """Every epilogue form of ops.graph_spmm on one (matrix, B, C) against the same expression in float64."""
    from fusion_gcn_amd import ops
    V = adj.shape[0]
    g = torch.Generator().manual_seed(seed)
    wide = guarded.to(torch.randn(B, V, C + ld_extra, generator=g), dev())
    x = wide[..., :C]                                                       # row stride C + ld_extra
    b = guarded.to(torch.randn(B, V, C, generator=g), dev())
    vec = torch.zeros(4, C)
    vec[2], vec[3] = torch.randn(C, generator=g), torch.randn(C, generator=g)
    vec = guarded.to(vec, dev())
    csr = ops.csr_from_dense(guarded.to(adj, dev()))
    a64 = guarded.to(adj.double(), dev())
    x64, b64 = x.double(), b.double()
    prod = torch.matmul(a64, x64)                                           # float64 dense product adj @ in[b]
    mag = torch.matmul(a64.abs(), x64.abs())
    n_row = guarded.to((adj != 0).sum(1).double(), dev()).view(1, V, 1)
    worst = {}
    for form in forms:
        kw, want, s = {}, prod, mag
        if form in ("identity", "affine"):
            kw["b"] = b
            if form == "affine":
                kw["vec_b"] = vec
                want = prod + b64 * vec[2].double() + vec[3].double()
                s = mag + (b64 * vec[2].double()).abs() + vec[3].double().abs()
            else:
                want, s = prod + b64, mag + b64.abs()
        relu = form != "plain"
        if relu:
            want = want.clamp_min(0)
        got, mask = ops.graph_spmm(x, csr, relu=relu, sign_mask=True, **kw)
        bound = 2 * (n_row + 1) * U * s
        err = (got.double() - want).abs()
        worst[form] = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else 0.0
        assert bool((err <= bound).all()), (form, V, B, C, worst[form])
        if C % 8 == 0:                                                      # the sign image equals out > 0 bit for bit
            bits = np.unpackbits(mask.cpu().numpy(), bitorder="little").astype(bool)
            assert np.array_equal(bits, (got > 0).flatten().cpu().numpy()), (form, V, B, C)
        else:
            assert mask is None
        assert torch.equal(ops.graph_spmm(x, csr, relu=relu, **kw), got)    # the form without the mask: the same bits
    return worst


@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("back", [1, 2])
def test_kernel_on_the_config_graph(inter, back):
    adj = config_adj(inter, back)
    print(check_forms(adj, 8, 512, seed=10 * back + inter))
    print(check_forms(adj, 3, 36, seed=20 * back + inter, ld_extra=12))


V_ALL, C_ALL, B_ALL = (1, 48, 240, 1956), (4, 8, 36, 512, 2048, 4096), (1, 3, 8)
# every V with every C, the batch sizes rotating so that every (V, B) and every (C, B) pair occurs; and the largest of all three
RANDOM_CASES = [(V, C, B_ALL[(i + j) % 3]) for i, V in enumerate(V_ALL) for j, C in enumerate(C_ALL)] + [(1956, 4096, 8), (1, 4, 8)]


@pytest.mark.parametrize("V,C,B", RANDOM_CASES)
def test_kernel_on_random_patterns(V, C, B):
    adj = random_adj(V, seed=V + C + B)
    assert int((adj != 0).sum(1).min()) == 0 or V < 4
    print(check_forms(adj, B, C, seed=V * 7 + C + B, ld_extra=8 if (C + B) % 2 else 0))


def test_kernel_is_deterministic_and_ignores_the_math_mode():
    from fusion_gcn_amd import ops
    g = torch.Generator().manual_seed(5)
    for adj, C in ((config_adj(True, 2), 512), (random_adj(240, 9), 36)):
        V = adj.shape[0]
        x, b = guarded.to(torch.randn(3, V, C, generator=g), dev()), guarded.to(torch.randn(3, V, C, generator=g), dev())
        vec = guarded.to(torch.randn(4, C, generator=g), dev())
        csr = ops.csr_from_dense(guarded.to(adj, dev()))
        first = ops.graph_spmm(x, csr, relu=True, b=b, vec_b=vec)
        assert torch.equal(ops.graph_spmm(x, csr, relu=True, b=b, vec_b=vec), first)          # two launches: the same bits
        for m in ("f32", "bf16x3", "f16x2", "bf16"):
            with ops.math_mode(m):
                assert torch.equal(ops.graph_spmm(x, csr, relu=True, b=b, vec_b=vec), first), m


@pytest.mark.parametrize("which", ["config", "config_inter2", "random240", "random48"])
def test_transposed_form_is_the_data_gradient(which):
    from fusion_gcn_amd import ops
    adj = {"config": lambda: config_adj(), "config_inter2": lambda: config_adj(True, 2), "random240": lambda: random_adj(240, 2),
           "random48": lambda: random_adj(48, 4)}[which]()
    V, B, C = adj.shape[0], 3, 64
    d = guarded.to(torch.randn(B, V, C, generator=torch.Generator().manual_seed(11)), dev())
    got = ops.graph_spmm(d, ops.csr_from_dense(guarded.to(adj, dev()), transpose=True))
    at = guarded.to(adj.t().double(), dev())
    want, mag = torch.matmul(at, d.double()), torch.matmul(at.abs(), d.double().abs())
    n_row = guarded.to((adj.t() != 0).sum(1).double(), dev()).view(1, V, 1)
    assert bool(((got.double() - want).abs() <= 2 * (n_row + 1) * U * mag).all())


def stgcn_case(tag):
    if tag in CASES:
        return CASES[tag]
    if tag == "value240":
        return (40, 6), 27, 4, dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=5, inner_feature_dim=64)
    if tag == "wide2048":
        return (8, 6), 27, 2, dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=4, inner_feature_dim=1024)
    assert tag == "value1956"
    return (326, 6), 27, 2, dict(gc_model="stgcn", graph_node_format="node_per_value", num_layers=3, inner_feature_dim=32)


STGCN_TAGS = ["value48", "sensor16", "value240", "value1956", "wide2048"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", STGCN_TAGS)
def test_sparse_model_matches_the_oracle(tag, mode):
    """tests/test_imu_gcn.py::test_hip_imu_gcn_matches_the_oracle with sparse=True: the same oracle, the same tolerances, every parameter."""
    from fusion_gcn_amd import ops
    shape, classes, batch, kw = stgcn_case(tag)
    model, sd = build(tag, shape, classes, dict(kw, sparse=True))
    x, y = inputs(tag, shape, batch, classes)
    ref_eval = O.imu_gcn_forward(x, sd, train=False, **fmt(kw))
    ref_logits, ref_loss, ref_grads = O.loss_and_grads(x, y, sd, **fmt(kw))
    model = guarded.to(model, dev())
    with ops.math_mode(mode):
        model.eval()
        with torch.no_grad():
            got_eval = model(guarded.to(x.float(), dev())).cpu().double()
        assert rel_l2(got_eval.numpy(), ref_eval.numpy()) < 2e-5
        model.train()
        logits = model(guarded.to(x.float(), dev()))
        loss = F.cross_entropy(logits, guarded.to(y, dev()))
        loss.backward()
    assert rel_l2(logits.detach().cpu().double().numpy(), ref_logits.numpy()) < 2e-5
    assert abs(float(loss.detach()) - float(ref_loss)) < 2e-5 * max(1.0, abs(float(ref_loss)))
    scale = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    seen = 0
    for name, p in model.named_parameters():
        k = name.replace("_model.", "")
        want = ref_grads[k]
        got = p.grad.detach().cpu().double()
        seen += 1
        if k.endswith("residual.0.bias"):                 # in front of a train-mode BatchNorm: exactly zero here
            assert float(got.abs().max()) == 0.0 and float(want.abs().max()) < 1e-9 * max(1.0, scale)
            continue
        tol = 2e-3 if k.endswith("residual.0.weight") else 5e-4
        assert rel_l2(got.numpy(), want.numpy()) < tol, (k, rel_l2(got.numpy(), want.numpy()))
    assert seen == len(ref_grads)                         # nothing excluded
    if tag in CASES:
        assert rel_l2(logits.detach().cpu().double().numpy(), GOLD[f"{tag}.train.logits"]) < 2e-5
        bn = dict(model.named_buffers())
        for k in GOLD.files:
            if k.startswith(f"{tag}.after."):
                assert rel_l2(bn["_model." + k[len(f"{tag}.after."):]].cpu().double().numpy(), GOLD[k]) < 1e-5, k


@pytest.mark.parametrize("tag", ["value240", "wide2048"])
def test_sparse_model_bf16_contract(tag):
    """Math mode bf16: the sparse route's adjacency product stays float32 while the dense route rounds its operands, so the check is the
    mode's model contract of tests/test_bf16_gpu.py (logits rel-L2 <= 1e-2, gradient cosine >= 0.98 against the f32 mode)."""
    from fusion_gcn_amd import ops
    shape, classes, batch, kw = stgcn_case(tag)
    model, _ = build(tag, shape, classes, dict(kw, sparse=True))
    model = guarded.to(model, dev()).train()
    x, y = inputs(tag, shape, batch, classes)
    x, y = guarded.to(x.float(), dev()), guarded.to(y, dev())

    def run():
        for p in model.parameters():
            p.grad = None
        logits = model(x)
        F.cross_entropy(logits, y).backward()
        return logits.detach().clone(), torch.cat([p.grad.flatten() for p in model.parameters()]).clone()
    with ops.math_mode("bf16"):
        lg_b, g_b = run()
    with ops.math_mode("f32"):
        lg_f, g_f = run()
    e_logits = float((lg_b - lg_f).norm() / lg_f.norm())
    cos = float(torch.dot(g_b, g_f) / (g_b.norm() * g_f.norm()))
    print(f"sparse {tag} bf16: logits rel-L2 {e_logits:.2e}, gradient cosine {cos:.4f}")
    assert e_logits <= 1e-2 and cos >= 0.98


class Counter:
    def __init__(self, monkeypatch, ops, names):
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(ops, k, self.wrap(k, getattr(ops, k)))

    def wrap(self, k, fn):
        def inner(*a, **kw):
            self.n[k] += 1
            return fn(*a, **kw)
        return inner


@pytest.mark.parametrize("mode", MODES)
def test_route(monkeypatch, mode):
    """sparse=True: no transposes and two graph_spmm calls per layer (forward, data gradient); without the kwarg: no graph_spmm and the
    four transposes per layer of the dense route -- it launches no new kernel."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.models.mmargcn.graph_convolution import STGCNGraphConvolution
    shape, classes, batch, kw = stgcn_case("value240")
    x, y = inputs("value240", shape, batch, classes)
    for sparse in (True, False):
        model, _ = build("value240", shape, classes, dict(kw, sparse=True) if sparse else kw)
        model = guarded.to(model, dev()).train()
        layers = sum(isinstance(m, STGCNGraphConvolution) for m in model.modules())
        with monkeypatch.context() as mp, ops.math_mode(mode):
            c = Counter(mp, ops, ("transpose", "transpose_into", "graph_spmm"))
            F.cross_entropy(model(guarded.to(x.float(), dev())), guarded.to(y, dev())).backward()
            torch.cuda.synchronize()
        want = (0, 0, 2 * layers) if sparse else (2 * layers, 2 * layers, 0)
        assert (c.n["transpose"], c.n["transpose_into"], c.n["graph_spmm"]) == want, (sparse, c.n)


def test_auto_route_through_path_options(monkeypatch):
    """PathOptions.graph_spmm_auto sends a dense-configured model down the sparse route when its adjacency is sparse enough -- and gives the
    sparse=True model's result bit for bit; a threshold below the graph's density leaves it on the dense route."""
    from fusion_gcn_amd import ops
    shape, classes, batch, kw = stgcn_case("value240")
    x, y = inputs("value240", shape, batch, classes)
    x, y = guarded.to(x.float(), dev()), guarded.to(y, dev())
    dense, _ = build("value240", shape, classes, kw)
    sparse, _ = build("value240", shape, classes, dict(kw, sparse=True))
    dense, sparse = guarded.to(dense, dev()).train(), guarded.to(sparse, dev()).train()
    want = sparse(x).detach()
    for ppm, calls in ((50_000, True), (10, False)):
        with ops.context() as ctx, monkeypatch.context() as mp:
            ctx.paths.graph_spmm_auto, ctx.paths.graph_spmm_auto_density_ppm = True, ppm
            c = Counter(mp, ops, ("graph_spmm",))
            got = dense(x)
            got.sum().backward()
        assert (c.n["graph_spmm"] > 0) == calls
        if calls:
            assert torch.equal(got.detach(), want)


@pytest.mark.parametrize("mode", MODES)
def test_sparse_late_fusion_matches_the_oracle(mode):
    """tests/test_imu_gcn.py::test_hip_late_fusion_matches_the_oracle (gc_model stgcn) with sparse=True."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.graph_convolution import STGCNGraphConvolution
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    from test_imu_gcn import LATE_KW, LATE_SHAPES
    dense, sd = late_build(gc_model="stgcn")
    model = Model(LATE_SHAPES, 27, Graph(utd.skeleton_edges, center_joint=utd.center_joint), mode="skeleton_imu_gcn_late_fusion",
                  **dict(LATE_KW, gc_model="stgcn", sparse=True))
    model.load_state_dict(dense.state_dict())
    layers = [m for m in model.modules() if isinstance(m, STGCNGraphConvolution)]
    assert layers and all(m.sparse for m in layers)
    x, y = late_inputs()
    ref_logits, ref_loss, ref_grads = late_loss_and_grads(x, y, sd)
    ref_eval = late_oracle(x, sd, train=False).detach()
    model = guarded.to(model, dev())
    xg = {k: guarded.to(v.float(), dev()) for k, v in x.items()}
    with ops.math_mode(mode):
        model.eval()
        with torch.no_grad():
            assert rel_l2(model(xg).cpu().double().numpy(), ref_eval.numpy()) < 5e-5
        model.train()
        logits = model(xg)
        loss = F.cross_entropy(logits, guarded.to(y, dev()))
        loss.backward()
    assert rel_l2(logits.detach().cpu().double().numpy(), ref_logits.numpy()) < 5e-5
    assert abs(float(loss.detach()) - float(ref_loss)) < 1e-4
    assert rel_l2(logits.detach().cpu().double().numpy(), GOLD["late.train.logits"]) < 5e-5
    for name, p in model.named_parameters():
        k = name.replace("_model.", "")
        want = ref_grads[k]
        got = p.grad.detach().cpu().double()
        wn = 0.0 if want is None else float(want.norm())
        if wn < 1e-9:
            assert float(got.norm()) < 1e-6, k
        else:
            assert abs(float(got.norm()) - wn) < 1e-2 * wn, (k, float(got.norm()), wn)


@pytest.mark.parametrize("mode", MODES)
def test_sparse_model_in_a_recorded_step(mode):
    """GraphStep: a sparse=True model recorded and replayed gives the eager step's loss and gradients; after the model moved
    (``model.to``: new buffer addresses) or its adjacency buffer was replaced, the next step records again with rebuilt CSR forms."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.models.mmargcn.graph_convolution import STGCNGraphConvolution
    from fusion_gcn_amd.session.procedures import DefaultStep, GraphStep
    shape, classes, batch, kw = stgcn_case("value240")
    model, _ = build("value240", shape, classes, dict(kw, sparse=True))
    model = guarded.to(model, dev()).train()
    x, y = inputs("value240", shape, batch, classes)
    x, y = guarded.to(x.float(), dev()), guarded.to(y, dev())
    layers = [m for m in model.modules() if isinstance(m, STGCNGraphConvolution)]

    def run(step):
        state = [b.detach().clone() for b in model.buffers()]
        for p in model.parameters():
            p.grad = None
        with ops.math_mode(mode):
            _, loss = step.forward(model, F.cross_entropy, x, y)
            step.backward(loss)
        torch.cuda.synchronize()
        out = float(loss.detach()), torch.cat([p.grad.flatten() for p in model.parameters()]).clone()
        with torch.no_grad():
            for b, s in zip(model.buffers(), state):          # every run starts from the same BatchNorm statistics
                b.copy_(s)
        return out

    def same(a, b):
        assert abs(a[0] - b[0]) <= 1e-6 * abs(b[0]) and float((a[1] - b[1]).norm()) <= 1e-5 * float(b[1].norm())
    step = GraphStep()
    eager = run(DefaultStep())
    same(run(step), eager)
    same(run(step), eager)                                    # a replay
    assert step.replays == 2 and all(m._csr_cache[1] in m.recording_pins() for m in layers)
    # a replaced adjacency buffer with other values: the recording is stale, the CSR forms are rebuilt from the new buffer
    old_keys = [m._csr_cache[0] for m in layers]
    for m in layers:
        m.adj = (m.adj * 0.5).clone()
    eager2 = run(DefaultStep())
    assert abs(eager2[0] - eager[0]) > 1e-4 * abs(eager[0])
    same(run(step), eager2)
    assert all(m._csr_cache[0] != k and m._csr_cache[0][1] == m.adj.data_ptr() for m, k in zip(layers, old_keys))
    assert all(torch.equal(m._csr_cache[1]["adj"][2], m.adj[m.adj != 0]) for m in layers)
    # model.to(...): every parameter and buffer gets a new home
    for p in model.parameters():          # (Module.to converts a held .grad in place -- here a view of the step's flat buffer: drop them first)
        p.grad = None
    guarded.to(model.to("cpu"), dev())
    same(run(step), eager2)
    assert all(m._csr_cache[0][1] == m.adj.data_ptr() for m in layers)


@pytest.mark.parametrize("tag", STGCN_TAGS)
def test_sparse_model_inference(tag):
    """Eval mode under torch.no_grad(): forward only, 2e-5 against the oracle; no autograd graph, no saved tensors."""
    shape, classes, batch, kw = stgcn_case(tag)
    model, sd = build(tag, shape, classes, dict(kw, sparse=True))
    x, _ = inputs(tag, shape, batch, classes)
    want = O.imu_gcn_forward(x, sd, train=False, **fmt(kw))
    model = guarded.to(model, dev()).eval()
    with torch.no_grad():
        got = model(guarded.to(x.float(), dev()))
    assert not got.requires_grad and rel_l2(got.cpu().double().numpy(), want.numpy()) < 2e-5
