"""``dropout=`` in the IMU graph convolution and the MS-G3D MLP on the GPU: the kernels against the numpy generator
bit for bit, the device-side step counter eagerly and under HIP-graph replay, the layers against float64 restatements that take the
layer's own kept-bit image (tests/dropout_ref.py; tests/test_dropout.py checks on the CPU that those references stay off the ReLU's
kink), repeatability of whole training steps, GraphStep, and the late-fusion model.

Tolerances are those the same kernels meet without dropout: tests/test_imu_gcn.py's for the graph convolution (forward 2e-5, gradients
5e-4, the residual conv's weight in front of its BatchNorm 2e-3), tests/test_msg3d.py's for the MLP layer (2e-5) and for
MultiScale_GraphConv (FWD_TOL 2e-5, GRAD_TOL 2e-4 of test_multi_scale_graph_conv_matches_the_oracle).  Dropout itself adds one exact
select and one float32 multiplication per element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dropout_ref as R
from conftest import rel_l2

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]
DEV = torch.device("cuda:0")
MODES = pytest.mark.parametrize("fgcn_math", ["f32", "bf16x3", "f16x2"], indirect=True)
WG = 256 * 8                 # elements one workgroup of the dropout kernels covers


def _word(t):
    return int(t.view(torch.int64).cpu().item())


def _set_word(t, value):
    t.copy_(torch.tensor([value], dtype=torch.uint64))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _fused(model):
    from fusion_gcn_amd.fops import FusedDropout
    return [m for m in model.modules() if isinstance(m, FusedDropout)]


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [8, 12, WG, 3 * WG + 20])
def test_kernels_match_the_numpy_generator_bit_for_bit(n, p):
    """one thread; the four-element tail thread; one workgroup's worth; several workgroups and a tail"""
    from fusion_gcn_amd import ops
    seed = 0x9E3779B97F4A7C15
    x, dy = R.rnd(n, seed=n).float(), R.rnd(n, seed=n + 1).float()
    xg, dyg = guarded.to(x, DEV), guarded.to(dy, DEV)
    s = R.scale(p)
    for site in (0, 7):
        for step in (0, 2 ** 32 + 5):
            word = guarded.to(torch.tensor([step], dtype=torch.uint64), DEV)
            y, mask = ops.dropout_fwd(xg, p, seed, site, word)
            kept = R.keep(n, p, seed, site, step)
            assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), R.pack(kept)), (site, step)
            want = np.where(kept, x.numpy() * s, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(_bits(y), want.view(np.uint32)), (site, step)
            assert _word(word) == step                                    # the forward reads the word and leaves it
            want_dx = np.where(kept, dy.numpy() * s, np.float32(0.0)).astype(np.float32)
            assert np.array_equal(_bits(ops.dropout_bwd(dyg, mask, p)), want_dx.view(np.uint32)), (site, step)
            buf = dyg.clone()
            assert ops.dropout_bwd(buf, mask, p, out=buf) is buf and np.array_equal(_bits(buf), want_dx.view(np.uint32))      # in place
    assert torch.equal(xg.cpu(), x) and torch.equal(dyg.cpu(), dy)        # the inputs are untouched


def test_ops_check_their_arguments_like_their_neighbours():
    from fusion_gcn_amd import _lib, ops
    x, word = torch.zeros(16, device=DEV), guarded.to(torch.zeros(1, dtype=torch.uint64), DEV)
    for bad in (x.double(), x.cpu(), torch.zeros(4, 8, device=DEV)[:, ::2]):
        with pytest.raises(_lib.FgcnError):
            ops.dropout_fwd(bad, 0.5, 1, 0, word)
    for bad in (word.cpu(), torch.zeros(1, dtype=torch.int64, device=DEV), guarded.to(torch.zeros(2, dtype=torch.uint64), DEV)):
        with pytest.raises(_lib.FgcnError):
            ops.dropout_fwd(x, 0.5, 1, 0, bad)
        with pytest.raises(_lib.FgcnError):
            ops.rng_advance(bad)
    with pytest.raises(_lib.FgcnError):
        ops.dropout_fwd(torch.zeros(6, device=DEV), 0.5, 1, 0, word)       # n % 4
    with pytest.raises(_lib.FgcnError):
        ops.dropout_fwd(x, 1.0, 1, 0, word)
    with pytest.raises(_lib.FgcnError):
        ops.dropout_bwd(x, torch.zeros(3, dtype=torch.uint8, device=DEV), 0.5)


# ---- the step counter ----------------------------------------------------------------------------------------------------------------
def test_two_calls_draw_the_masks_of_two_consecutive_steps():
    from fusion_gcn_amd import fops
    drop = guarded.to(fops.FusedDropout(0.5), DEV)
    drop.reseed(11, site=2)
    start = 2 ** 32 - 1                                                    # the second step carries into the high half of the word
    _set_word(drop.step, start)
    n = WG + 12
    x = guarded.to(R.rnd(n, seed=3).float(), DEV).requires_grad_(True)
    outs = []
    for k in range(2):
        y = fops.dropout(x, drop, drop.p, True)
        kept = R.keep(n, 0.5, 11, 2, start + k)
        assert np.array_equal(drop.keep_mask.cpu().numpy(), R.pack(kept)), k
        outs.append((y, kept))
    assert _word(drop.step) == start + 2
    assert not np.array_equal(outs[0][1], outs[1][1])
    (outs[0][0].sum() + 2 * outs[1][0].sum()).backward()                  # each backward reads the image of its own forward
    want = (outs[0][1] * R.scale(0.5) + 2 * (outs[1][1] * R.scale(0.5))).astype(np.float32)
    assert np.array_equal(x.grad.cpu().numpy(), want)
    assert fops.dropout(x, drop, drop.p, False) is x and fops.dropout(x, drop, 0.0, True) is x and _word(drop.step) == start + 2
    assert not fops.dropout(x, drop, 1.0, True).any()


def test_a_captured_forward_and_advance_draw_new_masks_on_every_replay():
    from fusion_gcn_amd import fops
    drop = guarded.to(fops.FusedDropout(0.3), DEV)
    n = 3 * WG + 20
    x = guarded.to(R.rnd(n, seed=4).float(), DEV)
    drop.reseed(13)
    drop.draw(x)                                                           # eager warm-up: the library and the device check are loaded
    drop.reseed(13)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, mask = drop.draw(x)
    assert _word(drop.step) == 0                                           # recorded, not run
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        kept = R.keep(n, 0.3, 13, 0, k)
        assert np.array_equal(mask.cpu().numpy(), R.pack(kept)), k
        assert np.array_equal(_bits(y), np.where(kept, x.cpu().numpy() * R.scale(0.3), np.float32(0.0)).astype(np.float32).view(np.uint32)), k
    assert _word(drop.step) == 3


# ---- the IMU graph convolution against its float64 restatement -------------------------------------------------------------------
_refs = {}


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _gc_layer(kind, sparse, dropout):
    from fusion_gcn_amd.models.mmargcn.graph_convolution import STGCNGraphConvolution
    fin, o, residual = R.GC_CASES[kind]
    layer = STGCNGraphConvolution(fin, o, R.ring_adjacency().float(), residual=residual, sparse=sparse, dropout=dropout)
    missing = layer.load_state_dict({k: v.float() for k, v in R.gc_case(kind)["params"].items()}, strict=False)
    assert not missing.unexpected_keys
    return guarded.to(layer, DEV)


def _gc_input(kind):
    x = R.gc_case(kind)["x"].float()
    return guarded.to(F.pad(x, (0, (-x.shape[-1]) % 4)).contiguous(), DEV).requires_grad_(True)        # node-major, channels padded to 4


@MODES
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("kind", list(R.GC_CASES))
def test_graph_convolution_with_dropout_matches_float64(kind, sparse, fgcn_math):
    """relu(mask s (conv(x) adj^T) + res) with the layer's own keep_mask, all three residual kinds, the dense and the gather route."""
    fin, o, _ = R.GC_CASES[kind]
    case = R.gc_case(kind)
    layer = _gc_layer(kind, sparse, R.GC_P).train()
    assert layer.takes_sparse_route() == sparse and layer.res_kind == kind
    layer.dropout.reseed(R.GC_SEED)
    xg = _gc_input(kind)
    out = layer(xg)
    n = R.B * R.V * o
    kept = R.unpack(layer.dropout.keep_mask.cpu().numpy(), n).reshape(R.B, R.V, o)
    assert np.array_equal(kept.reshape(-1), R.keep(n, R.GC_P, R.GC_SEED, 0, 0)) and _word(layer.dropout.step) == 1
    ref = _cached(("gc", kind), lambda: R.gc_reference(kind, kept))
    assert R.off_the_kink(ref["pre"], kept if kind == "none" else None) >= 1e-4               # no ReLU flip can hide
    (out * guarded.to(case["probe"].float(), DEV)).sum().backward()
    named = dict(layer.named_parameters())
    errors = {"forward": rel_l2(out.detach().cpu().numpy(), ref["out"].numpy()),
              "dx": rel_l2(xg.grad[..., :fin].cpu().numpy(), ref["gx"].numpy())}
    for k, g in ref["grads"].items():
        if k == "residual.0.bias":          # in front of a train-mode BatchNorm: exactly zero here, rounding noise in autograd
            assert float(named[k].grad.abs().max()) == 0.0 and float(g.abs().max()) < 1e-9
        else:
            errors[k] = rel_l2(named[k].grad.cpu().numpy(), g.numpy())
    print(f"[dropout gc {kind} sparse={sparse} {fgcn_math}] " + ", ".join(f"{k} {e:.2e}" for k, e in errors.items()))
    for k, e in errors.items():
        assert e < (2e-5 if k == "forward" else 2e-3 if k == "residual.0.weight" else 5e-4), (k, e)
    assert not xg.grad[..., fin:].any()                                                    # the zero pad channels receive nothing
    # eval mode: the calls of a layer without dropout, bit for bit
    plain = _gc_layer(kind, sparse, 0.0)
    plain.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert torch.equal(layer.eval()(xg), plain.eval()(xg)) and _word(layer.dropout.step) == 1


# ---- the MS-G3D MLP ------------------------------------------------------------------------------------------------------------------
def _mlp(dropout):
    from fusion_gcn_amd.models.msg3d.mlp import MLP
    mlp = MLP(R.MLP_SHAPE[-1], [R.MLP_OUT], dropout=dropout)
    i = len(mlp.layers) - 3
    p = R.mlp_case()["params"]
    mlp.load_state_dict({f"layers.{i}.weight": p["weight"].float(), f"layers.{i}.bias": p["bias"].float(),
                         f"layers.{i + 1}.weight": p["gamma"].float(), f"layers.{i + 1}.bias": p["beta"].float()}, strict=False)
    return guarded.to(mlp, DEV)


@MODES
def test_mlp_with_dropout_matches_float64(fgcn_math):
    case = R.mlp_case()
    mlp = _mlp(R.MLP_P).train()
    drop, conv, bn, _ = mlp.layers
    drop.reseed(R.MLP_SEED)
    xg = guarded.to(case["x"].float(), DEV).requires_grad_(True)
    out = mlp(xg)
    n = xg.numel()
    kept = R.unpack(drop.keep_mask.cpu().numpy(), n).reshape(R.MLP_SHAPE)
    assert np.array_equal(kept.reshape(-1), R.keep(n, R.MLP_P, R.MLP_SEED, 0, 0)) and _word(drop.step) == 1
    ref = _cached("mlp", lambda: R.mlp_reference(kept))
    assert R.off_the_kink(ref["pre"]) >= 1e-4
    (out * guarded.to(case["probe"].float(), DEV)).sum().backward()
    errors = {"forward": rel_l2(out.detach().cpu().numpy(), ref["out"].numpy()), "dx": rel_l2(xg.grad.cpu().numpy(), ref["gx"].numpy()),
              "weight": rel_l2(conv.weight.grad.cpu().numpy(), ref["grads"]["weight"].numpy()),
              "gamma": rel_l2(bn.weight.grad.cpu().numpy(), ref["grads"]["gamma"].numpy()),
              "beta": rel_l2(bn.bias.grad.cpu().numpy(), ref["grads"]["beta"].numpy())}
    print(f"[dropout mlp {fgcn_math}] " + ", ".join(f"{k} {e:.2e}" for k, e in errors.items()))
    for k, e in errors.items():
        assert e < 2e-5, (k, e)
    assert float(conv.bias.grad.abs().max()) == 0.0 and float(ref["grads"]["bias"].abs().max()) < 1e-9
    assert int(bn.num_batches_tracked) == 1
    # eval mode: a dropout=0 MLP loaded with the renumbered weights, bit for bit
    plain = _mlp(0)
    plain.load_state_dict({f"layers.{int(k.split('.')[1]) - 1}.{k.split('.', 2)[2]}": v for k, v in mlp.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(mlp.eval()(xg), plain.eval()(xg)) and _word(drop.step) == 1


@MODES
def test_multi_scale_graph_conv_with_dropout_matches_float64(fgcn_math):
    """MS_GCN(dropout=) with two scales and a 3-channel input that travels as 4: the dropped tensor is the scale-major aggregate, one zero pad
    channel per scale group included."""
    from fusion_gcn_amd.models.msg3d.ms_gcn import MultiScale_GraphConv
    case = R.msgcn_case()
    b, t, v, c = R.GCN_SHAPE
    mod = MultiScale_GraphConv(R.GCN_SCALES, c, R.GCN_OUT, R.chain_graph(), dropout=R.GCN_P)
    p = case["params"]
    mod.load_state_dict({"A_res": p["A_res"].float(), "mlp.layers.1.weight": p["weight"].float(), "mlp.layers.1.bias": p["bias"].float(),
                         "mlp.layers.2.weight": p["gamma"].float(), "mlp.layers.2.bias": p["beta"].float()}, strict=False)
    a_powers = mod.A_powers.double().clone()
    mod = guarded.to(mod, DEV).train()
    drop, conv, bn, _ = mod.mlp.layers
    drop.reseed(R.GCN_SEED)
    seen = []
    hook = drop.register_forward_hook(lambda m, args, result: seen.append(result.detach()))
    xg = guarded.to(F.pad(case["x"].float(), (0, 1)).contiguous(), DEV).requires_grad_(True)
    out = mod(xg)
    hook.remove()
    n = b * t * v * R.GCN_SCALES * (c + 1)
    assert seen[0].shape == (b, t, v, R.GCN_SCALES * (c + 1))
    kept = R.unpack(drop.keep_mask.cpu().numpy(), n).reshape(b, t, v, -1)
    assert np.array_equal(kept.reshape(-1), R.keep(n, R.GCN_P, R.GCN_SEED, 0, 0))
    assert not seen[0].view(b, t, v, R.GCN_SCALES, c + 1)[..., c].any()                      # pad channels: zero and still zero
    ref = _cached("msgcn", lambda: R.msgcn_reference(a_powers, kept))
    assert R.off_the_kink(ref["pre"]) >= 1e-4
    assert rel_l2(seen[0].cpu().numpy(), ref["dropped"].numpy()) < 2e-5
    (out * guarded.to(case["probe"].float(), DEV)).sum().backward()
    errors = {"forward": rel_l2(out.detach().cpu().numpy(), ref["out"].numpy()),
              "dx": rel_l2(xg.grad[..., :c].cpu().numpy(), ref["gx"].numpy()),
              "A_res": rel_l2(mod.A_res.grad.cpu().numpy(), ref["grads"]["A_res"].numpy()),
              "weight": rel_l2(conv.weight.grad.cpu().numpy(), ref["grads"]["weight"].numpy()),
              "gamma": rel_l2(bn.weight.grad.cpu().numpy(), ref["grads"]["gamma"].numpy()),
              "beta": rel_l2(bn.bias.grad.cpu().numpy(), ref["grads"]["beta"].numpy())}
    print(f"[dropout ms_gcn {fgcn_math}] " + ", ".join(f"{k} {e:.2e}" for k, e in errors.items()))
    for k, e in errors.items():
        assert e < (2e-5 if k == "forward" else 2e-4), (k, e)
    assert not xg.grad[..., c:].any() and float(conv.bias.grad.abs().max()) == 0.0


# ---- whole models --------------------------------------------------------------------------------------------------------------------
def _gcn(nodes, features, classes, **kw):
    from fusion_gcn_amd.models.mmargcn.gcn import GCN
    torch.manual_seed(3)
    model = guarded.to(GCN(R.ring_adjacency(nodes).float(), (features, nodes), classes, dropout=0.3, gc_model="stgcn", **kw), DEV).train()
    for m in _fused(model):
        m.reseed(1)
    return model


def test_two_models_from_one_seed_take_bit_identical_steps():
    batches = [(guarded.to(R.rnd(4, 1, 24, seed=40 + i).float(), DEV), torch.tensor([0, 3, 1, 4], device=DEV).roll(i)) for i in range(2)]

    def run():
        model = _gcn(24, 1, 5, num_layers=3, inner_feature_dim=16)
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        trace = []
        for x, y in batches:
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(model(x), y)
            loss.backward()
            trace.append((loss.detach().clone(), torch.cat([p.grad.reshape(-1) for p in model.parameters()]).clone()))
            opt.step()
        assert all(_word(m.step) == 2 for m in _fused(model))
        return trace

    first, second = run(), run()
    for (la, ga), (lb, gb) in zip(first, second):
        assert torch.equal(la, lb) and torch.equal(ga, gb) and bool(torch.isfinite(ga).all())
    assert not torch.equal(first[0][1], first[1][1])


def test_graph_step_draws_a_new_mask_per_replay_and_counts_real_steps_only():
    from fusion_gcn_amd.session.procedures import GraphStep
    model = _gcn(16, 3, 4, num_layers=4, inner_feature_dim=8)          # 16 nodes: the smallest graph of tests/test_imu_gcn.py
    drops = _fused(model)
    assert len(drops) == 3
    x, y = guarded.to(R.rnd(4, 3, 16, seed=50).float(), DEV), torch.tensor([0, 1, 2, 3], device=DEV)
    step = GraphStep()
    masks, losses = [], []
    for _ in range(3):
        for p in model.parameters():
            p.grad = None
        _, loss = step.forward(model, F.cross_entropy, x, y)
        step.backward(loss)
        torch.cuda.synchronize()
        masks.append([m.keep_mask.clone() for m in drops])
        losses.append(float(loss))
    assert step.replays == 3 and len(step._recorded) == 1
    assert all(np.isfinite(v) for v in losses) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    for i in range(len(drops)):
        assert not any(torch.equal(masks[a][i], masks[b][i]) for a, b in ((0, 1), (0, 2), (1, 2)))
    assert [_word(m.step) for m in drops] == [3, 3, 3]                   # warm-up and recording were rolled back
    n = masks[0][1].numel() * 8
    for k in range(3):                                                   # ... and replay k drew step k's mask
        assert np.array_equal(masks[k][1].cpu().numpy(), R.pack(R.keep(n, 0.3, 1, 0, k)))


def test_late_fusion_with_dropout_trains_and_evaluates_like_the_model_without():
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    kw = dict(gc_model="stgcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4, inner_feature_dim=64)
    shapes = {"skeleton": (1, 16, 20, 3), "inertial": (8, 6)}
    graph = Graph(utd.skeleton_edges, center_joint=utd.center_joint)
    torch.manual_seed(5)
    model = guarded.to(Model(shapes, 27, graph, mode="skeleton_imu_gcn_late_fusion", dropout=0.2, **kw), DEV).train()
    x = {"skeleton": guarded.to(R.rnd(3, *shapes["skeleton"], seed=60).float(), DEV), "inertial": guarded.to(R.rnd(3, *shapes["inertial"], seed=61).float(), DEV)}
    y = torch.tensor([1, 26, 7], device=DEV)
    loss = F.cross_entropy(model(x), y)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert all(_word(m.step) == 1 for m in _fused(model)) and _fused(model)
    # the same values in a dropout=0 model: the skeleton branch's nn.Dropout modules took every other l<i> slot (l0, l2, ... -> l0, l1, ...)
    plain = guarded.to(Model(shapes, 27, graph, mode="skeleton_imu_gcn_late_fusion", **kw), DEV)

    def renumber(k):
        parts = k.split(".")
        for i, part in enumerate(parts):
            if i and parts[i - 1] == "agcn" and part[0] == "l" and part[1:].isdigit():
                parts[i] = f"l{int(part[1:]) // 2}"
        return ".".join(parts)
    plain.load_state_dict({renumber(k): v for k, v in model.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(model.eval()(x), plain.eval()(x))
