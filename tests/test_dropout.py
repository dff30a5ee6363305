"""``dropout=`` in the IMU graph convolution and the MS-G3D MLP, the part that needs no GPU: the generator's known
answers through the C ABI, the host-side argument checks of fgcn_dropout_fwd / _bwd / fgcn_rng_advance (they precede any launch), the
statistics of the keep rule, the constructors that used to raise and their state-dict keys, and the condition under which the GPU tests
of tests/test_dropout_gpu.py compare gradients: the float64 references stay off the ReLU's kink.  References: tests/dropout_ref.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dropout_ref as R
from fusion_gcn_amd import _lib, build

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _lib_philox(lib, ctr, key):
    out = (C.c_uint * 4)()
    assert lib.fgcn_philox4x32_10((C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), out) == 0
    return list(out)


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(lib, ctr, key, want):
    want = [int(w, 16) for w in want.split()]
    assert _lib_philox(lib, ctr, key) == want
    assert R.philox4x32_10(ctr, key).tolist() == want                  # the tests' own generator agrees with the published vectors too


def test_library_and_numpy_generators_agree_on_random_counters(lib):
    rng = np.random.default_rng(5)
    ctrs, keys = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64), rng.integers(0, 2 ** 32, (64, 2), dtype=np.uint64)
    for ctr, key in zip(ctrs.tolist(), keys.tolist()):
        assert _lib_philox(lib, ctr, key) == R.philox4x32_10(ctr, key).tolist()
    assert lib.fgcn_philox4x32_10(None, (C.c_uint * 2)(), (C.c_uint * 4)()) == -1 and b"null pointer" in lib.fgcn_last_error()


def test_host_side_validation(lib):
    """include/fgcn.h's list, each FGCN_E_BADARG before any launch (no device is touched: this runs without one)."""
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16

    def fwd(x=p, y=p + 64, mask=p + 128, n=16, prob=0.5, step=p + 192):
        return lib.fgcn_dropout_fwd(x, y, mask, n, prob, 7, 0, step, None)

    def bwd(dy=p, mask=p + 128, dx=p + 64, n=16, prob=0.5):
        return lib.fgcn_dropout_bwd(dy, mask, dx, n, prob, None)

    for call in (fwd, bwd):
        for n in (0, -4, 6, 2 ** 34, 2 ** 34 + 4):
            assert call(n=n) == -1 and b"n=" in lib.fgcn_last_error(), n
        for prob in (-0.1, 1.0, 1.5, math.nan, math.inf, -math.inf):
            assert call(prob=prob) == -1 and b"p=" in lib.fgcn_last_error(), prob
    for name in ("x", "y", "mask", "step"):
        assert fwd(**{name: None}) == -1 and b"null pointer" in lib.fgcn_last_error(), name
    for name in ("dy", "mask", "dx"):
        assert bwd(**{name: None}) == -1 and b"null pointer" in lib.fgcn_last_error(), name
    for name in ("x", "y"):
        assert fwd(**{name: p + 4}) == -1 and b"aligned" in lib.fgcn_last_error(), name
    for name in ("dy", "dx"):
        assert bwd(**{name: p + 8}) == -1 and b"aligned" in lib.fgcn_last_error(), name
    assert fwd(step=p + 4) == -1 and b"aligned" in lib.fgcn_last_error()
    assert lib.fgcn_rng_advance(None, None) == -1 and lib.fgcn_rng_advance(p + 4, None) == -1


def test_ops_have_no_fallback_off_the_gpu():
    """Host tensors raise FgcnError (without a device: the device check does), nothing is computed by torch instead."""
    from fusion_gcn_amd import fops, ops
    x, step = torch.zeros(8), torch.zeros(1, dtype=torch.uint64)
    with pytest.raises(_lib.FgcnError):
        ops.dropout_fwd(x, 0.5, 1, 0, step)
    with pytest.raises(_lib.FgcnError):
        ops.dropout_bwd(x, torch.zeros(1, dtype=torch.uint8), 0.5)
    with pytest.raises(_lib.FgcnError):
        ops.rng_advance(step)
    drop = fops.FusedDropout(0.5)
    with pytest.raises(_lib.FgcnError):
        drop(x)
    assert drop.eval()(x) is x and fops.dropout(x, drop, 0.0, True) is x          # nothing to do: the input itself, no launch
    assert not fops.dropout(torch.ones(8), drop, 1.0, True).any()                 # p == 1: zeros, as torch's
    with pytest.raises(ValueError):
        fops.dropout(x, drop, 1.5, True)


def test_keep_share_of_the_numpy_generator():
    p, n = 0.3, 2 ** 20
    kept = R.keep(n, p, seed=0x1234567887654321, site=3, step=2 ** 32 + 9)
    assert abs(float(kept.mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)
    other = R.keep(n, p, seed=0x1234567887654321, site=3, step=2 ** 32 + 10)
    assert 0.3 < float((kept != other).mean()) < 0.55                            # another step: another mask (2 p (1 - p) = 0.42 of the bits)
    assert R.keep(16, 0.0, 1, 0, 0).all()
    assert np.array_equal(R.unpack(R.pack(kept[:20]), 20), kept[:20]) and R.pack(kept[:20]).size == 3


def test_fused_dropout_module_surface():
    from fusion_gcn_amd.fops import FusedDropout
    drop = FusedDropout(0.4)
    assert isinstance(drop, torch.nn.Dropout) and isinstance(drop, torch.nn.modules.dropout._DropoutNd) and drop.p == 0.4
    assert list(drop.state_dict()) == [] and [n for n, _ in drop.named_buffers()] == ["step"]       # a non-persistent buffer
    assert drop.step.dtype == torch.uint64 and drop.step.numel() == 1 and int(drop.step.item()) == 0
    assert drop.seed is None and drop.keep_mask is None
    drop.reseed(2 ** 64 + 5, site=7)
    assert (drop.seed, drop.site) == (5, 7) and int(drop.step.item()) == 0
    with pytest.raises(ValueError):
        FusedDropout(1.5)


def test_graph_convolution_constructors_take_dropout():
    from fusion_gcn_amd.fops import FusedDropout
    from fusion_gcn_amd.models.mmargcn.gcn import GCN
    from fusion_gcn_amd.models.mmargcn.graph_convolution import AGCNGraphConvolution, STGCNGraphConvolution
    adj = R.ring_adjacency(8).float()
    layer = STGCNGraphConvolution(8, 8, adj, dropout=0.5)
    assert isinstance(layer.dropout, FusedDropout) and layer.dropout.p == 0.5
    assert STGCNGraphConvolution(8, 8, adj).dropout is None and STGCNGraphConvolution(8, 8, adj, dropout=0.0).dropout is None
    assert sorted(layer.state_dict()) == sorted(STGCNGraphConvolution(8, 8, adj).state_dict())
    adj24 = R.ring_adjacency(24).float()
    with_p, without = (GCN(adj24, (1, 24), 5, dropout=p, gc_model="stgcn", num_layers=3) for p in (0.3, 0.0))
    assert list(with_p.state_dict()) == list(without.state_dict())
    assert with_p.gc1.dropout is None and with_p.gc2.dropout.p == 0.3 and with_p.gc3.dropout.p == 0.3      # the input layer has none
    # the reference's AGCN graph convolution takes `dropout` and ignores it: so does ours
    agcn = AGCNGraphConvolution(8, 16, np.stack([np.eye(8)] * 3), dropout=0.5)
    assert not any(isinstance(m, torch.nn.Dropout) for m in agcn.modules())


def test_late_fusion_model_with_dropout_builds():
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.fops import FusedDropout
    from fusion_gcn_amd.models.mmargcn.mmargcn import Model
    from fusion_gcn_amd.util import Graph
    kw = dict(gc_model="stgcn", graph_node_format="node_per_sensor", num_signals=2, num_layers=4, inner_feature_dim=64)
    shapes = {"skeleton": (1, 16, 20, 3), "inertial": (8, 6)}
    graph = Graph(utd.skeleton_edges, center_joint=utd.center_joint)
    model = Model(shapes, 27, graph, mode="skeleton_imu_gcn_late_fusion", dropout=0.2, **kw)
    fused = [m for m in model.modules() if isinstance(m, FusedDropout)]
    plain = [m for m in model.modules() if isinstance(m, torch.nn.Dropout) and not isinstance(m, FusedDropout)]
    assert fused and all(m.p == 0.2 for m in fused)                       # the IMU branch
    assert plain and all(m.p == 0.2 for m in plain)                       # the skeleton branch keeps torch's module between its blocks
    # (the skeleton branch's Dropout modules take `l<i>` slots of their own and hold no state: same parameter and buffer values either way)
    imu_keys = [k for k in model.state_dict() if "imu_gcn" in k]
    ref_keys = [k for k in Model(shapes, 27, graph, mode="skeleton_imu_gcn_late_fusion", **kw).state_dict() if "imu_gcn" in k]
    assert imu_keys == ref_keys
    imu = Model({"inertial": (8, 6)}, 5, None, mode="imu_gcn", dropout=0.3, **kw)
    assert any(isinstance(m, FusedDropout) for m in imu.modules())


def test_mlp_layouts_and_keys():
    from fusion_gcn_amd.fops import FusedDropout
    from fusion_gcn_amd.models.msg3d.mlp import MLP
    from fusion_gcn_amd.models.msg3d.ms_gcn import MultiScale_GraphConv
    from fusion_gcn_amd.models.msg3d.ms_gtcn import SpatialTemporal_MS_GCN
    conv, bn = ("weight", "bias"), ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    want = [f"layers.{i}.{k}" for i, ks in ((1, conv), (2, bn), (5, conv), (6, bn)) for k in ks]
    mlp = MLP(16, [32, 32], dropout=0.25)
    assert list(mlp.state_dict()) == want
    assert [type(m) for m in mlp.layers][0::4] == [FusedDropout, FusedDropout] and len(mlp.layers) == 8
    assert list(MLP(16, [32]).state_dict()) == [f"layers.{i}.{k}" for i, ks in ((0, conv), (1, bn)) for k in ks]
    assert len(MLP(16, [32], dropout=0.001).layers) == 3                          # the reference's threshold: dropout > 0.001
    a = np.zeros((6, 6))
    a[np.arange(5), np.arange(1, 6)] = a[np.arange(1, 6), np.arange(5)] = 1.0
    assert "mlp.layers.1.weight" in MultiScale_GraphConv(2, 3, 8, a, dropout=0.25).state_dict()
    assert "mlp.layers.1.weight" in SpatialTemporal_MS_GCN(3, 8, a, 2, 3, dropout=0.25).state_dict()


@pytest.mark.parametrize("kind", list(R.GC_CASES))
def test_graph_convolution_reference_stays_off_the_relu_kink(kind):
    """What the GPU comparison of tests/test_dropout_gpu.py needs, from the float64 reference alone: with the mask the layer will draw
    (seed GC_SEED, site 0, step 0) no pre-ReLU value lies within 1e-4 of zero, so float32 has no ReLU decision to take differently."""
    o = R.GC_CASES[kind][1]
    kept = R.keep(R.B * R.V * o, R.GC_P, R.GC_SEED, 0, 0).reshape(R.B, R.V, o)
    ref = R.gc_reference(kind, kept)
    assert R.off_the_kink(ref["pre"], kept if kind == "none" else None) >= 1e-4
    assert 0.3 < kept.mean() < 0.7


def test_mlp_reference_stays_off_the_relu_kink():
    kept = R.keep(int(np.prod(R.MLP_SHAPE)), R.MLP_P, R.MLP_SEED, 0, 0).reshape(R.MLP_SHAPE)
    assert R.off_the_kink(R.mlp_reference(kept)["pre"]) >= 1e-4


def test_multi_scale_graph_conv_reference_stays_off_the_relu_kink():
    from fusion_gcn_amd.models.msg3d.ms_gcn import k_hop_stack
    b, t, v, c = R.GCN_SHAPE
    kept = R.keep(b * t * v * R.GCN_SCALES * (c + 1), R.GCN_P, R.GCN_SEED, 0, 0).reshape(b, t, v, -1)
    ref = R.msgcn_reference(torch.from_numpy(k_hop_stack(R.chain_graph(), R.GCN_SCALES)).double(), kept)
    assert R.off_the_kink(ref["pre"]) >= 1e-4
    assert not ref["dropped"].view(b, t, v, R.GCN_SCALES, c + 1)[..., c].any()                  # pad channels: zero before, zero after
