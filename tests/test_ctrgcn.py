"""Host-side checks of ``model: ctrgcn``: it resolves, its state dict is the stated one with the stated initial values, the float64
restatement tests/ctrgcn_ref.py agrees with itself (two writings of the graph convolution) and with autograd's numerical check and can see
a transposed topology, and every fgcn_ctr_* entry point refuses what it does not take before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctrgcn_ref as R
from oracle import filler

SHAPE, CLASSES = (2, 16, 25, 3), 7
BADARG, ALIGN = -1, -2


def _graph():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.util import Graph
    return Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)


def _model(**kw):
    from fusion_gcn_amd.util.dynamic_import import import_model
    return import_model("ctrgcn")({"skeleton": SHAPE}, CLASSES, _graph(), **kw)


def test_import_model_resolves_ctrgcn():
    from fusion_gcn_amd.models.ctrgcn.ctrgcn import Model
    from fusion_gcn_amd.util.dynamic_import import import_model
    assert import_model("ctrgcn") is Model and import_model("CTRGCN") is Model


def test_state_dict_keys_order_shapes_and_initial_values():
    from fusion_gcn_amd.util.partition_strategy import GraphPartitionStrategy
    torch.manual_seed(3)
    model = _model()
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.expected_keys(SHAPE, CLASSES)
    pa = torch.from_numpy(GraphPartitionStrategy().get_adjacency_matrix_array(_graph()).astype(np.float32))
    for i in range(1, 11):
        g = f"l{i}.gcn1."
        assert float(sd[g + "alpha"]) == 0.0 and torch.equal(sd[g + "PA"], pa), g
        assert torch.all(sd[g + "bn.weight"] == 1e-6) and torch.all(sd[g + "bn.bias"] == 0), g
        assert (g + "down.0.weight" in sd) == (i in (1, 5, 8)) and (f"l{i}.residual.conv.weight" in sd) == (i in (5, 8))
    for k, v in sd.items():
        if v.dim() == 4:                             # a convolution: kaiming normal over its fan-out, zero bias
            assert float(sd[k[:-6] + "bias"].abs().max()) == 0.0, k
            std = (2.0 / (v.shape[0] * v.shape[2])) ** 0.5
            assert v.numel() < 2000 or 0.85 * std < float(v.std()) < 1.15 * std, (k, float(v.std()), std)
        elif k.endswith("weight") and v.dim() == 1 and ".tcn1." in k:
            assert 0.9 < float(v.min()) and float(v.max()) < 1.1 and float(v.std()) > 0.005, k          # normal(1, 0.02)
        elif k.endswith("weight") and v.dim() == 1 and ".gcn1.bn." not in k:
            assert torch.all(v == 1), k
    assert 0.8 * (2 / CLASSES) ** 0.5 < float(sd["fc.weight"].std()) < 1.2 * (2 / CLASSES) ** 0.5
    # the reference modules carry the same keys: a product state dict loads into them (what the GPU tests rely on)
    ref = R.RefModel(SHAPE, CLASSES)
    assert set(ref.state_dict()) == set(sd)
    ref.load_state_dict(sd)


def test_state_dict_round_trips_and_adaptive_false_drops_pa():
    a = _model()
    filler.fill_state_dict(a.state_dict(), skip=("alpha",))
    b = _model()
    b.load_state_dict(a.state_dict())
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    fixed = _model(adaptive=False)
    keys = list(fixed.state_dict())
    assert keys == [k for k, _ in R.expected_keys(SHAPE, CLASSES, adaptive=False)] and not any(k.endswith("PA") for k in keys)
    assert not any(n.endswith(("PA", ".A")) for n, _ in fixed.named_parameters())
    assert torch.equal(fixed.l3.gcn1.A, b.l1.gcn1.PA.detach() * 0 + _model().l3.gcn1.PA.detach()) and not fixed.l3.gcn1.A.requires_grad


def _unit_state(cin, cout, V, seed="host"):
    mod = R.RefUnitGCN(cin, cout, V).double()
    R.fill(mod, 0, prefix=f"{seed}.")
    return {k: v.detach().clone().requires_grad_(True) for k, v in mod.named_parameters() if not k.startswith(("bn.", "down."))}


def test_the_two_writings_of_the_graph_convolution_agree():
    B, T, V, cin, cout = 2, 5, 7, 16, 24
    sd = _unit_state(cin, cout, V)
    x = torch.from_numpy(filler.bellish("x.two", (B, T, V, cin))).double().requires_grad_(True)
    probe = torch.from_numpy(filler.uniform("probe.two", (B, T, V, cout), -1, 1)).double()
    y_cl = R.gc_cl(x, sd)
    g_cl = torch.autograd.grad((y_cl * probe).sum(), [x] + list(sd.values()))
    y_nchw = R.gc_nchw(x.permute(0, 3, 1, 2), sd).permute(0, 2, 3, 1)
    g_nchw = torch.autograd.grad((y_nchw * probe).sum(), [x] + list(sd.values()))
    assert float((y_cl - y_nchw).abs().max()) < 1e-12
    for k, a, b in zip(["x"] + list(sd), g_cl, g_nchw):
        assert float((a - b).abs().max()) < 1e-12 * max(1.0, float(b.abs().max())), k
        assert float(b.abs().max()) > 0, k


def test_graph_convolution_passes_gradcheck():
    B, T, V, cin, cout = 2, 3, 5, 16, 8
    sd = _unit_state(cin, cout, V, "gradcheck")
    keys = list(sd)
    x = torch.from_numpy(filler.bellish("x.gradcheck.ctr", (B, T, V, cin))).double().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x, *p: R.gc_cl(x, dict(zip(keys, p))), (x, *sd.values()), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("case", R.OP_CASES, ids=lambda c: R.tag_of(*c))
def test_op_inputs_see_a_transposed_topology(case):
    """x1 indexes the output joint, x2 the joint summed over: with the roles swapped (and negated, so that only the transposition of the
    refinement differs) the output moves by a relative 0.1 or more"""
    ref = R.op_case(case)
    x3, x12, w4, b4, alpha, pa = ref["inputs"]
    half = x12.shape[-1] // 2
    swapped = torch.cat([-x12[..., half:], -x12[..., :half]], -1)
    y = R.op_ref(x3, swapped, w4, b4, alpha, pa)
    rel = float((y - ref["y"]).norm() / ref["y"].norm())
    print(f"{case}: salt {R.op_salt(case)}, alpha terms cancel {ref['cond']:.1f}-fold, transposed refinement moves y by {rel:.2f}")
    assert rel >= 0.1
    assert ref["cond"] < R.COND_MAX and all(float(g.abs().max()) > 0 for g in ref["grads"])


def test_every_entry_point_refuses_what_it_does_not_take():
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(B=2, T=4, V=25, C=64, R=8)

    def agg(fn, B, T, V, Cc, Rr, ptrs=None):
        return fn(*(ptrs or [p] * 7), B, T, V, Cc, Rr, None)
    bad = [dict(V=33), dict(C=96), dict(C=576), dict(R=6), dict(R=68), dict(B=65536), dict(T=1 << 20, V=32, C=512)]
    for change in bad:
        d = {**ok, **change}
        for fn in (lib.fgcn_ctr_aggregate, lib.fgcn_ctr_bwd_dx3):
            assert agg(fn, d["B"], d["T"], d["V"], d["C"], d["R"]) == BADARG, change
        if "R" not in change:
            assert lib.fgcn_ctr_bwd_da(p, p, p, d["B"], d["T"], d["V"], d["C"], None) == BADARG, change
        if "T" not in change:
            assert lib.fgcn_ctr_bwd_small(*[p] * 11, d["B"], d["V"], d["C"], d["R"], None) == BADARG, change
            assert lib.fgcn_ctr_param_grads(*[p] * 9, d["B"], d["V"], d["C"], d["R"], None) == BADARG, change
        if "C" not in change and "T" not in change:
            assert lib.fgcn_ctr_tanh(p, p, d["B"], d["V"], d["R"], None) == BADARG, change
    assert lib.fgcn_ctr_mean_t(p, p, 2, 4, 25, 6, None) == BADARG and lib.fgcn_ctr_mean_t(p, p, 2, 4, 33, 4, None) == BADARG
    assert lib.fgcn_ctr_mean_t_bwd(p, p, 2, 4, 25, 6, 0, None) == BADARG and lib.fgcn_ctr_mean_t_bwd(p, p, 65536, 4, 25, 4, 0, None) == BADARG
    # null pointers, each in turn
    for fn, n, tail in ((lib.fgcn_ctr_aggregate, 7, (2, 4, 25, 64, 8)), (lib.fgcn_ctr_bwd_dx3, 7, (2, 4, 25, 64, 8)), (lib.fgcn_ctr_bwd_da, 3, (2, 4, 25, 64)),
                        (lib.fgcn_ctr_bwd_small, 11, (2, 25, 64, 8)), (lib.fgcn_ctr_param_grads, 9, (2, 25, 64, 8)), (lib.fgcn_ctr_tanh, 2, (2, 25, 8)),
                        (lib.fgcn_ctr_mean_t, 2, (2, 4, 25, 4)), (lib.fgcn_ctr_mean_t_bwd, 2, (2, 4, 25, 4, 0))):
        for i in range(n):
            ptrs = [p] * n
            ptrs[i] = None
            assert fn(*ptrs, *tail, None) == BADARG, (fn.__name__, i)
            assert b"null pointer" in lib.fgcn_last_error()
    # tensors read in 16-byte groups
    for i in (0, 1, 2):                              # x3 / dy, th, w4
        ptrs = [p] * 7
        ptrs[i] = p + 4
        assert agg(lib.fgcn_ctr_aggregate, 2, 4, 25, 64, 8, ptrs) == ALIGN and agg(lib.fgcn_ctr_bwd_dx3, 2, 4, 25, 64, 8, ptrs) == ALIGN
    assert lib.fgcn_ctr_bwd_da(p, p + 4, p, 2, 4, 25, 64, None) == ALIGN
    assert lib.fgcn_ctr_mean_t(p + 4, p, 2, 4, 25, 4, None) == ALIGN and lib.fgcn_ctr_mean_t_bwd(p, p + 4, 2, 4, 25, 4, 0, None) == ALIGN
    # the host geometry queries
    assert lib.fgcn_ctr_chunk() >= 1 and lib.fgcn_ctr_split_frames(0, 4, 25, 64) == 0
    assert lib.fgcn_ctr_split_frames(2, 4, 33, 64) == 0 and lib.fgcn_ctr_split_frames(2, 4, 25, 96) == 0 and lib.fgcn_ctr_split_frames(65536, 4, 25, 64) == 0
    assert lib.fgcn_ctr_split_frames(2, 37, 25, 64) == 19
    for B, T, V, Cc in ((3, 13, 25, 64), (128, 64, 25, 64), (1, 300, 32, 512), (65535, 1, 5, 64)):
        fps = lib.fgcn_ctr_split_frames(B, T, V, Cc)
        assert 1 <= fps <= T and (T + fps - 1) // fps <= 65535, (B, T, V, Cc, fps)
