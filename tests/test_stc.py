"""Host-side checks of the STC attention module (MS-AAGCN) of the AGCN block: the parameters a model gains with ``attention=True`` and
that it gains nothing without it, the float64 restatement tests/stc_ref.py against autograd's numerical check, the ReLU margins of the
GPU cases' references, and the kernel plan of an attention block."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import stc_ref
import test_block_plan as TP


def _utd_graph():
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.util import Graph
    return Graph(utd.skeleton_edges, center_joint=utd.center_joint)


def _model(module: str, **kw):
    import importlib
    Model = importlib.import_module(f"fusion_gcn_amd.models.{module}").Model
    shape = (1, 16, 20, 3)
    if module == "agcn.agcn":
        return Model({"skeleton": shape}, 27, _utd_graph(), **kw)
    return Model(shape, 27, _utd_graph(), **kw)


@pytest.mark.parametrize("module,first", [("mmargcn.agcn", "l0"), ("agcn.agcn", "l1")])
def test_attention_adds_eight_tensors_behind_gcn1s_others(module, first):
    torch.manual_seed(11)
    plain = _model(module)
    torch.manual_seed(11)
    att = _model(module, attention=True)
    keys, base = list(att.state_dict()), list(plain.state_dict())
    assert [k for k in keys if k.rsplit(".", 2)[-2] not in ("conv_sa", "conv_ta", "fc1c", "fc2c")] == base
    widths = [64] * 4 + [128] * 3 + [256] * 3
    for i, C in enumerate(widths):
        p = f"l{i + int(first[1:])}.gcn1."
        mine = [k for k in keys if k.startswith(p)]
        # registered after everything gcn1 has today, in the stated order
        assert mine[-8:] == [p + k for k in stc_ref.STC_KEYS], mine
        assert mine[:-8] == [k for k in base if k.startswith(p)]
        sd = att.state_dict()
        for k, shape in zip(stc_ref.STC_KEYS, stc_ref.param_shapes(C, 20)):
            assert tuple(sd[p + k].shape) == shape, (p + k, tuple(sd[p + k].shape))
        assert sd[p + "conv_sa.weight"].shape[-1] == 19                      # 20 joints: the even-V rule
        for k in ("conv_sa.bias", "conv_ta.weight", "conv_ta.bias", "fc1c.bias", "fc2c.weight", "fc2c.bias"):
            assert float(sd[p + k].abs().max()) == 0.0, p + k
        for k, std in (("conv_sa.weight", (2.0 / ((C + 1) * 19)) ** 0.5), ("fc1c.weight", (2.0 / C) ** 0.5)):      # xavier / kaiming normal
            assert 0.8 * std < float(sd[p + k].std()) < 1.2 * std, (p + k, float(sd[p + k].std()), std)
    gcn = getattr(att, first).gcn1
    assert gcn.conv_sa.padding == (9,) and gcn.conv_ta.padding == (4,) and gcn.conv_ta.kernel_size == (9,)
    assert getattr(att, first).cfg.attention and not getattr(plain, first).cfg.attention


@pytest.mark.parametrize("module", ["mmargcn.agcn", "agcn.agcn"])
def test_attention_false_is_the_model_without_the_argument(module):
    torch.manual_seed(5)
    a = _model(module)
    after_a = torch.rand(1)
    torch.manual_seed(5)
    b = _model(module, attention=False)
    after_b = torch.rand(1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(after_a, after_b)             # no random number drawn
    # the block's own parameter list, and the draws of an attention model: everything up to a block's gate parameters is the plain model's
    from fusion_gcn_amd import block
    blk = b.l1
    assert block.param_names(blk.cfg) == block.param_names(dataclasses.replace(blk.cfg, attention=True))[:-8]
    assert block.param_names(dataclasses.replace(blk.cfg, attention=True))[-8:] == ["gcn1." + k for k in stc_ref.STC_KEYS]


def test_the_switch_reaches_the_fusion_models():
    from fusion_gcn_amd.models.mmargcn import early_fusion_models as E
    from fusion_gcn_amd.models.mmargcn.rgb_feature_models import agcn_kwargs
    assert "attention" in E._BUILD_SWITCHES
    assert agcn_kwargs({"attention": True})["attention"] is True and agcn_kwargs({})["attention"] is False


@pytest.mark.parametrize("shape", [(2, 5, 6, 8), (2, 5, 7, 8)])
def test_reference_passes_gradcheck(shape):
    """an even and an odd joint count: both sides of the kernel-size rule"""
    from oracle import filler
    B, T, V, C = shape
    g = torch.from_numpy(filler.bellish("g.gradcheck", shape)).requires_grad_(True)
    params = [torch.from_numpy(filler.fill_value_for(f"gradcheck.{k}", s)).requires_grad_(True)
              for k, s in zip(stc_ref.STC_KEYS, stc_ref.param_shapes(C, V))]
    assert params[0].shape[-1] == (5 if V == 6 else 7)
    cap = {}
    stc_ref.stc_ref(g, *params, capture=cap)
    assert stc_ref.least_pre(cap) > 1e-3             # (the numerical check steps by 1e-6: no ReLU decision in reach)
    assert torch.autograd.gradcheck(stc_ref.stc_ref, (g, *params), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_reference_is_the_product_of_the_three_gates():
    """G' = G (1 + s)(1 + tg)(1 + cg) with cm = mean_t (1 + tg) m: the identity the kernels use to skip the third pass over G"""
    case = stc_ref.op_case(stc_ref.OP_SHAPES[0])
    g, (w_sa, b_sa, w_ta, b_ta, w1, b1, w2, b2) = case["g"], case["params"]
    B, T, V, C = g.shape
    F = torch.nn.functional
    s = torch.sigmoid(F.conv1d(g.mean(1).transpose(1, 2), w_sa, b_sa, padding=12)).view(B, 1, V, 1)
    m = (g * (1 + s)).mean(2)
    tg = torch.sigmoid(F.conv1d(m.transpose(1, 2), w_ta, b_ta, padding=4)).view(B, T, 1)
    cm = ((1 + tg) * m).mean(1)
    cg = torch.sigmoid(F.linear(torch.relu(F.linear(cm, w1, b1)), w2, b2)).view(B, 1, 1, C)
    assert float((g * (1 + s) * (1 + tg.view(B, T, 1, 1)) * (1 + cg) - case["out"]).abs().max()) < 1e-12


@pytest.mark.parametrize("shape", stc_ref.OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_cases_decide_no_relu_within_rounding(shape):
    case = stc_ref.op_case(shape)
    print(f"{shape}: salt {stc_ref.op_salt(shape)}, least |pre-activation| {case['least_pre']:.3e}")
    assert case["least_pre"] > stc_ref.PRE_MIN
    assert all(float(p.abs().min()) > 0 for p in case["params"])             # random non-zero values in all eight parameters


@pytest.mark.parametrize("case", stc_ref.BLOCK_CASES, ids=[c.name for c in stc_ref.BLOCK_CASES])
def test_block_cases_decide_no_relu_within_rounding(case):
    for phase in ("train", "eval"):
        ora = stc_ref.block_oracle(case, phase)
        print(f"{case.name} {phase}: salt {stc_ref.block_salt(case)}, least |pre-activation| {ora['least_pre']:.3e}, scalar bias gradients "
              f"cancel {ora['bias_cond']:.1f}-fold at most")
        assert ora["least_pre"] > stc_ref.PRE_MIN and ora["bias_cond"] < stc_ref.COND_MAX
        for k in stc_ref.STC_KEYS:                   # every gate parameter has a gradient of its own in the oracle
            assert float(np.abs(ora["want"]["gcn1." + k]).max()) > 0, k


SIX = ("fuse_g", "bn_sums_in_dgrad", "g_bf16", "u_bf16", "dg_bf16", "dx_bf16")


@pytest.mark.parametrize("mode", TP.MODES)
def test_attention_block_plans_no_fusion_across_the_gate(mode):
    """over test_block_plan's blocks, joint counts and option sets, in every phase: the six fields are False in an attention block, and
    its plan differs from the plain block's in nothing else than what those fields explain"""
    from fusion_gcn_amd import block, ops, routes
    from fusion_gcn_amd.models.mmargcn.agcn import SpatialTemporalConv
    plans = differ = 0
    with ops.context(mode):
        for cin, cout, stride, residual, static, T in TP.BLOCKS:
            mod = SpatialTemporalConv(cin, cout, np.zeros((3, 25, 25), np.float32), stride=stride, residual=residual, static_adjacency=static,
                                      attention=True)
            cfg = mod.cfg
            assert cfg.attention
            plain = dataclasses.replace(cfg, attention=False)
            forms = block.pack_weights({n: mod._tensor(n) for n in block.param_names(cfg)}, cfg)
            for (phase, (train, inference)), V, (name, o) in itertools.product(TP.PHASES.items(), TP.JOINTS, TP.option_sets(mode)):
                half = bool(train and mode == "bf16" and o.half_storage["bf16"] and o.half_activations["bf16"] and V <= 32)
                for x_bf16 in ((False, True) if half else (False,)):
                    kw = dict(x_bf16=x_bf16, train=train, inference=inference, pool_groups=0, out_half=x_bf16, forms=forms, mode=mode, paths=o, kt=9)
                    pl = routes.plan_block(cfg, 128, T, V, **kw)
                    assert not any(getattr(pl, f) for f in SIX), (phase, V, name, pl)
                    TP.check(pl, cfg, mode, train)
                    ref = routes.plan_block(plain, 128, T, V, **kw)
                    differ += any(getattr(ref, f) for f in SIX)
                    plans += 1
    print(f"{mode}: {plans} plans, {differ} of them differ from the plain block's")
    assert mode == "f32" or differ > 0           # the sweep reaches plans the switch really changes
