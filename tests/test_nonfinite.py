"""Host side of the non-finite contract (include/fgcn.h "Non-finite values in the inputs"): the comparison of
tests/nonfinite_ref.py on hand-written arrays -- every rule made to fail once and to pass once -- and the CONDITIONS of
tests/test_nonfinite_gpu.py run on the float64 reference alone, so that no assertion there is vacuous: the poisoned oracle really is
non-finite where the GPU test expects a non-finite kernel and finite where it expects containment."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_routes as R
import nonfinite_ref as NF

NAN, INF = float("nan"), float("inf")


# ---- classes / compare ----------------------------------------------------------------------------------------------------------------------
def test_classes_is_the_four_way_map():
    got = NF.classes(torch.tensor([[0.0, NAN, INF], [-INF, -1e38, 3.0]]))
    assert got.dtype == np.uint8 and got.tolist() == [[NF.FINITE, NF.NAN, NF.PINF], [NF.NINF, NF.FINITE, NF.FINITE]]
    assert NF.classes(torch.tensor([NAN, 1.0]).to(torch.bfloat16)).tolist() == [NF.NAN, NF.FINITE]


def test_rule_1_passes_and_fails():
    want = np.array([1.0, NAN, INF, -INF, 2.0])
    ok = NF.compare(np.array([1.0, NAN, INF, -INF, 2.0]), want, "class", 1e-6, "t")
    assert ok.ok and ok.matching == 5 and ok.message == ""
    swallowed = NF.compare(np.array([1.0, 0.0, INF, -INF, 2.0]), want, "class", 1e-6, "t")       # fmaxf(NaN, 0) = 0
    assert not swallowed.ok and (swallowed.swallowed, swallowed.corrupted) == (1, 0) and "(1,)" in swallowed.message and "rule 1" in swallowed.message
    sign = NF.compare(np.array([1.0, NAN, -INF, -INF, 2.0]), want, "class", 1e-6, "t")           # an inf that lost its sign
    assert not sign.ok and (sign.swallowed, sign.corrupted) == (0, 1)
    nan_for_inf = NF.compare(np.array([1.0, NAN, NAN, -INF, 2.0]), want, "class", 1e-6, "t")     # rule 1 wants the class, not "non-finite"
    assert not nan_for_inf.ok and nan_for_inf.corrupted == 1
    spread = NF.compare(np.array([NAN, NAN, INF, -INF, 2.0]), want, "class", 1e-6, "t")          # a NaN where the reference is finite
    assert not spread.ok and spread.corrupted == 1
    off = NF.compare(np.array([1.0, NAN, INF, -INF, 2.1]), want, "class", 1e-6, "t")             # finite positions keep their tolerance
    assert not off.ok and off.corrupted >= 1 and off.err > 1e-2
    bits = NF.compare(np.array([1.0, NAN, INF, -INF, 2.0 + 1e-12]), want, "class", None, "t", exact=True)
    assert not bits.ok and bits.corrupted == 1


def test_rule_3_passes_and_fails():
    want = np.array([1.0, NAN, INF, 2.0, 3.0, 4.0])
    assert NF.compare(np.array([1.0, NAN, INF, 2.0, 3.0, 4.0]), want, "contain", 1e-6, "t").ok
    assert NF.compare(np.array([1.0, INF, NAN, 2.0, 3.0, 4.0]), want, "contain", 1e-6, "t").ok   # NaN against inf need not match
    assert NF.compare(np.array([1.0, NAN, NAN, NAN, 3.0, 4.0]), want, "contain", 1e-6, "t").ok   # finite reference, non-finite kernel: allowed
    sw = NF.compare(np.array([1.0, 0.0, INF, 2.0, 3.0, 4.0]), want, "contain", 1e-6, "t")
    assert not sw.ok and sw.swallowed == 1 and "rule 3" in sw.message
    wrong = NF.compare(np.array([1.0, NAN, INF, 0.0, 0.0, 4.0]), want, "contain", 1e-6, "t")     # the f16x2 flush: finite and wrong
    assert not wrong.ok and wrong.corrupted == 2 and wrong.swallowed == 0 and "(3,), (4,)" in wrong.message
    cos = NF.compare(np.array([1.0, NAN, INF, 2.0, 3.0, 4.1]), want, "contain", 0.98, "t", cosine=True)
    assert cos.ok and cos.err > 0.98
    assert not NF.compare(np.array([1.0, NAN, INF, -2.0, -3.0, 4.0]), want, "contain", 0.98, "t", cosine=True).ok


def test_rule_4_passes_and_fails():
    want = np.array([[1.0, NAN], [2.0, 3.0]])
    clean = np.array([[False, False], [True, True]])
    assert NF.compare(np.array([[NAN, NAN], [2.0, 3.0]]), want, "contain", 1e-6, "t", clean=clean).ok
    sp = NF.compare(np.array([[1.0, NAN], [NAN, 3.0]]), want, "contain", 1e-6, "t", clean=clean)  # rule 3 alone would let this through
    assert not sp.ok and (sp.swallowed, sp.corrupted, sp.spilled) == (0, 0, 1) and "(1, 0)" in sp.message
    fails = []
    NF.check(fails, np.array([[1.0, NAN], [NAN, 3.0]]), want, "contain", 1e-6, "t", clean=clean)
    assert len(fails) == 1


# ---- rule 2: the reference's gate -----------------------------------------------------------------------------------------------------------
def test_torch_relu_keeps_nan_and_passes_the_gradient_at_a_nan_output():
    y = torch.tensor([NAN, INF, -INF, -1.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    out = torch.relu(y)
    assert NF.classes(out.detach()).tolist() == [NF.NAN, NF.PINF, NF.FINITE, NF.FINITE, NF.FINITE, NF.FINITE]
    g, = torch.autograd.grad(out.sum(), y)
    assert g.tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert NF.relu_gate(out.detach()).tolist() == [bool(v) for v in g.tolist()]


def test_pack_sign_image_follows_the_gate():
    from oracle import relu_masks as RM
    t = torch.tensor([NAN, 1.0, -1.0, 0.0, INF, -INF, -0.0, 5.0], dtype=torch.float64).view(1, 8, 1, 1)      # (B, C, T, V): one (b, t, v) row
    assert RM.pack_sign_image(t).tolist() == [0b10010011]
    assert NF.pack_gate(t.reshape(-1)).tolist() == [0b10010011]
    finite = torch.randn(2, 8, 3, 5, dtype=torch.float64)
    assert np.array_equal(RM.pack_sign_image(finite), np.packbits((finite.permute(0, 2, 3, 1) > 0).reshape(-1).numpy(), bitorder="little"))


# ---- the block leg's conditions on the oracle -----------------------------------------------------------------------------------------------
CASES = [c for c in R.CASES if c.name in NF.BLOCK_CASES]


@pytest.mark.parametrize("value", list(NF.POISONS))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_eval_oracle_is_poisoned_in_its_sample_and_clean_in_the_others(case, value):
    ora = NF.oracle_case(case, "eval", NF.block_poison(case, value))
    base = NF.oracle_case(case, "eval")
    s = NF.POISONED_SAMPLE
    others = [b for b in range(R.B) if b != s]
    for name in ("out", "dx") + (() if case.static else ("adj_c",)):
        t = ora[name]
        if not (case.static and name == "dx"):          # (static adjacency: the block is piecewise linear in x, and a NaN output passes its gradient)
            assert not bool(torch.isfinite(t[s]).all()), (name, "the poisoned sample is finite")
        assert bool(torch.isfinite(t[others]).all()), (name, "the poison left its sample")
        # (the poisoned oracle runs on the float32-rounded input the device gets, the plain one on the float64 input: 2^-24 per element)
        assert R.rel_l2(t[others].numpy(), base[name][others].numpy()) < 1e-6, name
    assert any(not np.isfinite(g).all() for g in ora["want"].values())


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_train_oracle_carries_nan_through_the_batch_statistics(case):
    ora = NF.oracle_case(case, "train", NF.block_poison(case, "nan"))
    assert bool(torch.isnan(ora["out"]).any())
    # the BatchNorm behind the spatial stage sees the poisoned rows in every channel: all its channels, and their running statistics, are NaN
    assert bool(torch.isnan(ora["stats"]["gcn1.bn.running_mean"]).all()) and bool(torch.isnan(ora["stats"]["gcn1.bn.running_var"]).all())
    assert bool(torch.isnan(ora["g"]).all()) and bool(torch.isnan(ora["out"]).all())
    assert int(ora["stats"]["gcn1.bn.num_batches_tracked"]) == 1


@pytest.mark.parametrize("mode", R.ALL_MODES)
@pytest.mark.parametrize("phase", R.PHASES)
def test_the_covering_subset_covers(mode, phase):
    sub = NF.covering_subset(mode, phase)
    pool = [e for e in R.matrix(mode, phase) if e.case.name in NF.BLOCK_CASES and not e.half]
    assert all(any(e is o for o in pool) for e in sub)
    assert NF.route_values(sub) == NF.route_values(pool)
    assert {e.case.name for e in sub} == set(NF.BLOCK_CASES)
    for e in sub:                                   # no entry is redundant
        rest = [o for o in sub if o is not e]
        assert not (rest and NF.route_values(rest) == NF.route_values(pool) and {o.case.name for o in rest} == set(NF.BLOCK_CASES))
    print(f"[{mode} {phase}] {len(sub)} of {len(pool)} entries cover {len(NF.route_values(pool))} route values")
    assert len(sub) <= 12


# ---- the loss leg's conditions on torch -----------------------------------------------------------------------------------------------------
def test_cross_entropy_reference_classes():
    z = torch.randn(5, 67, dtype=torch.float64)
    y = torch.tensor([3, 66, 0, 10, 64])
    for value, at_target, want in ((-INF, False, NF.FINITE), (-INF, True, NF.PINF), (INF, False, NF.NAN), (INF, True, NF.NAN),
                                   (NAN, False, NF.NAN), (NAN, True, NF.NAN)):
        zz = z.clone()
        zz[1, 66 if at_target else 65] = value
        zr = zz.requires_grad_(True)
        loss = F.cross_entropy(zr, y, reduction="none")
        g, = torch.autograd.grad(loss.sum(), zr)
        assert NF.classes(loss.detach()).tolist() == [0, want, 0, 0, 0], (value, at_target)
        assert bool(torch.isfinite(g[[0, 2, 3, 4]]).all())
        assert bool(torch.isfinite(g[1]).all()) == (value == -INF), (value, at_target)      # the masking idiom keeps a finite gradient row


# ---- the model leg's conditions on the oracle -----------------------------------------------------------------------------------------------
def test_model_oracle_with_one_nan_coordinate():
    import test_nonfinite_gpu as G
    x, labels, sd = G.model_inputs()
    from oracle import agcn_oracle as O
    with torch.no_grad():
        z_eval = O.model_forward(x.double(), sd, train=False, num_layers=2)
    assert bool(torch.isnan(z_eval[G.BAD_CLIP]).all())
    assert bool(torch.isfinite(z_eval[[i for i in range(x.shape[0]) if i != G.BAD_CLIP]]).all())
    _, loss, grads, _ = O.loss_and_grads(x.double(), labels, sd, train=True, num_layers=2)
    assert bool(torch.isnan(loss)) and all(bool(torch.isnan(g).any()) for g in grads.values() if g is not None and g.abs().sum() != 0)
