"""NaN and inf IN the kernels' inputs, on the MI355X, against the float64 references of the existing kernel, block, loss and model tests run
on the same input with the same non-finite element in it (include/fgcn.h "Non-finite values in the inputs").

  rule 1  elementwise kernels and epilogues give the reference's class (finite / NaN / +inf / -inf) at every position;
  rule 2  the backward's ReLU gate is torch's `grad if !(y <= 0) else 0`, from the sign image and from `out`: a NaN output passes its gradient;
  rule 3  contractions are non-finite wherever the reference is, and where it is finite they are within the unpoisoned tolerance or non-finite;
  rule 4  eval phase: the samples other than the poisoned one are finite (f16x2 with an inf poison: rule 3 alone -- an inf takes its scaling block);
  rule 5  a route that skips the structural zeros of a constant matrix by contract (the SpMM route) has torch's sparse product as its reference.

tests/nonfinite_ref.py holds the comparison; tests/test_nonfinite.py proves on the host that the poisoned references are non-finite and finite
where the assertions here need them to be.  Poisoned inputs are ordinary data: nothing here can address memory with them.  Every kernel call
runs on guarded allocations (tests/guarded.py), so a route that stores past a tensor while it carries a NaN fails too."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_routes as R
import guarded
import nonfinite_ref as NF
from guarded import guarded_allocations  # noqa: F401  (the fixture)
from test_block_routes_gpu import tolerances as block_tolerances
from test_kernels_gpu import FWD_TOL, _eval_vec, ref_rows_conv
from test_loss_options_gpu import reference as ce_reference
from test_loss_options_gpu import run as ce_run

pytestmark = pytest.mark.gpu
guard = pytest.mark.usefixtures("guarded_allocations")       # (the block leg's BlockRun brings its own Guard)
DEV = torch.device("cuda:0")
VALUES = list(NF.POISONS)
BWD_TOL = 2e-5              # test_batchnorm_epilogue_forward_backward's bound on da / db
BF16_STORE = 2.0 ** -9      # a bfloat16 store rounds to nearest: half an ulp of an 8-bit significand per element, hence also in relative L2
CE_TOL = 2e-6               # tests/test_loss_options_gpu.py
RED_TOL = 2e-5              # tests/test_kernels_gpu.py: per-channel sums over the rows


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def f32(t):
    """the float32 rounding of a float64 tensor, as float64: what the device gets"""
    return t.float().double()


def bf(t):
    return t.float().to(torch.bfloat16).double()


def put(t, dtype=None):
    return guarded.put(t.float(), dtype, device=DEV)


def raise_all(fails):
    assert not fails, "\n".join(fails)


def mask_bits(mask: torch.Tensor) -> np.ndarray:
    return np.unpackbits(mask.cpu().numpy(), bitorder="little").astype(bool)


def check_sign_image(fails, mask, y_ref: torch.Tensor, where: str):
    """rule 2 on a sign image: bit e = !(y[e] <= 0) of the reference's pre-gate value, wherever that value is not within 1e-5 of zero (a
    float32 kernel may decide the other way there) -- in particular at every NaN and inf"""
    y = y_ref.reshape(-1)
    decided = ~(y.abs() <= 1e-5)
    got, want = torch.from_numpy(mask_bits(mask)), NF.relu_gate(y)
    bad = (got != want) & decided
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        fails.append(f"{where}: rule 2 broken: {int(bad.sum())} sign-image bits differ, first at flat element {i}: y = {float(y[i])!r}, bit {bool(got[i])}")


# =============================================================================================================================================
# elementwise leg
# =============================================================================================================================================
def positions(rows, C):
    """the first element, the last element of the last four- / eight-group, and an element of the ODD lane of a pair that shares a sign byte"""
    n = rows * C
    return {"first": 0, "last": n - 1, "pair": (n // 2) // 8 * 8 + 5}


def vec4(C, seed):
    """(4, C) = mean, rstd, scale, shift as fgcn_bn_finalize / fgcn_bn_eval_coeffs lay them out"""
    return _eval_vec(C, seed).double()


def bn_act_ref(a, va, b, vb, res):
    y = a * va[2] + va[3]
    if res == 1:
        y = y + b
    elif res == 2:
        y = y + b * vb[2] + vb[3]
    return y


# name -> (math mode, rows, C, bfloat16 inputs, bfloat16 output): the four-wide float32 kernel, its bfloat16-output form, the typed four-wide
# form (C % 8 != 0) with either output, the eight-wide form (C % 8 == 0) that stores through bfloat16
BN_FORMS = {"f32": ("f32", 333, 64, False, False), "o16": ("bf16", 333, 64, False, True), "typed4": ("bf16", 334, 12, True, False),
            "typed4_o16": ("bf16", 334, 12, True, True), "typed8": ("bf16", 333, 64, True, True), "typed8_o32": ("bf16", 333, 64, True, False)}


def entries(res):
    """(operand the poison enters through, position name) -- every operand once, every position at least once"""
    out = [("a", "first"), ("a", "last"), ("a", "pair"), ("scale_a", "last"), ("shift_a", "pair")]
    if res:
        out += [("b", "first"), ("b", "last"), ("b", "pair")]
    if res == 2:
        out += [("scale_b", "first"), ("shift_b", "last")]
    return out


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("form", list(BN_FORMS))
def test_bn_act_and_its_backward_keep_the_class(form, res, value):
    """fgcn_bn_act in RES 0/1/2, with and without the sign image, and fgcn_bn_act_bwd_apply gated from the image and from `out`: rule 1 on the
    output, rule 2 on the image and on da / db, for a poison in the pre-activation, the residual, and the per-channel scale and shift"""
    from fusion_gcn_amd import ops
    mode, rows, C, in16, o16 = BN_FORMS[form]
    rd = bf if in16 else f32
    a0, b0, d0 = rd(rnd(rows, C, seed=1) * 1.7 + 0.3), rd(rnd(rows, C, seed=2)), rd(rnd(rows, C, seed=3))
    va0, vb0 = vec4(C, 10), vec4(C, 20)
    pos, fails = positions(rows, C), []
    dt = torch.bfloat16 if in16 else None
    out_tol = FWD_TOL + (BF16_STORE if o16 else 0.0)
    with ops.math_mode(mode):
        for enter, pname in entries(res):
            r, c = divmod(pos[pname], C)
            a, b, va, vb = a0.clone(), b0.clone(), va0.clone(), vb0.clone()
            if enter == "a":
                a[r, c] = NF.POISONS[value]
            elif enter == "b":
                b[r, c] = NF.POISONS[value]
            else:
                (va if enter.endswith("_a") else vb)[2 if enter.startswith("scale") else 3, c] = NF.POISONS[value]
            where = f"[bn_act {form} res={res} {value} in {enter} at {pname} ({r}, {c})]"
            ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y = bn_act_ref(ar, va, br, vb, res)
            want = torch.relu(y)
            grads = torch.autograd.grad((want * d0).sum(), [ar] + ([br] if res else []))
            ag, bg = put(a, dt), (put(b, dt) if res else None)
            vag, vbg = put(va), (put(vb) if res == 2 else None)
            out, mask = ops.bn_act(ag, vag, bg, vbg, relu=True, sign_mask=True, out_bf16=o16)
            plain = ops.bn_act(ag, vag, bg, vbg, relu=True, out_bf16=o16)
            if not torch.equal(out.view(torch.int16 if o16 else torch.int32), plain.view(torch.int16 if o16 else torch.int32)):
                fails.append(f"{where}: the kernel with the sign image and the one without give different bits")
            NF.check(fails, out.float(), want.detach(), "class", out_tol, where + " out")
            check_sign_image(fails, mask, y.detach(), where + " sign image")
            # backward: the ORACLE's decisions as the gate (image, and `out` where the form reads it), so that rule 2 is all that can differ
            bits = guarded.to(torch.from_numpy(NF.pack_gate(want.detach())), DEV)
            gates = [("image", None, bits)] + ([] if in16 else [("out", put(want.detach()), None)])
            for gname, gate_out, gate_bits in gates:
                da, db, _ = ops.bn_act_bwd(put(d0, dt), gate_out, ag, vag, bg, vbg, res_mode=res, relu=True, train=False, sign_mask=gate_bits,
                                           need_sums=False, da_bf16=o16 and in16)
                NF.check(fails, da.float(), grads[0], "class", BWD_TOL + (BF16_STORE if (o16 and in16) else 0.0), f"{where} da (gate from the {gname})")
                if res:
                    NF.check(fails, db.float(), grads[1], "class", BWD_TOL, f"{where} db (gate from the {gname})")
                if not in16:
                    # the reduction pass (fgcn_bn_act_bwd_reduce) under the same gate: sums = sum dP, sum dP * a_hat, sum dP * b_hat per channel,
                    # dP = dout where the gate is open -- at a NaN output it is (rule 2); a closed gate there would drop one dout from the sums
                    _, _, sums = ops.bn_act_bwd(put(d0), gate_out, ag, vag, bg, vbg, res_mode=res, relu=True, train=False, sign_mask=gate_bits,
                                                need_sums=True)
                    dp = d0 * NF.relu_gate(want.detach())
                    ref = [dp.sum(0), (dp * (a - va[0]) * va[1]).sum(0)] + ([(dp * (b - vb[0]) * vb[1]).sum(0)] if res == 2 else [])
                    NF.check(fails, sums[:len(ref)], torch.stack(ref), "class", RED_TOL, f"{where} sums (gate from the {gname})")
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("res", [0, 1, 2])
@pytest.mark.parametrize("in16", [False, True], ids=["f32", "typed"])
def test_pooled_epilogue_keeps_the_class_and_does_not_mix_groups(in16, res, value):
    """fgcn_bn_act_pool: the mean over each group's rows of relu(...), and the sign image it leaves for the backward"""
    from fusion_gcn_amd import ops
    groups, per, C = 4, 84, 64
    rows = groups * per
    rd = bf if in16 else f32
    a0, b0 = rd(rnd(rows, C, seed=4) * 1.7 + 0.3), rd(rnd(rows, C, seed=5))
    va0, vb0 = vec4(C, 30), vec4(C, 40)
    fails, dt = [], (torch.bfloat16 if in16 else None)
    with ops.math_mode("bf16" if in16 else "f32"):
        for enter, pname in entries(res):
            r, c = divmod(positions(rows, C)[pname], C)
            a, b, va, vb = a0.clone(), b0.clone(), va0.clone(), vb0.clone()
            if enter in ("a", "b"):
                (a if enter == "a" else b)[r, c] = NF.POISONS[value]
            else:
                (va if enter.endswith("_a") else vb)[2 if enter.startswith("scale") else 3, c] = NF.POISONS[value]
            y = bn_act_ref(a, va, b, vb, res)
            want = torch.relu(y).view(groups, per, C).mean(1)
            where = f"[bn_act_pool {'typed' if in16 else 'f32'} res={res} {value} in {enter} at {pname} ({r}, {c})]"
            pooled, mask = ops.bn_act_pool(put(a, dt), put(va), put(b, dt) if res else None, put(vb) if res == 2 else None, groups)
            clean = torch.ones(groups, C, dtype=torch.bool)
            if enter in ("a", "b"):
                clean[r // per, c] = False                 # everything but the poisoned (group, channel) stays finite
            else:
                clean[:, c] = False                        # a channel's scale or shift: that channel of every group
            NF.check(fails, pooled, want, "class", BWD_TOL, where + " pooled", clean=clean.numpy())
            check_sign_image(fails, mask, y, where + " sign image")
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
def test_add_act_keeps_the_class_forward_and_backward(value):
    """fops.add_act (MS-G3D's joins): relu(a + b) and both gated gradients through autograd"""
    from fusion_gcn_amd import fops
    rows, C = 333, 64
    a0, b0, d0 = f32(rnd(rows, C, seed=6)), f32(rnd(rows, C, seed=7)), f32(rnd(rows, C, seed=8))
    fails = []
    for enter, pname in [("a", "first"), ("b", "last"), ("a", "pair")]:
        r, c = divmod(positions(rows, C)[pname], C)
        a, b = a0.clone(), b0.clone()
        (a if enter == "a" else b)[r, c] = NF.POISONS[value]
        ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        want = torch.relu(ar + br)
        ga, gb = torch.autograd.grad((want * d0).sum(), [ar, br])
        ag, bg = put(a).requires_grad_(True), put(b).requires_grad_(True)
        out = fops.add_act(ag, bg, relu=True)
        out.backward(put(d0))
        where = f"[add_act {value} in {enter} at {pname}]"
        NF.check(fails, out.detach(), want.detach(), "class", FWD_TOL, where + " out")
        NF.check(fails, ag.grad, ga, "class", BWD_TOL, where + " da")
        NF.check(fails, bg.grad, gb, "class", BWD_TOL, where + " db")
    raise_all(fails)


def temporal_ref(g, w, kt):
    B, T, V, C = g.shape
    pad = (kt - 1) // 2
    u = torch.zeros(B, T, V, w.shape[2], dtype=torch.float64)
    for j in range(kt):
        lo, hi = max(0, pad - j), min(T, T + pad - j)
        u[:, lo:hi] += g[:, lo + j - pad:hi + j - pad] @ w[j]
    return u


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("res", ["identity", "conv"])
def test_temporal_conv_epilogue_keeps_the_class(res, value):
    """fgcn_tconv_halo_bn_relu (math mode bf16x3): a poison in the shortcut or in the BatchNorm vector is the epilogue's own input -- rule 1;
    a poison in the convolved tensor goes through the contraction first -- rule 3, and for a NaN nothing outside its nine frames moves"""
    from fusion_gcn_amd import ops
    B, T, V, C, kt = 3, 37, 25, 64, 9
    pad = (kt - 1) // 2
    g0, w = f32(rnd(B, T, V, C, seed=90)), f32(rnd(kt, C, C, seed=91, scale=(kt * C) ** -0.5))
    bias, vec0 = f32(rnd(C, seed=92)), vec4(C, 93)
    r0, rvec = f32(rnd(B, T, V, C, seed=97)), (vec4(C, 98) if res == "conv" else None)
    u0, fails = temporal_ref(g0, w, kt), []
    with ops.math_mode("bf16x3"):
        w4 = ops.pack_split3(put(w))
        for enter, pname in [("res", "first"), ("res", "last"), ("res", "pair"), ("scale", "pair"), ("shift", "first"), ("g", "first"), ("g", "last")]:
            idx = np.unravel_index(positions(B * T * V, C)[pname], (B, T, V, C))
            g, r, vec = g0.clone(), r0.clone(), vec0.clone()
            if enter == "g":
                g[idx] = NF.POISONS[value]
            elif enter == "res":
                r[idx] = NF.POISONS[value]
            else:
                vec[2 if enter == "scale" else 3, idx[3]] = NF.POISONS[value]
            u = temporal_ref(g, w, kt) if enter == "g" else u0
            z = (u + bias) * vec[2] + vec[3] + (r if res == "identity" else r * rvec[2] + rvec[3])
            want = torch.relu(z)
            out = torch.empty(B, T, V, C, device=DEV)
            ops.tconv_halo_bn_relu(put(g), w4, out, taps=kt, tb=1, tc=-pad, vec=put(vec), bias=put(bias), res=put(r),
                                   res_vec=None if rvec is None else put(rvec))
            where = f"[tconv_halo_bn_relu {res} {value} in {enter} at {pname} {tuple(int(i) for i in idx)}]"
            if enter == "g":
                clean = torch.isfinite(want).numpy() if value == "nan" else None
                NF.check(fails, out, want, "contain", FWD_TOL, where, clean=clean)
            else:
                NF.check(fails, out, want, "class", FWD_TOL, where)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("down", [False, True], ids=["identity", "down"])
def test_spatial_tile_epilogue_keeps_the_class(down, value):
    """fgcn_spatial_fwd_tile_bn_relu (math mode bf16x3): as for the temporal kernel.  With the identity shortcut x is both the contracted
    tensor and the residual, so its poison is under rule 3"""
    from fusion_gcn_amd import ops
    V, T, cin, cout, B = (27, 9, 64, 128, 1) if down else (25, 13, 64, 64, 2)
    x0, a = f32(rnd(B, T, V, cin, seed=300)), f32(rnd(B, 3, V, V, seed=301, scale=0.3))
    wd, bias = f32(rnd(3, cin, cout, seed=302, scale=(3 * cin) ** -0.5)), f32(rnd(cout, seed=303))
    vec0 = vec4(cout, 304)
    d0, dvec = (f32(rnd(B, T, V, cout, seed=308)), vec4(cout, 309)) if down else (None, None)
    fails = []
    legs = [("x", "first"), ("x", "last"), ("scale", "pair"), ("shift", "last")] + ([("res", "first"), ("res", "last"), ("res", "pair")] if down else [])
    with ops.math_mode("bf16x3"):
        w3 = ops.pack_split3(put(wd.reshape(1, 3 * cin, cout)))
        for enter, pname in legs:
            x, d, vec = x0.clone(), (d0.clone() if down else None), vec0.clone()
            if enter == "x":
                idx = np.unravel_index(positions(B * T * V, cin)[pname], (B, T, V, cin))
                x[idx] = NF.POISONS[value]
            elif enter == "res":
                idx = np.unravel_index(positions(B * T * V, cout)[pname], (B, T, V, cout))
                d[idx] = NF.POISONS[value]
            else:
                idx = (positions(B * T * V, cout)[pname] % cout,)
                vec[2 if enter == "scale" else 3, idx[0]] = NF.POISONS[value]
            y = torch.einsum("btwkc,kco->btwo", torch.einsum("btvc,bkvw->btwkc", x, a), wd) + bias
            z = y * vec[2] + vec[3] + (d * dvec[2] + dvec[3] if down else x)
            want = torch.relu(z)
            got = ops.spatial_fwd_tile_bn_relu(put(x), put(a), w3, put(bias), put(vec), Cin=cin, Cout=cout, res=put(d) if down else put(x),
                                               res_vec=put(dvec) if down else None)
            where = f"[spatial_fwd_tile_bn_relu {'down' if down else 'identity'} {value} in {enter} at {pname} {tuple(int(i) for i in idx)}]"
            if enter == "x":
                NF.check(fails, got, want, "contain", FWD_TOL, where, clean=torch.isfinite(want).numpy() if value == "nan" else None)
            else:
                NF.check(fails, got, want, "class", FWD_TOL, where)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("res", [0, 1, 2])
def test_graph_spmm_relu_keeps_the_class_over_its_stored_entries(res, value):
    """fgcn_graph_spmm (the sparse=True route) with its residual and ReLU epilogue.  Rule 5: the route skips the structural zeros of the constant
    adjacency by contract, so the reference is torch's sparse product over the same stored entries -- a NaN in node u reaches exactly the nodes
    with a stored entry in column u.  Rule 1 against that reference, rule 2 on the sign image."""
    from fusion_gcn_amd import ops
    B, V, C = 3, 41, 64
    adj = torch.zeros(V, V, dtype=torch.float64)
    for v in range(V):                                  # a ring with self loops and a few chords: 3 to 11 entries per row, row 7 empty
        for u in (v, (v + 1) % V, (v - 1) % V):
            adj[v, u] = 0.2 + 0.01 * ((3 * v + u) % 7)
    adj[5, ::4] = 0.1
    adj[7] = 0.0
    adj = f32(adj)
    x0, b0, vb = f32(rnd(B, V, C, seed=50)), f32(rnd(B, V, C, seed=51)), vec4(C, 52)
    csr = ops.csr_from_dense(adj.float(), device=DEV)
    sp = adj.to_sparse()
    fails = []
    for enter, pname in [("x", "first"), ("x", "last"), ("x", "pair")] + ([("b", "first"), ("b", "pair")] if res else []):
        idx = np.unravel_index(positions(B * V, C)[pname], (B, V, C))
        x, b = x0.clone(), b0.clone()
        (x if enter == "x" else b)[idx] = NF.POISONS[value]
        y = torch.stack([torch.sparse.mm(sp, x[i]) for i in range(B)])
        if res:
            y = y + (b if res == 1 else b * vb[2] + vb[3])
        want = torch.relu(y)
        out, mask = ops.graph_spmm(put(x), csr, relu=True, b=put(b) if res else None, vec_b=put(vb) if res == 2 else None, sign_mask=True)
        where = f"[graph_spmm res={res} {value} in {enter} at {pname} {tuple(int(i) for i in idx)}]"
        rep = NF.check(fails, out, want, "class", FWD_TOL, where)
        check_sign_image(fails, mask, y, where + " sign image")
        if enter == "x":                                # the dense product would poison every node of the sample: the route's reference does not
            reached = int((~torch.isfinite(y[idx[0], :, idx[2]])).sum())
            assert 0 < reached <= 11 and rep is not None, (where, reached)
    raise_all(fails)


# =============================================================================================================================================
# contraction leg
# =============================================================================================================================================
def two_poisons(shape):
    """one element of the first row tile and one of the last, partial one: the first and the last element of the tensor"""
    return [("first tile", tuple(0 for _ in shape)), ("last tile", tuple(s - 1 for s in shape))]


def contain(fails, got, want, tol, where, value):
    """rule 3; for a NaN poison also: every row outside the poisoned element's receptive field (= where the reference stayed finite) is finite"""
    return NF.check(fails, got, want, "contain", tol, where, clean=torch.isfinite(want).numpy() if value == "nan" else None)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("mode", R.ALL_MODES)
def test_rows_gemm_never_swallows(mode, value):
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = 2, 20, 25, 64, 64, 9, 1
    rd = bf if mode == "bf16" else f32
    x0, w, b = rd(rnd(B, T, V, K, seed=1)), rd(rnd(kt, K, N, seed=2, scale=K ** -0.5)), f32(rnd(N, seed=3))
    tol = 2e-5 if mode == "bf16" else FWD_TOL           # tests/test_bf16_gpu.py's TOL: f32 sums of exactly representable products
    fails = []
    with ops.math_mode(mode):
        for tile, idx in two_poisons(x0.shape):
            x = NF.put_poison(x0, idx, NF.POISONS[value])
            want = ref_rows_conv(x, w, ops.conv_tmap(kt, s), T, b)
            out = torch.empty(B, T, V, N, device=DEV)
            ops.rows_gemm(put(x), put(w), out, K=K, N=N, tmap=ops.conv_tmap(kt, s), bias=put(b))
            contain(fails, out, want, tol, f"[rows_gemm {mode} {value} in the {tile}]", value)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("mode", ["bf16x3", "f16x2", "bf16"])
def test_pw_gemm_never_swallows(mode, value):
    from fusion_gcn_amd import ops
    rows, K, N = 517, 192, 128
    rd = bf if mode == "bf16" else f32
    x0, w, b = rd(rnd(rows, 1, 1, K, seed=200)), rd(rnd(1, K, N, seed=201, scale=K ** -0.5)), f32(rnd(N, seed=202))
    tol = 2e-5 if mode == "bf16" else FWD_TOL           # bf16: the reference is rounded to bfloat16 as in rows_gemm (tests/test_bf16_gpu.py's TOL)
    fails = []
    with ops.math_mode(mode):
        assert ops.pw_gemm_available()
        w3 = ops.pack_conv(put(w))
        for tile, idx in two_poisons(x0.shape):
            x = NF.put_poison(x0, idx, NF.POISONS[value])
            want = x.reshape(rows, K) @ w[0] + b
            out = torch.empty(rows, 1, 1, N, device=DEV)
            ops.pw_gemm(put(x), w3, out, bias=put(b))
            contain(fails, out.view(rows, N), want, tol, f"[pw_gemm {mode} {value} in the {tile}]", value)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("mode", R.ALL_MODES)
def test_halo_temporal_conv_never_swallows(mode, value):
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.block import temporal_dgrad, temporal_fwd
    B, T, V, C, O, kt = 3, 20, 25, 64, 64, 9
    rd = bf if mode == "bf16" else f32
    wt, bias = rd(rnd(kt, C, O, seed=80, scale=(kt * C) ** -0.5)), f32(rnd(O, seed=81))
    x0, du0 = rd(rnd(B, T, V, C, seed=82)), rd(rnd(B, T, V, O, seed=83))
    tol = 2e-5 if mode == "bf16" else FWD_TOL
    fails = []
    with ops.math_mode(mode):
        wg, wg_t = put(wt), put(wt.permute(0, 2, 1))
        W = {"t": wg, "t_t": wg_t, "t4": ops.pack_conv(wg), "t_t4": ops.pack_conv(wg_t)}
        for tile, idx in two_poisons(x0.shape):
            x = NF.put_poison(x0, idx, NF.POISONS[value])
            u = torch.empty(B, T, V, O, device=DEV)
            temporal_fwd(put(x), u, W, put(bias), kt, 1, stats=False)
            contain(fails, u, temporal_ref(x, wt, kt) + bias, tol, f"[tconv_halo {mode} {value} in the {tile}]", value)
            du = NF.put_poison(du0, idx, NF.POISONS[value])
            dg = torch.empty(B, T, V, C, device=DEV)
            temporal_dgrad(put(du), dg, W, kt, 1)
            contain(fails, dg, temporal_ref(du, wt.flip(0).permute(0, 2, 1), kt), tol, f"[tconv_halo data gradient {mode} {value} in the {tile}]", value)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("order", [None, (1,), (2, 1)], ids=["joint_mix", "vec1", "vec2"])
def test_joint_mix_never_swallows(order, value, monkeypatch):
    """fgcn_joint_mix and the channel-group kernel in both widths (they do not read the math mode); per-sample and shared matrices.  The mixing
    matrices are dense operands: a zero entry is a value, not structure, and 0 * NaN = NaN reaches every joint of the poisoned frame"""
    from fusion_gcn_amd import block, ops
    from fusion_gcn_amd.block import spec_agg
    B, T, V, cin = 3, 9, 25, 64
    x0, a = f32(rnd(B, T, V, cin, seed=20)), f32(rnd(B, 3, V, V, seed=21, scale=0.3))
    a[:, :, 3, :] = 0.0                                 # exact zeros in the operand: the reference multiplies them with the NaN too
    if order is not None:
        monkeypatch.setattr(ops.paths(), "mix_vw_order", order)
    fails = []
    for tile, idx in two_poisons(x0.shape):
        x = NF.put_poison(x0, idx, NF.POISONS[value])
        for shared in (False, True):
            mats = a[:1] if shared else a
            want = torch.einsum("btvc,bkvw->btwkc", x, mats.expand(B, 3, V, V)).reshape(B, T, V, 3 * cin)
            agg = put(torch.full((B, T, V, 3 * cin), 7.0))
            if order is None:
                ops.joint_mix(put(x), agg, put(mats), spec_agg(cin), in_channels=cin, out_channels=3 * cin)
            else:
                block.mix_agg(put(x), agg, put(mats), cin)
            contain(fails, agg, want, FWD_TOL, f"[joint_mix {order} {value} in the {tile}, {'shared' if shared else 'per-sample'} matrices]", value)
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
def test_row_softmax_never_swallows(value):
    from fusion_gcn_amd import ops
    B, K, V, ld, scale = 2, 3, 25, 28, 1.0 / 16
    st0 = torch.full((B, K, V, ld), float("nan"), dtype=torch.float64)
    adj = torch.full((K, V, ld), float("nan"), dtype=torch.float64)
    st0[..., :V], adj[..., :V] = f32(rnd(B, K, V, V, seed=V)), f32(rnd(K, V, V, seed=V + 1, scale=0.2))
    fails = []
    for tile, idx in [("first row", (0, 0, 0, 0)), ("last row", (B - 1, K - 1, V - 1, V - 1))]:
        st = NF.put_poison(st0, idx, NF.POISONS[value])
        c_want = torch.softmax(scale * st[..., :V], dim=-1)
        c, a = ops.row_softmax_fwd(put(st), put(adj), V, scale)
        where = f"[row_softmax_fwd {value} in the {tile}]"
        contain(fails, c[..., :V], c_want, 1e-5, where + " c", value)
        contain(fails, a[..., :V], c_want + adj[..., :V], 1e-5, where + " a", value)
        if value == "-inf":                             # the masking idiom: the reference is finite everywhere, so the kernel must be right
            assert bool(torch.isfinite(c_want).all())
        if not bool((c[..., V:] == 0).all() and (a[..., V:] == 0).all()):
            fails.append(f"{where}: the padding columns are not zero")
    raise_all(fails)


# ---- the f16x2 products and an inf: every scaled block, kernel by kernel ----------------------------------------------------------------------
# (at block level an inf's NaN region changes the ReLU gates, so finite gradients have no reference there; a kernel alone has one)
def amax_slot(t: torch.Tensor) -> torch.Tensor:
    """what the data-path kernels record for a tensor: its largest magnitude taken with fmaxf (a NaN is dropped, an inf is not), as float bits"""
    m = torch.where(torch.isnan(t), torch.zeros_like(t), t.abs()).max().float()
    return m.view(1).view(torch.int32).to(DEV)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("B,T,V,K,N,kt", [(2, 40, 25, 64, 64, 9), (2, 30, 25, 128, 192, 1)], ids=["all_taps", "pointwise"])
def test_f16x2_weight_gradient_never_corrupts(B, T, V, K, N, kt, value):
    """ops.tconv_wgrad / ops.rows_wgrad in math mode f16x2 (operands scaled by their tensor-wide maxima, test_weight_gradient_from_two_way_
    f16_splits' shapes and bound): a poison in either operand.  The reference is non-finite in one row (column) of dW and finite elsewhere;
    an inf maximum used as the scale would flush every other value to an f16 zero: finite, wrong everywhere else"""
    from fusion_gcn_amd import ops
    a0, g0 = f32(rnd(B, T, V, K, seed=300)), f32(rnd(B, T, V, N, seed=301))
    fails, pad = [], (kt - 1) // 2
    with ops.math_mode("f16x2"):
        for operand, (tile, idx) in [("a", two_poisons(a0.shape)[0]), ("g", two_poisons(g0.shape)[1])]:
            a = NF.put_poison(a0, idx, NF.POISONS[value]) if operand == "a" else a0
            g = NF.put_poison(g0, idx, NF.POISONS[value]) if operand == "g" else g0
            amax = (amax_slot(a), amax_slot(g))
            if kt > 1:
                got = ops.tconv_wgrad(put(a), put(g), taps=kt, stride=1, amax=amax)
            else:
                got = ops.rows_wgrad(put(a), put(g), K=K, N=N, amax=amax)
            want = torch.zeros(kt, K, N, dtype=torch.float64)
            for j in range(kt):
                lo, hi = max(0, pad - j), min(T, T + pad - j)
                want[j] = torch.einsum("btvk,btvn->kn", a[:, lo + j - pad:hi + j - pad], g[:, lo:hi])
            NF.check(fails, got.reshape(kt, K, N), want, "contain", RED_TOL, f"[f16x2 weight gradient {kt} taps, {value} in {operand} ({tile})]")
            assert bool(torch.isfinite(want).any()) and not bool(torch.isfinite(want).all())
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("operand", ["x", "a_hat"])
def test_f16x2_spatial_forward_never_corrupts(operand, value):
    """ops.spatial_fwd in math mode f16x2 (x scaled per frame pair and channel tile, the adjacency images per sample): a poison in x, and in one
    sample's adjacency.  Frames (samples) the poison cannot reach are finite and within the kernel's forward bound"""
    from fusion_gcn_amd import ops
    B, T, V, cin, cout = 2, 6, 25, 64, 64
    x0, a0 = f32(rnd(B, T, V, cin, seed=15)), f32(rnd(B, 3, V, V, seed=16, scale=0.3))
    wd = f32(rnd(3, cin, cout, seed=17, scale=(3 * cin) ** -0.5))
    fails = []
    with ops.math_mode("f16x2"):
        w = ops.pack_spatial(put(wd.reshape(3 * cin, cout)), cin)
        for tile, idx in two_poisons(x0.shape if operand == "x" else a0.shape):
            x = NF.put_poison(x0, idx, NF.POISONS[value]) if operand == "x" else x0
            a = NF.put_poison(a0, idx, NF.POISONS[value]) if operand == "a_hat" else a0
            want = torch.einsum("btwkc,kco->btwo", torch.einsum("btvc,bkvw->btwkc", x, a), wd)
            y, _ = ops.spatial_fwd(put(x), put(a), w, None, Cin=cin, Cout=cout, stats=False)
            assert bool(torch.isfinite(want).any()) and not bool(torch.isfinite(want).all())
            contain(fails, y, want, FWD_TOL, f"[f16x2 spatial_fwd {value} in {operand} ({tile})]", value)
    raise_all(fails)


# =============================================================================================================================================
# block leg
# =============================================================================================================================================
BLOCK_LEGS = [(m, p, c) for m in R.ALL_MODES for p in R.PHASES for c in NF.BLOCK_CASES]


def poisoned_input(run: R.BlockRun, poison) -> torch.Tensor:
    b, c, t, v, name = poison
    x = run.x_host.clone()                              # (B, T, V, C padded)
    x[b, t, v, c] = NF.POISONS[name]
    return x


def nchw_mask_of_other_samples(t: torch.Tensor) -> np.ndarray:
    m = torch.ones(t.shape, dtype=torch.bool)
    m[NF.POISONED_SAMPLE] = False
    return m.numpy()


def zero_bias_gradients(case, phase) -> tuple:
    """the conv biases in front of a batch-statistics BatchNorm (train phase): analytically zero, and handed out by the block as exact zeros
    (block._BiasGrads, 0 or NaN by its ``carry``).  The sweep holds them to rule 3 like every other gradient;
    test_train_phase_bias_gradients_carry_the_poison names them"""
    return R.oracle_case(case, phase)["zero"] if phase == "train" else ()


def check_block(fails, a, e, phase, ora, value, tag, ora_nan=None):
    """``ora_nan``: the oracle of the SAME poison position with a NaN in it, for an inf poison in the split-product modes.  There the inf leaves
    the first split as inf - inf = NaN (rule 3 says so), and from then on the block computes what the reference computes from a NaN: ReLUs
    that the reference closes at -inf (or opens at +inf) are open at the NaN (rule 2), so a finite gradient element is right if it is the NaN
    reference's.  dx and a parameter gradient pass if they meet rule 3 against either reference; out, adj_c and the buffers need no second one.

    f16x2 with an inf: the forward turns the inf's whole scaling blocks NaN (rule 4's exemption), a superset of the reference's non-finite
    region, and every ReLU in it is open (rule 2).  The backward is then the gradient under another gate pattern than either reference's, so
    its finite elements have no reference value: dx and the parameter gradients are held to "non-finite wherever the reference is" there."""
    mode, bf16 = e.plan.mode, e.plan.mode == "bf16"
    flips = NF.flips_outside_the_poisoned_sample(a["signs"], ora, R.B)
    tol_out, tol_c, tol_rs, tol_grad = block_tolerances(bf16, flips)          # the bounds of the un-injected run of the same entry
    f16x2_inf = mode == "f16x2" and value != "nan"
    rule4 = phase == "eval" and not f16x2_inf                                 # f16x2 with an inf: rule 3 alone
    if f16x2_inf:
        tol_grad = None
    if a["plans"] != [e.plan]:
        fails.append(f"{tag}: the block planned {a['plans']}, the matrix predicted {e.plan}")
    def either(got, name, get, tol, where, **kw):
        rep = NF.compare(got, get(ora), "contain", tol, where, **kw)
        if not rep.ok and ora_nan is not None and name != "out":
            alt = NF.compare(got, get(ora_nan), "contain", tol, where + " (against the NaN reference)", **kw)
            rep = alt if alt.ok else rep
        if not rep.ok:
            fails.append(rep.message)

    for name, tol in (("out", tol_out), ("dx", tol_grad)) + ((("adj_c", tol_c),) if ora["adj_c"] is not None else ()):
        clean = nchw_mask_of_other_samples(ora[name]) if rule4 else None
        either(a[name].cpu(), name, lambda o: o[name], tol, f"{tag} {name}", clean=clean, cosine=bf16 and name == "dx")
    for k, g in a["grads"].items():
        if k in ora["unused"]:
            continue                                    # no gradient in the oracle (static adjacency): nothing to classify
        shape = ora["want"][k].shape
        either(g.cpu().reshape(shape), k, lambda o: torch.from_numpy(o["want"][k]), tol_grad, f"{tag} d {k}", cosine=bf16)
    for k, v in a["buffers"].items():
        if phase == "eval" or k.endswith("adj_a"):
            if not torch.equal(v, a["buffers0"][k]):
                fails.append(f"{tag}: buffer {k} changed")
        elif k.endswith("num_batches_tracked"):
            if int(v) != int(ora["stats"][k]):
                fails.append(f"{tag}: {k} = {int(v)}")
        else:       # the reference's class; an inf that went through a split is a NaN (rule 3's own sentence), so there: non-finite where it is
            NF.check(fails, v.cpu(), ora["stats"][k], "class" if (mode == "f32" or value == "nan") else "contain", tol_rs, f"{tag} buffer {k}")


@pytest.mark.parametrize("mode,phase,case_name", BLOCK_LEGS, ids=[f"{m}-{p}-{c}" for m, p, c in BLOCK_LEGS])
def test_block_routes_with_a_poisoned_sample(mode, phase, case_name):
    """The covering subset of the route matrix (nonfinite_ref.covering_subset: every value of every ROUTE_TUPLE field the matrix reaches in
    these cases) with NaN, +inf and -inf in sample 1 of 3: rules 3 and 4 on out, dx, adj_c and every parameter gradient, the BatchNorm
    buffers' class in train phase, the plan really used"""
    from fusion_gcn_amd import _lib
    case = next(c for c in R.CASES if c.name == case_name)
    picked = [e for e in NF.covering_subset(mode, phase) if e.case == case]
    assert picked
    run = R.BlockRun(case, DEV)
    x_clean, fails = run.x_host, []
    try:
        for e in picked:
            for value in VALUES:
                poison = NF.block_poison(case, value)
                ora = NF.oracle_case(case, phase, poison)
                tag = f"[{mode} {phase} {case.name} | {e.option_name} | {value}]"
                run.x_host = poisoned_input(run, poison)
                try:
                    a = run.run(e, phase)
                except _lib.FgcnError as exc:
                    fails.append(f"{tag}: {exc}")
                    continue
                a["buffers0"] = run.buffers0
                n0 = len(fails)
                ora_nan = NF.oracle_case(case, phase, NF.block_poison(case, "nan")) if (mode != "f32" and value != "nan") else None
                check_block(fails, a, e, phase, ora, value, tag, ora_nan=ora_nan)
                print(f"{tag} {'ok' if len(fails) == n0 else 'FAILED'}", flush=True)
    finally:
        run.x_host = x_clean
    raise_all(fails)


@pytest.mark.parametrize("mode", R.ALL_MODES)
def test_train_phase_bias_gradients_carry_the_poison(mode):
    """Rule 3 on the gradients of the conv biases in front of a batch-statistics BatchNorm.  The reference's are NaN: autograd sums a NaN
    gradient tensor.  The block hands these out as exact zeros in train phase (block._BiasGrads: the batch mean cancels such a bias,
    SURVEY.md Appendix A.3); they must become NaN where the BatchNorm backward's channel sums are not numbers."""
    fails = []
    for case in (c for c in R.CASES if c.name in NF.BLOCK_CASES):
        e = next(x for x in NF.covering_subset(mode, "train") if x.case == case)
        poison = NF.block_poison(case, "nan")
        ora, run = NF.oracle_case(case, "train", poison), R.BlockRun(case, DEV)
        run.x_host = poisoned_input(run, poison)
        a = run.run(e, "train")
        for k in zero_bias_gradients(case, "train"):
            want = torch.from_numpy(ora["want"][k])
            NF.check(fails, a["grads"][k].cpu().reshape(want.shape), want, "contain", None, f"[{mode} train {case.name} | {e.option_name} | nan] d {k}")
    raise_all(fails)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("mode", R.ALL_MODES)
@pytest.mark.parametrize("case_name", NF.BLOCK_CASES)
def test_block_inference_route_with_a_poisoned_sample(case_name, mode, value):
    """block_forward(inference=True): module.eval() under no_grad, where BatchNorm, shortcut and ReLU are the epilogues of the two north-star
    kernels in the modes that have those forms.  Rules 3 and 4 on the output against the eval-phase oracle."""
    from fusion_gcn_amd import block, ops
    case = next(c for c in R.CASES if c.name == case_name)
    poison = NF.block_poison(case, value)
    ora = NF.oracle_case(case, "eval", poison)
    run = R.BlockRun(case, DEV)
    blk = run.blk.eval()
    plans, real = [], block.plan_block

    def spy(*a, **kw):
        plans.append(real(*a, **kw))
        return plans[-1]
    block.plan_block = spy
    try:
        with ops.context(mode), guarded.Guard() as g, torch.no_grad():
            R.poison(DEV)
            out = blk(guarded.put(poisoned_input(run, poison), device=DEV))
            torch.cuda.synchronize()
            g.check()
    finally:
        block.plan_block = real
    assert len(plans) == 1 and not plans[0].train and plans[0].mode == mode
    print(f"[{mode} {case.name}] inference plan: temporal_bn_relu={plans[0].temporal_bn_relu} spatial_fwd={plans[0].spatial_fwd}")
    if case.name == "identity64":       # where both fused epilogues have a form (stride 1, 64 -> 64): taken exactly in the modes that build them
        with ops.context(mode):
            built = bool(ops.inference_kernels_available() and ops.paths().fused_inference)
        assert plans[0].temporal_bn_relu == built and (plans[0].spatial_fwd == "tile_bn_relu") == built, (mode, plans[0])
    fails = []
    rule4 = not (mode == "f16x2" and value != "nan")
    got = out.float().permute(0, 3, 1, 2).cpu()
    NF.check(fails, got, ora["out"], "contain", block_tolerances(mode == "bf16", flips=1)[0], f"[inference {mode} {case.name} {value}] out",
             clean=nchw_mask_of_other_samples(ora["out"]) if rule4 else None)
    raise_all(fails)


# =============================================================================================================================================
# loss leg
# =============================================================================================================================================
CE_ROWS, CE_ROW = 5, 1
CE_PLACES = [(classes, place) for classes in (60, 67, 130) for place in ("target", "other", "past64") if classes > 64 or place != "past64"]


@functools.lru_cache(maxsize=None)
def ce_inputs(classes):
    g = torch.Generator().manual_seed(77 + classes)
    npad = classes // 4 * 4 + 4
    z = (torch.randn(CE_ROWS, npad, generator=g) * 3).double()
    y = torch.tensor([3, 11, 0, classes - 1, 20])
    w = (torch.rand(classes, generator=g) + 0.1).double()
    w[classes // 2] = 0.0
    t = torch.zeros(CE_ROWS, npad)
    t[:, :classes] = torch.softmax(torch.randn(CE_ROWS, classes, generator=g) * 2, dim=1)
    return z, y, w, t.double(), torch.randn(CE_ROWS, generator=g).double()


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("classes,place", CE_PLACES)
def test_cross_entropy_options_with_a_non_finite_logit(classes, place, value):
    """fusion_gcn_amd.loss.CrossEntropyLoss (fgcn_ce_fwd / fgcn_ce_bwd) against torch.nn.functional.cross_entropy in float64 with one logit
    of row 1 replaced, at the target class, at another class, and at a class a lane reaches in its second trip; class weights with a zero,
    label smoothing, probability targets, the three reductions.  The loss (per row under `none`) and the gradient have the reference's
    class at every position; finite values within 2e-6; a -inf at a non-target class -- the masking idiom -- stays finite and right"""
    z0, y, w, t, up = ce_inputs(classes)
    col = {"target": int(y[CE_ROW]), "other": 7, "past64": classes - 2}[place]
    assert col != classes // 2 and (place == "target") == (col == int(y[CE_ROW])) and (place != "past64" or col >= 64)
    z = z0.clone()
    z[CE_ROW, col] = NF.POISONS[value]
    fails = []
    for prob in (False, True):
        for use_w in (False, True):
            for eps in (0.0, 0.1):
                for reduction in ("none", "mean", "sum"):
                    weight = w if use_w else None
                    target = t[:, :classes] if prob else y
                    want, want_grad = ce_reference(z, target, classes, weight, -100, reduction, eps, up)
                    dev_target = guarded.to(t.float(), DEV)[:, :classes] if prob else guarded.to(y, DEV)
                    got, grad = ce_run(z, dev_target, classes, weight, -100, reduction, eps, up)
                    where = f"[cross_entropy C={classes} {value} at the {place} class, {'probabilities' if prob else 'labels'} w={use_w} eps={eps} {reduction}]"
                    NF.check(fails, got, want, "class", CE_TOL, where + " loss")
                    NF.check(fails, grad[:, :classes], want_grad, "class", CE_TOL, where + " gradient")
                    if float(grad[:, classes:].abs().max()) != 0.0:
                        fails.append(f"{where}: the pad columns of the gradient are not zero")
                    if value == "-inf" and place != "target" and eps == 0.0 and not prob:
                        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(want_grad).all()), where      # the idiom: nothing to hide behind
    raise_all(fails)


@guard
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("classes,place", CE_PLACES)
def test_plain_cross_entropy_with_a_non_finite_logit(classes, place, value):
    """the plain path (fgcn_cross_entropy_fwd / _bwd, mean reduction) under the same poisons"""
    from fusion_gcn_amd.loss import cross_entropy
    z0, y, _, _, _ = ce_inputs(classes)
    col = {"target": int(y[CE_ROW]), "other": 7, "past64": classes - 2}[place]
    z = z0[:, :classes].clone()
    z[CE_ROW, col] = NF.POISONS[value]
    zr = z.clone().requires_grad_(True)
    want = F.cross_entropy(zr, y)
    want_grad, = torch.autograd.grad(want, zr)
    zg = put(z).requires_grad_(True)
    got = cross_entropy(zg, guarded.to(y, DEV))
    got.backward()
    fails = []
    where = f"[plain cross_entropy C={classes} {value} at the {place} class]"
    NF.check(fails, got.detach(), want.detach(), "class", CE_TOL, where + " loss")
    NF.check(fails, zg.grad, want_grad, "class", CE_TOL, where + " gradient")
    raise_all(fails)


# =============================================================================================================================================
# model and session leg
# =============================================================================================================================================
BAD_CLIP, MODEL_SHAPE, MODEL_CLASSES = 2, (1, 16, 20, 3), 27


def small_model():
    from fusion_gcn_amd.datasets.utd_mhad import constants as utd
    from fusion_gcn_amd.models.mmargcn.agcn import Model
    from fusion_gcn_amd.util import Graph
    from oracle import filler
    model = Model(MODEL_SHAPE, MODEL_CLASSES, Graph(utd.skeleton_edges, center_joint=utd.center_joint), num_layers=2)
    filler.fill_state_dict(model.state_dict())
    return model


@functools.lru_cache(maxsize=None)
def model_inputs():
    """(x with one NaN coordinate in clip 2 of 4, labels, the float64 state dict): the two-block AGCN model of the ensemble and session tests"""
    from oracle import filler
    x = torch.from_numpy(filler.skeleton_input("x.nonfinite", (4,) + MODEL_SHAPE)).float()
    x[BAD_CLIP, 0, 8, 10, 1] = float("nan")
    labels = torch.from_numpy(filler.uniform("y.nonfinite", (4,), 0, MODEL_CLASSES).astype(np.int64))
    sd = {k: (v.detach().double() if v.is_floating_point() else v.detach().clone()) for k, v in small_model().state_dict().items()}
    return x, labels, sd


@guard
@pytest.mark.parametrize("grad", [False, True], ids=["inference", "eval_with_autograd"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
def test_model_eval_contains_a_nan_clip(mode, grad):
    """eval: the poisoned clip's scores have the oracle's class (all NaN), the other clips' scores are within the model tolerance (1e-5, the
    bound of the existing model tests) -- through the pooled epilogue of the last block, which must not mix the clips' groups"""
    from fusion_gcn_amd import block, ops
    from oracle import agcn_oracle as O
    x, _, sd = model_inputs()
    with torch.no_grad():
        want = O.model_forward(x.double(), sd, train=False, num_layers=2)
    model = guarded.to(small_model(), DEV).eval()
    plans, real = [], block.plan_block

    def spy(*a, **kw):
        plans.append(real(*a, **kw))
        return plans[-1]
    block.plan_block = spy
    try:
        with ops.math_mode(mode), torch.set_grad_enabled(grad):
            got = model(put(x)).detach().cpu()
    finally:
        block.plan_block = real
    assert len(plans) == 2 and plans[-1].pool_groups == x.shape[0], plans       # the last block pooled per clip in its epilogue
    clean = torch.ones_like(want, dtype=torch.bool)
    clean[BAD_CLIP] = False
    fails = []
    NF.check(fails, got, want, "class", 1e-5, f"[model eval {mode}] scores", clean=clean.numpy())
    raise_all(fails)


class _Losses:
    """the part of the metrics container Session.train_epoch uses: keeps every reported loss"""

    def __init__(self):
        self.losses = []

    def update_training(self, loss, pair, model, indices):
        self.losses.append(loss.detach().clone())

    def format_training(self):
        return ""


@guard
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_session_skips_a_step_whose_forward_is_not_finite(mode):
    """The sibling of test_overflowing_batch_through_the_session for a forward pass that is itself non-finite: one NaN coordinate makes the
    batch statistics, the loss and every gradient NaN (as in the reference); with skip_nonfinite=True the reported loss is NaN, and the
    parameters, the optimizer state and the applied-step count are those from before the step, bit for bit"""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.loss import cross_entropy
    from fusion_gcn_amd.optim import create_optimizer
    from fusion_gcn_amd.session.procedures import DefaultBatchProcessor, DefaultStep
    from fusion_gcn_amd.session.session import Session
    from oracle import filler
    x_bad, labels, _ = model_inputs()
    x_good = torch.from_numpy(filler.skeleton_input("x.nonfinite.good", (4,) + MODEL_SHAPE)).float()
    model = guarded.to(small_model(), DEV)
    opt = create_optimizer("ADAM", model, 1e-3, weight_decay=0.01, skip_nonfinite=True)
    proc, seen = DefaultBatchProcessor(DefaultStep()), _Losses()
    with ops.math_mode(mode):
        Session.train_epoch(proc, model, cross_entropy, [(x_good, labels, torch.arange(4))], opt, metrics=seen)
        torch.cuda.synchronize()
        assert opt.steps == 1 and opt.skipped_steps == 0 and bool(torch.isfinite(seen.losses[0]))
        params = [p.detach().clone() for p in model.parameters()]
        state = copy.deepcopy(opt.state_dict()["state"])
        Session.train_epoch(proc, model, cross_entropy, [(x_bad, labels, torch.arange(4))], opt, metrics=seen)
        torch.cuda.synchronize()
    assert len(seen.losses) == 2 and bool(torch.isnan(seen.losses[1])), seen.losses
    assert opt.steps == 1 and opt.skipped_steps == 1
    for p0, p in zip(params, model.parameters()):
        assert torch.equal(p0, p.detach())
    after = opt.state_dict()["state"]
    assert set(after) == set(state) and len(state) > 0
    for k, entry in state.items():
        for name, v in entry.items():
            same = torch.equal(v, after[k][name]) if isinstance(v, torch.Tensor) else v == after[k][name]
            assert same, (k, name)
