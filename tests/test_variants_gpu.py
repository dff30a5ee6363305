"""Every kernel variant that fgcn_set_tuning selects and no other test launches (the rows of tests/variants.py with a ``case``), on the MI355X:
the kernel runs under ``tuned(key, value)`` at the row's smallest engaging shapes, in every math mode the row names, and each result is
compared twice --

  (a) with the float64 formula of the kernel's own parity test, at that test's tolerance for the mode (tests/test_kernels_gpu.py: 3e-6 for
      forward-type results, 2e-5 for reductions; tests/test_bf16_gpu.py for math mode bf16: the formula on operands rounded to bfloat16 where
      the kernel rounds them, 2e-5 / 1e-4 / 2e-4 / 2e-3 as the test of that kernel has it);
  (b) with the default variant on the same inputs: bit for bit where the row is order-only, within the same tolerance otherwise; partial sums
      (BatchNorm statistics, gram and weight-gradient slabs) in total, and bit for bit too where the row says the partials are the same sums.

The accumulating forms and the epilogues with statistics are included wherever the kernel's own test includes them.  Outputs are guarded
allocations pre-filled with a sentinel (tests/guarded.py): a tile that no workgroup computes stays the sentinel, a store past an extent lands in
a margin and is reported by name at teardown.  References are computed once per (case, shape) and shared by every row and mode that uses them."""
import functools
from collections import namedtuple

import pytest
import torch

import guarded
import test_bf16_gpu as TB
import test_kernels_gpu as TK
import variants as VT
from conftest import rel_l2
from guarded import guarded_allocations  # noqa: F401  (the fixture)
from variants import tuned

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]

rnd, to_gpu, dev = TK.rnd, TK.to_gpu, TK.dev
Res = namedtuple("Res", "name kind got want tol raw")       # kind "out": got = the device tensor; "sum": got = float64 totals, raw = the partials
SENTINEL = 3.0


def tols(mode, fwd_bf16=TB.TOL, red_bf16=1e-4):
    """(forward, reduction) tolerance of a kernel in ``mode``: the kernel tests' pair, or what the bf16 test of that kernel asserts"""
    return (fwd_bf16, red_bf16) if mode == "bf16" else (TK.FWD_TOL, TK.RED_TOL)


def rounding(bf16):
    """where a kernel of math mode bf16 rounds an operand, its formula does (tests/test_bf16_gpu.py); the other modes' formulas round nothing"""
    return TB.bf if bf16 else (lambda t: t)


def out(name, got, want, tol):
    return Res(name, "out", got, want, tol, None)


def total(name, partial, dim, want, tol, window=None):
    tot = partial.double().sum(dim).cpu()
    return Res(name, "sum", tot if window is None else tot[..., :window, :window], want, tol, partial)


def filled(*shape, value=SENTINEL, dtype=torch.float32):
    return guarded.put(torch.full(shape, value), dtype=dtype, device=dev()) if dtype != torch.float32 else to_gpu(torch.full(shape, value))


def conv_wgrad_ref(a, g, kt, s):
    """weight gradient of the (kt x 1) conv with padding (kt - 1) // 2 and stride s: (kt, K, N)"""
    B, T, V, K = a.shape
    Tg, pad = g.shape[1], (kt - 1) // 2
    ap = torch.zeros(B, T + 2 * pad, V, K, dtype=torch.float64)
    ap[:, pad:pad + T] = a
    return torch.stack([torch.einsum("btvk,btvn->kn", ap[:, j:j + (Tg - 1) * s + 1:s], g) for j in range(kt)])


# ---- row GEMM --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_rows_gemm(shape, bf16):
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    q, tmap, T_out = rounding(bf16), ops.conv_tmap(kt, s), (T - 1) // s + 1
    x, w, b = rnd(B, T, V, K, seed=1), rnd(kt, K, N, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    base = rnd(B, T_out, V, N, seed=6)
    plain = TK.ref_rows_conv(q(x), q(w), tmap, T_out)
    return dict(x=x, w=w, b=b, base=base, want=plain + b, want_acc=base + plain)


def run_rows_gemm(shape, mode):
    """test_rows_gemm_forward_and_stats + the accumulating form of test_rows_gemm_channel_windows_and_accumulate (bf16: test_rows_gemm_bf16)"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    R, (fwd, red) = ref_rows_gemm(shape, mode == "bf16"), tols(mode)
    tmap, T_out = ops.conv_tmap(kt, s), (T - 1) // s + 1
    y = filled(B, T_out, V, N)
    part = ops.rows_gemm(to_gpu(R["x"]), to_gpu(R["w"]), y, K=K, N=N, tmap=tmap, bias=to_gpu(R["b"]), stats=True)
    flat = R["want"].reshape(-1, N)
    acc = to_gpu(R["base"])
    ops.rows_gemm(to_gpu(R["x"]), to_gpu(R["w"]), acc, K=K, N=N, tmap=tmap, accumulate=True)
    res = [out("out", y, R["want"], fwd), out("accumulated", acc, R["want_acc"], fwd)]
    tot = part.double().sum(0).cpu()
    res.append(Res("sum", "sum", tot[0], flat.sum(0), red, part))
    if mode != "bf16":                              # (test_rows_gemm_bf16 checks the sums only)
        res.append(Res("sum of squares", "sum", tot[1], (flat ** 2).sum(0), red, part))
    return res


@functools.lru_cache(maxsize=None)
def ref_wgrad(shape, bf16):
    B, T, V, K, N, kt, s = shape
    q = rounding(bf16)
    a, g = rnd(B, T, V, K, seed=10), rnd(B, (T - 1) // s + 1, V, N, seed=11)
    return dict(a=a, g=g, want=conv_wgrad_ref(q(a), q(g), kt, s))


def wgrad_results(run, R, red):
    got = run(None)
    acc = got.clone()
    run(acc)
    return [out("gradient", got, R["want"], red), out("accumulated", acc, 2 * R["want"], red)]


def run_rows_wgrad(shape, mode):
    """test_rows_wgrad, the per-tap kernel (wide=False); bf16: test_weight_gradients_bf16"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    R = ref_wgrad(shape, mode == "bf16")
    a, g = to_gpu(R["a"]), to_gpu(R["g"])
    return wgrad_results(lambda acc: ops.rows_wgrad(a, g, K=K, N=N, tmap=ops.conv_tmap(kt, s), wide=False, out=acc, accumulate=acc is not None), R,
                         tols(mode)[1])


def run_tconv_wgrad(shape, mode):
    """test_tconv_wgrad_all_taps_in_one_pass (the slab count is asked for on every call: the partial buffer follows the key)"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    R = ref_wgrad(shape, mode == "bf16")
    a, g = to_gpu(R["a"]), to_gpu(R["g"])
    return wgrad_results(lambda acc: ops.tconv_wgrad(a, g, taps=kt, stride=s, all_taps=True, out=acc, accumulate=acc is not None), R, tols(mode)[1])


def run_pw_wgrad(shape, mode):
    """test_pointwise_wgrad_channel_chunks: the 1x1 form (wide=True), optionally strided"""
    from fusion_gcn_amd import ops
    B, T, V, K, N, kt, s = shape
    assert kt == 1
    R = ref_wgrad(shape, mode == "bf16")
    a, g = to_gpu(R["a"]), to_gpu(R["g"])
    return wgrad_results(lambda acc: ops.rows_wgrad(a, g, K=K, N=N, tmap=(1, s, 0, 0, 1), wide=True, out=acc, accumulate=acc is not None), R,
                         tols(mode)[1])


# ---- halo conv -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_tconv_halo(shape, bf16):
    from fusion_gcn_amd import ops
    B, T, V, K, N = shape
    q, kt = rounding(bf16), 9
    wt, bias, g = rnd(kt, K, N, seed=400, scale=(kt * K) ** -0.5), rnd(N, seed=402), rnd(B, T, V, K, seed=401)
    plain = TK.ref_rows_conv(q(g), q(wt), ops.conv_tmap(kt, 1), T)
    R = dict(wt=wt, bias=bias, g=g, want=plain + bias, want_acc=2 * plain + bias)
    if K == N and N <= 64:          # the data gradient with the BatchNorm-backward sums (test_halo_data_gradient_emits_the_batchnorm_backward_sums)
        du, a, xres = rnd(B, T, V, N, seed=120), rnd(B, T, V, N, seed=122), rnd(B, T, V, N, seed=123)
        gamma, beta = rnd(N, seed=124).abs() + 0.5, rnd(N, seed=125)
        mean, var = a.reshape(-1, N).mean(0), a.reshape(-1, N).var(0, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        g_pre = (a - mean) * rstd * gamma + beta + xres
        dg = TK.ref_rows_conv(du, wt, ops.conv_dgrad_tmap(kt, 1), T)
        dp = dg * (g_pre.float() > 0)
        R.update(du=du, a=a, xres=xres, vec=torch.stack([mean, rstd, gamma * rstd, beta - mean * gamma * rstd]), want_dg=dg,
                 want_bn=torch.stack([dp.reshape(-1, N).sum(0), (dp * (a - mean) * rstd).reshape(-1, N).sum(0)]))
    return R


def run_tconv_halo(shape, mode):
    """the nine-tap halo conv as test_halo_conv_wave_arrangements_agree runs it: forward with the BatchNorm moments, the accumulating second
    pass with moments, and (split kernels of the float32-class modes, K == N <= 64) the data gradient with the BatchNorm-backward sums"""
    from fusion_gcn_amd import ops
    B, T, V, K, N = shape
    R, (fwd, red) = ref_tconv_halo(shape, mode == "bf16"), tols(mode)
    w4, g, bias = ops.pack_conv(to_gpu(R["wt"])), to_gpu(R["g"]), to_gpu(R["bias"])
    u = filled(B, T, V, N)
    part = ops.tconv_halo(g, w4, u, Th=T, taps=9, tb=1, tc=-4, bias=bias, stats=True)
    acc = u.clone()
    part_acc = ops.tconv_halo(g, w4, acc, Th=T, taps=9, tb=1, tc=-4, accumulate=True, stats=True)
    flat, flat_acc = R["want"].reshape(-1, N), R["want_acc"].reshape(-1, N)
    res = [out("out", u, R["want"], fwd), out("accumulated", acc, R["want_acc"], fwd),
           Res("sum", "sum", part.double().sum(0).cpu()[0], flat.sum(0), red, part),
           Res("sum, accumulated", "sum", part_acc.double().sum(0).cpu()[0], flat_acc.sum(0), red, part_acc)]
    if mode != "bf16":
        res.append(Res("sum of squares", "sum", part.double().sum(0).cpu()[1], (flat ** 2).sum(0), red, part))
    if "want_dg" in R and mode in VT.X3 and ops.tconv_halo_bn_sums():
        a, vec = to_gpu(R["a"]), to_gpu(R["vec"])
        _, sign = ops.bn_act(a, vec, to_gpu(R["xres"]), None, relu=True, sign_mask=True)
        dg = filled(B, T, V, N)
        part_bn = ops.tconv_halo(to_gpu(R["du"]), w4, dg, Th=T, taps=9, tb=-1, tc=4, bn_bwd=(a, sign, vec))
        res += [out("data gradient", dg, R["want_dg"], fwd), Res("BatchNorm-backward sums", "sum", part_bn.double().sum(0).cpu(), R["want_bn"], red, part_bn)]
    return res


@functools.lru_cache(maxsize=None)
def ref_bf16_out_halo(shape):
    from fusion_gcn_amd import ops
    B, T, V, K, N = shape
    g = TB.bf(rnd(B, T, V, K, seed=5))
    wt, bias = rnd(9, K, N, seed=7, scale=(9 * K) ** -0.5), rnd(N, seed=8)
    return dict(g=g, wt=wt, bias=bias, want=TK.ref_rows_conv(g, TB.bf(wt), ops.conv_tmap(9, 1), T) + bias,
                want_dg=TK.ref_rows_conv(g, TB.bf(wt), ops.conv_dgrad_tmap(9, 1), T))


BF16_STORE = 2.0 ** -9        # a bfloat16 store rounds the float32 result to 8 significand bits, to nearest even: <= 2^-9 relative per element


def run_tconv_halo_bf16_out(shape, mode):
    """test_halo_conv_writes_bfloat16 (math mode bf16, half_mask 3): the bfloat16 output is the rounding of the float32 output of the same call
    and the moments are those of the float32 values, bit for bit -- asserted here as that test does -- and against float64: the float32 form at
    test_halo_conv_bf16_forward_and_data_gradient's tolerance, the bfloat16 form at that plus one bfloat16 rounding"""
    from fusion_gcn_amd import ops
    assert mode == "bf16"
    B, T, V, K, N = shape
    R = ref_bf16_out_halo(shape)
    g16 = guarded.put(R["g"].float(), dtype=torch.bfloat16, device=dev())
    w, bias = ops.pack_split3(to_gpu(R["wt"])), to_gpu(R["bias"])
    u32, u16 = filled(B, T, V, N), filled(B, T, V, N, dtype=torch.bfloat16)
    p32 = ops.tconv_halo(g16, w, u32, Th=T, taps=9, tb=1, tc=-4, bias=bias, stats=True)
    p16 = ops.tconv_halo(g16, w, u16, Th=T, taps=9, tb=1, tc=-4, bias=bias, stats=True)
    assert torch.equal(u16, u32.to(torch.bfloat16)) and torch.equal(p32, p16)
    res = [out("float32 out", u32, R["want"], TB.TOL), out("bfloat16 out", u16, R["want"], TB.TOL + BF16_STORE),
           Res("sum", "sum", p16.double().sum(0).cpu()[0], R["want"].reshape(-1, N).sum(0), 1e-4, p16)]
    d32, d16 = filled(B, T, V, N), filled(B, T, V, N, dtype=torch.bfloat16)      # the data-gradient tap order through the same store epilogue
    ops.tconv_halo(g16, w, d32, Th=T, taps=9, tb=-1, tc=4)
    ops.tconv_halo(g16, w, d16, Th=T, taps=9, tb=-1, tc=4)
    assert torch.equal(d16, d32.to(torch.bfloat16))
    return res + [out("float32 data gradient", d32, R["want_dg"], TB.TOL), out("bfloat16 data gradient", d16, R["want_dg"], TB.TOL + BF16_STORE)]


# ---- spatial stage ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_spatial(shape, bf16):
    V, T, cin, cout, B = shape
    q = rounding(bf16)
    x, a = rnd(B, T, V, cin, seed=300), rnd(B, 3, V, V, seed=301, scale=0.3)
    wd, bias = rnd(3, cin, cout, seed=302, scale=(3 * cin) ** -0.5), rnd(cout, seed=303)
    dy, base = rnd(B, T, V, cout, seed=312), rnd(B, T, V, cin, seed=313)
    agg = torch.einsum("btvc,bkvw->btwkc", q(x), q(a))
    agg1 = torch.einsum("btvc,kvw->btwkc", q(x), q(a[0]))
    wt = wd.permute(2, 0, 1).reshape(1, cout, 3 * cin)                          # [o][k cin + c] = Wd_k[c][o]
    dagg = q(torch.einsum("btwo,okc->btwkc", q(dy), q(wt).reshape(cout, 3, cin)))
    R = dict(x=x, a=a, wd=wd, bias=bias, dy=dy, base=base, wt=wt,
             want_y=torch.einsum("btwkc,kco->btwo", q(agg), q(wd)) + bias, want_y1=torch.einsum("btwkc,kco->btwo", q(agg1), q(wd)),
             want_w=torch.einsum("btwkc,btwo->kco", q(agg), q(dy)).reshape(3 * cin, cout),
             want_w1=torch.einsum("btwkc,btwo->kco", q(agg1), q(dy)).reshape(3 * cin, cout),
             want_dx=torch.einsum("btwkc,bkvw->btvc", dagg, q(a)), want_dx1=torch.einsum("btwkc,kvw->btvc", dagg, q(a[0])),
             want_g=torch.einsum("btvc,btwkc->bkvw", q(x), dagg))
    gate = torch.zeros(B, T, V, cin, dtype=torch.float64)
    R["gated"] = []
    for i in range(2):
        e, pre = rnd(B, T, V, cin, seed=320 + i), rnd(B, T, V, cin, seed=330 + i)
        gate = gate + e * (pre.float() > 0)
        R["gated"].append((e, pre))
    R["want_gated"] = R["want_dx"] + gate
    return R


def run_spatial_fwd(shape, mode):
    """fgcn_spatial_fwd in a split mode against test_spatial_forward_tile_form's einsums (it compares this kernel with them through the tile
    form): per-sample adjacency with bias and BatchNorm moments -- the moments against the output written, as that test has them --, shared
    adjacency without"""
    from fusion_gcn_amd import ops
    V, T, cin, cout, B = shape
    R, (fwd, red) = ref_spatial(shape, False), tols(mode)
    wd = ops.pack_spatial(to_gpu(R["wd"].reshape(3 * cin, cout)), cin)
    y, part = ops.spatial_fwd(to_gpu(R["x"]), to_gpu(R["a"]), wd, to_gpu(R["bias"]), Cin=cin, Cout=cout, stats=True)
    y1, _ = ops.spatial_fwd(to_gpu(R["x"]), to_gpu(R["a"][:1]), wd, None, Cin=cin, Cout=cout, stats=False)
    yd = y.double()
    tot = part.double().sum(0).cpu()
    return [out("y", y, R["want_y"], fwd), out("y, shared adjacency", y1, R["want_y1"], fwd),
            Res("sum", "sum", tot[0], yd.sum((0, 1, 2)).cpu(), red, part), Res("sum of squares", "sum", tot[1], (yd ** 2).sum((0, 1, 2)).cpu(), red, part)]


def run_spatial_wgrad(shape, mode):
    """test_spatial_wgrad_fused_agg_recompute: per-sample and shared adjacency"""
    from fusion_gcn_amd import ops
    R, red = ref_spatial(shape, False), tols(mode)[1]
    x, dy = to_gpu(R["x"]), to_gpu(R["dy"])
    return [out("gradient", ops.spatial_wgrad(x, dy, to_gpu(R["a"]))[0], R["want_w"], red),
            out("gradient, shared adjacency", ops.spatial_wgrad(x, dy, to_gpu(R["a"][:1]))[0], R["want_w1"], red)]


def gated_pairs(R, cin):
    from fusion_gcn_amd import ops
    ident = guarded.to(torch.stack([torch.zeros(cin), torch.ones(cin), torch.ones(cin), torch.zeros(cin)]).float(), dev())
    return [(to_gpu(e), ops.bn_act(to_gpu(pre), ident, relu=True, sign_mask=True)[1]) for e, pre in R["gated"]]


def run_spatial_bwd_tile(shape, mode):
    """test_spatial_backward_tile_form (bf16: test_spatial_tile_kernels_with_one_bf16_part, 2e-4): dx with and without accumulation, shared
    adjacency, the gated addends of the two identity shortcuts; the partial grams in total, their padding exactly zero"""
    from fusion_gcn_amd import ops
    V, T, cin, cout, B = shape
    assert ops.spatial_bwd_tile_available(V, cin, cout)
    R, (fwd, red) = ref_spatial(shape, mode == "bf16"), tols(mode, 2e-4, 2e-4)
    dy, x, a, w3 = to_gpu(R["dy"]), to_gpu(R["x"]), to_gpu(R["a"]), ops.pack_split3(to_gpu(R["wt"]))
    res = []
    for acc in (False, True):
        dx = to_gpu(R["base"])
        part = ops.spatial_bwd_tile(dy, x, a, w3, dx, accumulate=acc)
        assert V == 32 or (float(part[:, :, :, V:, :].abs().max()) == 0.0 and float(part[:, :, :, :, V:].abs().max()) == 0.0)
        res += [out(f"dx, accumulate={acc}", dx, R["want_dx"] + (R["base"] if acc else 0), fwd),
                total(f"grams, accumulate={acc}", part, 1, R["want_g"], red, window=V)]
    dx1 = filled(B, T, V, cin)
    ops.spatial_bwd_tile(dy, x, to_gpu(R["a"][:1]), w3, dx1, accumulate=False)
    res.append(out("dx, shared adjacency", dx1, R["want_dx1"], fwd))
    if mode != "bf16":
        dxg = filled(B, T, V, cin, value=float("nan"))
        part_g = ops.spatial_bwd_tile(dy, x, a, w3, dxg, accumulate=False, gated=gated_pairs(R, cin))
        res += [out("dx, gated addends", dxg, R["want_gated"], fwd), total("grams, gated addends", part_g, 1, R["want_g"], red, window=V)]
    return res


def run_spatial_fwd_tile_bf16_out(shape, mode):
    """test_spatial_tile_kernels_on_bfloat16_activations: y as bfloat16 is the rounding of the float32 y of the same call, the moments those
    of the float32 values -- asserted as that test does -- and against float64 at test_spatial_tile_kernels_with_one_bf16_part's 2e-4 (plus
    one bfloat16 rounding for the bfloat16 form)"""
    from fusion_gcn_amd import ops
    assert mode == "bf16"
    V, T, cin, cout, B = shape
    R = ref_spatial(shape, True)
    x32 = to_gpu(TB.bf(R["x"]))
    x16 = guarded.put(TB.bf(R["x"]).float(), dtype=torch.bfloat16, device=dev())
    a, bias = to_gpu(R["a"]), to_gpu(R["bias"])
    wd = ops.pack_split3(to_gpu(R["wd"].reshape(1, 3 * cin, cout)))
    y32, p32 = ops.spatial_fwd_tile(x32, a, wd, bias, Cin=cin, Cout=cout)
    res = [out("float32 y", y32, R["want_y"], 2e-4)]
    for name, xin in (("bfloat16 x", x16), ("float32 x", x32)):
        y16, p16 = ops.spatial_fwd_tile(xin, a, wd, bias, Cin=cin, Cout=cout, y_bf16=True)
        assert y16.dtype == torch.bfloat16 and torch.equal(y16, y32.to(torch.bfloat16)) and torch.equal(p32, p16)
        res += [out(f"bfloat16 y, {name}", y16, R["want_y"], 2e-4 + BF16_STORE),
                Res(f"sum, {name}", "sum", p16.double().sum(0).cpu()[0], y32.double().sum((0, 1, 2)).cpu(), TB.TOL, p16)]
    return res


# ---- joint kernels ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_joint_dagg(shape):
    V, T, C, B = shape
    x, a = rnd(B, T, V, C, seed=90), rnd(B, 3, V, V, seed=91, scale=0.3)
    dagg, base = rnd(B, T, V, 3 * C, seed=92), rnd(B, T, V, C, seed=93)
    d4 = dagg.reshape(B, T, V, 3, C)
    R = dict(x=x, a=a, dagg=dagg, base=base, want_dx=torch.einsum("btwkc,bkvw->btvc", d4, a), want_dx1=torch.einsum("btwkc,kvw->btvc", d4, a[0]),
             want_g=torch.einsum("btvc,btwkc->bkvw", x, d4), gated=[])
    gate = torch.zeros(B, T, V, C, dtype=torch.float64)
    for i in range(2):
        e, pre = rnd(B, T, V, C, seed=100 + i), rnd(B, T, V, C, seed=110 + i)
        gate = gate + e * (pre.float() > 0)
        R["gated"].append((e, pre))
    R["gate"] = gate
    return R


def run_joint_dagg(shape, mode):
    """test_joint_dagg_fused_dx_and_gram + test_joint_dagg_adds_the_gated_shortcut_gradients: dx with and without accumulation, with none
    and with both gated addends, shared adjacency; the partial grams in total, their padding exactly zero"""
    from fusion_gcn_amd import ops
    V, T, C, B = shape
    R, (fwd, red) = ref_joint_dagg(shape), tols(mode)
    x, dagg, a = to_gpu(R["x"]), to_gpu(R["dagg"]), to_gpu(R["a"])
    gated = gated_pairs(R, C)
    res = []
    for acc in (False, True):
        for pairs in ((), gated):
            dx = to_gpu(R["base"])
            part = ops.joint_dagg(x, dagg, a, dx, accumulate=acc, gated=pairs)
            assert V == 32 or float(part[:, :, :, V:, :].abs().max()) == 0.0
            tag = f"accumulate={acc}, {len(pairs)} gated"
            res += [out("dx, " + tag, dx, R["want_dx"] + (R["base"] if acc else 0) + (R["gate"] if pairs else 0), fwd),
                    total("grams, " + tag, part, 1, R["want_g"], red, window=V)]
    dx1 = filled(B, T, V, C)
    ops.joint_dagg(x, dagg, to_gpu(R["a"][:1]), dx1, accumulate=False)
    res.append(out("dx, shared adjacency", dx1, R["want_dx1"], fwd))
    return res


@functools.lru_cache(maxsize=None)
def ref_joint_gram(shape):
    V, T, ic = shape
    emb = rnd(3, T, V, 6 * ic, seed=26)
    e = emb.reshape(3, T, V, 3, 2, ic)
    return dict(emb=emb, want=torch.einsum("btvke,btwke->bkvw", e[..., 0, :], e[..., 1, :]))


def run_joint_gram(shape, mode):
    """test_joint_gram_and_adjacency_softmax's affinity gram theta_k^T phi_k: three items of one width that do not share their first operand"""
    from fusion_gcn_amd import ops
    V, T, ic = shape
    R = ref_joint_gram(shape)
    emb = to_gpu(R["emb"])
    part = ops.joint_gram(emb, emb, [(2 * k * ic, (2 * k + 1) * ic, ic) for k in range(3)])
    assert tuple(part.shape[2:]) == (3, 32, 32) and float(part[:, :, :, V:, :].abs().max()) == 0.0 and float(part[:, :, :, :, V:].abs().max()) == 0.0
    return [total("grams", part, 1, R["want"], tols(mode)[1], window=V)]


# ---- embedding backward ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_emb(shape, bf16):
    """test_embedding_backward_tile_form's reference (emb_backward_reference), with the roundings of test_embedding_backward_tile_form_bf16"""
    V, T, ic, cx, B = shape
    q = rounding(bf16)
    emb, ds = rnd(B, T, V, 6 * ic, seed=350), rnd(B, 3, V, V, seed=351, scale=0.3)
    x, base = rnd(B, T, V, cx, seed=352), rnd(B, T, V, cx, seed=353)
    w = rnd(6 * ic, cx, seed=354, scale=(6 * ic) ** -0.5)

    def demb_of(d_s):
        e = q(emb).reshape(B, T, V, 3, 2, ic)
        dtheta = torch.einsum("bkvw,btwke->btvke", q(d_s), e[..., 1, :])
        dphi = torch.einsum("bkvw,btvke->btwke", q(d_s), e[..., 0, :])
        return torch.stack([dtheta, dphi], dim=4).reshape(B, T, V, 6 * ic)
    demb, demb1 = demb_of(ds), demb_of(ds[:1].expand(B, 3, V, V))
    return dict(emb=emb, ds=ds, x=x, base=base, w=w, want_dx=q(demb) @ q(w), want_dx1=q(demb1) @ q(w),
                want_w=torch.einsum("btvj,btvc->jc", q(demb), q(x)), want_b=demb.sum((0, 1, 2)),
                want_w1=torch.einsum("btvj,btvc->jc", q(demb1), q(x)), want_b1=demb1.sum((0, 1, 2)))


def run_emb_dx_tile(shape, mode):
    from fusion_gcn_amd import ops
    V, T, ic, cx, B = shape
    assert ops.emb_tile_available(V, ic, cx) and cx > 64
    R, fwd = ref_emb(shape, mode == "bf16"), tols(mode, 2e-4)[0]
    emb, w3 = to_gpu(R["emb"]), ops.pack_split3(to_gpu(R["w"].reshape(1, 6 * ic, cx)))
    res = []
    for acc in (False, True):
        dx = to_gpu(R["base"]) if acc else filled(B, T, V, cx, value=float("nan"))          # without accumulation every element is written
        ops.emb_dx_tile(emb, to_gpu(R["ds"]), w3, dx, ic=ic, accumulate=acc)
        res.append(out(f"dx, accumulate={acc}", dx, R["want_dx"] + (R["base"] if acc else 0), fwd))
    dx1 = filled(B, T, V, cx)
    ops.emb_dx_tile(emb, to_gpu(R["ds"][:1]), w3, dx1, ic=ic, accumulate=False)
    res.append(out("dx, shared dS", dx1, R["want_dx1"], fwd))
    return res


def run_emb_wgrad_tile(shape, mode):
    from fusion_gcn_amd import ops
    V, T, ic, cx, B = shape
    assert ops.emb_tile_available(V, ic, cx)
    R = ref_emb(shape, mode == "bf16")
    red, red_b = (2e-4, TB.TOL) if mode == "bf16" else (TK.RED_TOL, TK.RED_TOL)
    emb, x = to_gpu(R["emb"]), to_gpu(R["x"])
    gw, gb = ops.emb_wgrad_tile(emb, x, to_gpu(R["ds"]), ic=ic)
    gw1, gb1 = ops.emb_wgrad_tile(emb, x, to_gpu(R["ds"][:1]), ic=ic)
    return [out("weight gradient", gw, R["want_w"], red), out("bias gradient", gb, R["want_b"], red_b),
            out("weight gradient, shared dS", gw1, R["want_w1"], red), out("bias gradient, shared dS", gb1, R["want_b1"], red_b)]


# ---- BatchNorm-backward reduction on bfloat16 operands ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_bn_reduce(shape):
    """the sums of test_batchnorm_epilogue_forward_backward (sum dp, sum dp * a_hat, and sum dp * b_hat of a residual BatchNorm) on bfloat16
    values, with the ReLU gate as a given bit image"""
    rows, C, res = shape
    a, b, d = TB.bf(rnd(rows, C, seed=1)), TB.bf(rnd(rows, C, seed=2)), TB.bf(rnd(rows, C, seed=3))
    vec = lambda seed: torch.stack([rnd(C, seed=seed), rnd(C, seed=seed + 1).abs() + 0.5, rnd(C, seed=seed + 2), rnd(C, seed=seed + 3)]).float()  # noqa: E731
    va, vb = vec(10), vec(20)
    gen = torch.Generator().manual_seed(rows + C)
    mask = torch.randint(0, 256, (rows * C // 8,), generator=gen, dtype=torch.uint8)
    bits = ((mask.view(-1, 1).int() >> torch.arange(8).view(1, 8)) & 1).reshape(rows, C).double()        # bit e % 8 of byte e / 8
    dp = d * bits
    want = torch.zeros(3, C, dtype=torch.float64)
    want[0], want[1] = dp.sum(0), (dp * (a - va[0].double()) * va[1].double()).sum(0)
    if res == 2:
        want[2] = (dp * (b - vb[0].double()) * vb[1].double()).sum(0)
    return dict(a=a, b=b, d=d, va=va, vb=vb, mask=mask, want=want)


def run_bn_reduce_bf16(shape, mode):
    from fusion_gcn_amd import ops
    assert mode == "bf16"
    rows, C, res = shape
    R = ref_bn_reduce(shape)
    h16 = lambda t: guarded.put(t.float(), dtype=torch.bfloat16, device=dev())       # noqa: E731
    mask = guarded.put(R["mask"], device=dev())
    b, vb = (h16(R["b"]) if res else None), (to_gpu(R["vb"]) if res == 2 else None)
    _, _, sums = ops.bn_act_bwd(h16(R["d"]), None, h16(R["a"]), to_gpu(R["va"]), b, vb, res_mode=res, sign_mask=mask, need_db=res == 2)
    n = 3 if res == 2 else 2
    return [out("sums", sums[:n], R["want"][:n], TK.RED_TOL)]


# ---- the test --------------------------------------------------------------------------------------------------------------------------------
RUNNERS = {name[4:]: fn for name, fn in list(globals().items()) if name.startswith("run_")}
CASES = [pytest.param(r, mode, id=f"key{r.key}-{r.value}-{mode}") for r in VT.gpu_rows() for mode in r.modes]


def values_of(r, shape):
    """the values a row is run at: its value, or for a workgroup target one segment per sample and two (B is the shape's last entry)"""
    return [1, 2 * shape[-1]] if r.value == "target" else [r.value]


def check_against_float64(results, where):
    for res in results:
        got = res.got.float().cpu().numpy() if res.kind == "out" else res.got.numpy()
        err = rel_l2(got, res.want.numpy())
        print(f"{where} {res.name}: {err:.2e} (< {res.tol:.1e})")
        assert err < res.tol, (where, res.name, err, res.tol)


@pytest.mark.parametrize("r,mode", CASES)
def test_variant_against_float64_and_the_default(r, mode):
    from fusion_gcn_amd import ops
    run = RUNNERS[r.case]
    with ops.math_mode(mode):
        for shape in r.shapes:
            with tuned(*r.with_keys[0], *r.with_keys[1:]) if r.with_keys else tuned(r.key, 0):
                default = run(shape, mode)
                check_against_float64(default, f"key {r.key} default {shape}")
                for value in values_of(r, shape):
                    with tuned(r.key, value):
                        variant = run(shape, mode)
                    where = f"key {r.key} = {value} {shape}"
                    check_against_float64(variant, where)
                    assert [v.name for v in variant] == [d.name for d in default]
                    for v, d in zip(variant, default):
                        if v.kind == "out":
                            if r.order_only:
                                assert torch.equal(v.got, d.got), (where, v.name, "not the default's bits")
                            else:
                                assert rel_l2(v.got.float().cpu().numpy(), d.got.float().cpu().numpy()) < v.tol, (where, v.name)
                        elif r.sums_bitwise:
                            assert torch.equal(v.raw, d.raw), (where, v.name, "not the default's partial sums")
                        else:
                            assert rel_l2(v.got.numpy(), d.got.numpy()) < v.tol, (where, v.name)


@pytest.mark.parametrize("shape", VT.SPATIAL_FWD_OLD)
def test_the_older_spatial_forward_is_not_selected_with_the_f16x2_products(shape):
    """Tuning key 7 bit 0 selects spatial_fwd_kernel<CI, CO, 2>, which reads the three-part bf16 weights.  With FGCN_PRODUCTS_F16X2 the weights
    are the two-part f16 form behind a 16-byte header: the launcher used to hand them to that kernel all the same (finite, wrong results); it
    now keeps the f16x2 kernel, so the bit changes no bit there."""
    from fusion_gcn_amd import ops
    with ops.math_mode("f16x2"):
        default = run_spatial_fwd(shape, "f16x2")
        with tuned(7, 1):
            variant = run_spatial_fwd(shape, "f16x2")
        check_against_float64(variant, f"key 7 = 1, f16x2 {shape}")
        for v, d in zip(variant, default):
            assert torch.equal(v.got if v.kind == "out" else v.raw, d.got if d.kind == "out" else d.raw), v.name
