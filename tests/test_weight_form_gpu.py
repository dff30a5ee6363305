"""The layout of a weight argument is an ARGUMENT (`w_form` of fgcn_tconv_halo / fgcn_pw_gemm / fgcn_spatial_fwd, include/fgcn.h "Product
form"), not a context setting that a wrapper writes around the call:

  * no kernel call changes the context it runs in -- math mode, product form and the 32 tuning keys read the same before and after it;
  * the form follows the weights -- FGCN_PACK_SPLIT3 and FGCN_PACK_SPLIT2H forms of one matrix, handed to the same kernels in turn inside ONE
    bf16x3 context, each give bit for bit what the call gives alone in a fresh context of the mode the form belongs to;
  * a form the math mode does not take is an error, not a run on weights read in another layout.

The smallest shapes these kernels take (B = 2, T = 8, V = 5, 32 -> 64 channels; three taps for the convolution and its weight gradient,
one for the 1x1 products); the tile kernels at the smallest sizes their `*_available` queries accept (V = 16, 64 -> 64 channels).  Every
tensor is a guarded allocation (tests/guarded.py): a weight buffer bounded at the wrong number of bytes per weight shows up as NaN results
or a damaged margin, not as a passing test."""
import pytest
import torch

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]

B, T, V, K, N, KT = 2, 8, 5, 32, 64, 3
TV, TC = 16, 64                      # the tile kernels: 16 <= V <= 32, whole 64-channel groups


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def gpu(x):
    return guarded.put(x.float(), device=dev())


def out(*shape):
    return guarded.put(torch.zeros(*shape), device=dev())


def settings():
    """what a kernel call must leave alone: the three readings of the calling thread's current context"""
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    return lib.fgcn_get_math_mode(), lib.fgcn_get_products(), tuple(lib.fgcn_get_tuning(k) for k in range(32))


def conv_forms(w):
    """the FGCN_PACK_SPLIT3 and FGCN_PACK_SPLIT2H forms of a packed (taps, K, N) matrix"""
    from fusion_gcn_amd import ops
    return {"split3": ops.pack_split3(w), "split2h": ops.pack_split2h(w)}


def spatial_forms(wd, cin):
    """the accumulator-ordered forms of the stacked (3 cin, N) matrix, as the two modes' ``pack_spatial`` builds them"""
    from fusion_gcn_amd import ops
    forms = {}
    for mode, name in (("bf16x3", "split3_acc"), ("f16x2", "split2h_acc")):
        with ops.context(mode):
            forms[name] = ops.pack_spatial(wd, cin)
    return forms


def amax_slots(a, g):
    """the operand scales of a weight gradient, as tconv_halo / pw_gemm record them: the float bits of max |a| and max |g|"""
    slots = torch.stack([a.abs().max(), g.abs().max()]).view(torch.int32)
    return slots[0:1], slots[1:2]


def eval_vec(C, seed):
    mean, var = rnd(C, seed=seed, scale=0.2), rnd(C, seed=seed + 1).abs() + 0.5
    gamma, beta = rnd(C, seed=seed + 2) * 0.3 + 1.0, rnd(C, seed=seed + 3, scale=0.2)
    rstd = (var + 1e-5).rsqrt()
    return torch.stack([mean, rstd, gamma * rstd, beta - mean * gamma * rstd])


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
def test_no_kernel_call_changes_the_context(mode):
    """fgcn_get_math_mode(), fgcn_get_products() and fgcn_get_tuning(0..31) before and after each call, in a context of each split mode:
    tconv_halo, pw_gemm and spatial_fwd with every weight form the mode takes; the 1x1 and the three-tap weight gradient with and without
    operand scales; tconv_halo_bn_relu, spatial_fwd_tile and spatial_bwd_tile where the mode has them."""
    from fusion_gcn_amd import ops
    x, g = gpu(rnd(B, T, V, K, seed=1)), gpu(rnd(B, T, V, N, seed=2))
    wt = conv_forms(gpu(rnd(KT, K, N, seed=3, scale=(KT * K) ** -0.5)))
    w1 = conv_forms(gpu(rnd(1, K, N, seed=4, scale=K ** -0.5)))
    a_hat = gpu(rnd(B, 3, V, V, seed=5, scale=0.3))
    wd = spatial_forms(gpu(rnd(3 * K, N, seed=6, scale=(3 * K) ** -0.5)), K)
    wd_k4 = gpu(rnd(3 * 4, N, seed=7))
    xt, dyt, at = gpu(rnd(B, T, TV, TC, seed=8)), gpu(rnd(B, T, TV, TC, seed=9)), gpu(rnd(B, 3, TV, TV, seed=10, scale=0.3))
    wt3 = ops.pack_split3(gpu(rnd(1, 3 * TC, TC, seed=11, scale=(3 * TC) ** -0.5)))      # the forward's [k Cin + c][o]
    wb3 = ops.pack_split3(gpu(rnd(1, TC, 3 * TC, seed=17, scale=TC ** -0.5)))            # the backward's [o][k Cin + c]
    vec, bias = gpu(eval_vec(N, 12)), gpu(rnd(N, seed=16))

    with ops.context(mode):
        assert ops.get_math_mode() == mode
        calls = []
        for name in ("split3", "split2h"):
            amax = torch.zeros(1, device=dev(), dtype=torch.int32) if name == "split2h" else None
            calls += [
                (f"tconv_halo {name}", lambda name=name, amax=amax: ops.tconv_halo(x, wt[name], out(B, T, V, N), Th=T, taps=KT, tb=1, tc=-1, amax_out=amax)),
                (f"pw_gemm {name}", lambda name=name, amax=amax: ops.pw_gemm(x, w1[name], out(B, T, V, N), amax_out=amax)),
                (f"spatial_fwd {name}_acc", lambda name=name: ops.spatial_fwd(x, a_hat, wd[name + "_acc"], None, Cin=K, Cout=N)),
            ]
        calls.append(("spatial_fwd k4", lambda: ops.spatial_fwd(x[..., :4].contiguous(), a_hat, ops.pack_spatial(wd_k4, 4), None, Cin=4, Cout=N)))
        for tag, amax in (("", None), (" amax", amax_slots(x, g))):
            calls += [
                ("rows_wgrad 1x1" + tag, lambda amax=amax: ops.rows_wgrad(x, g, K=K, N=N, amax=amax)),
                ("tconv_wgrad" + tag, lambda amax=amax: ops.tconv_wgrad(x, g, taps=KT, amax=amax)),
            ]
        assert ops.spatial_bwd_tile_available(TV, TC, TC)
        calls.append(("spatial_bwd_tile", lambda: ops.spatial_bwd_tile(dyt, xt, at, wb3, out(B, T, TV, TC), accumulate=False)))
        if mode == "bf16x3":          # (mode f16x2 has neither inference form nor the tile form of the forward: it keeps FGCN_PACK_SPLIT2H weights)
            assert ops.inference_kernels_available() and ops.spatial_fwd_tile_available(TV, TC, TC)
            calls += [
                ("tconv_halo_bn_relu", lambda: ops.tconv_halo_bn_relu(x, wt["split3"], out(B, T, V, N), taps=KT, tb=1, tc=-1, vec=vec, bias=bias)),
                ("spatial_fwd_tile", lambda: ops.spatial_fwd_tile(xt, at, wt3, None, Cin=TC, Cout=TC)),
            ]
        else:
            assert not ops.inference_kernels_available() and not ops.spatial_fwd_tile_available(TV, TC, TC)
        for tag, call in calls:
            before = settings()
            call()
            assert settings() == before, f"{tag} changed the context in mode {mode}: {before} -> {settings()}"
        assert ops.get_math_mode() == mode
    torch.cuda.synchronize()


def _bits(t):
    assert bool(torch.isfinite(t).all())
    return t.view(torch.int32)


def test_the_form_follows_the_weights():
    """tconv_halo and pw_gemm on the FGCN_PACK_SPLIT3 and FGCN_PACK_SPLIT2H forms of one matrix, 3, 2h, 3, 2h in a single bf16x3 context: every
    output is bitwise the same call made alone in a fresh context of the mode the form belongs to (bf16x3 / f16x2)."""
    from fusion_gcn_amd import ops
    x = gpu(rnd(B, T, V, K, seed=21))
    w = gpu(rnd(KT, K, N, seed=22, scale=(KT * K) ** -0.5))
    wt, w1 = conv_forms(w), conv_forms(w[1:2].contiguous())

    def conv(form):
        o = out(B, T, V, N)
        ops.tconv_halo(x, wt[form], o, Th=T, taps=KT, tb=1, tc=-1)
        return o

    def pw(form):
        o = out(B, T, V, N)
        ops.pw_gemm(x, w1[form], o)
        return o

    alone = {}
    for form, mode in (("split3", "bf16x3"), ("split2h", "f16x2")):
        with ops.context(mode):
            alone[form] = (conv(form), pw(form))
    assert not torch.equal(alone["split3"][0], alone["split2h"][0])       # (the two forms are two arithmetics: the comparison below can tell them apart)
    with ops.context("bf16x3"):
        for i, form in enumerate(("split3", "split2h", "split3", "split2h")):
            assert torch.equal(_bits(conv(form)), _bits(alone[form][0])), (i, form, "tconv_halo")
            assert torch.equal(_bits(pw(form)), _bits(alone[form][1])), (i, form, "pw_gemm")


def test_a_form_the_mode_does_not_take_is_refused():
    """Math mode bf16 reads FGCN_PACK_SPLIT3 weights (their first part): a FGCN_PACK_SPLIT2H form handed to it is an FgcnError that names the form
    and the mode, not a run that reads it as a three-part split; so is an accumulator-ordered form handed to the convolution."""
    from fusion_gcn_amd import _lib, ops
    x = gpu(rnd(B, T, V, K, seed=31))
    w = gpu(rnd(KT, K, N, seed=32))
    with ops.context("bf16"):
        with pytest.raises(_lib.FgcnError, match="FGCN_PACK_SPLIT2H.*FGCN_MATH_BF16"):
            ops.tconv_halo(x, ops.pack_split2h(w), out(B, T, V, N), Th=T, taps=KT, tb=1, tc=-1)
        with pytest.raises(_lib.FgcnError, match="FGCN_PACK_SPLIT2H.*FGCN_MATH_BF16"):
            ops.pw_gemm(x, ops.pack_split2h(w[:1].contiguous()), out(B, T, V, N))
    with ops.context("bf16x3"):
        acc = ops.ScaledWeights(KT, K, N, dev(), acc_order=True)
        with pytest.raises(_lib.FgcnError, match="FGCN_PACK_SPLIT2H_ACC.*FGCN_MATH_BF16X3"):
            ops.tconv_halo(x, acc, out(B, T, V, N), Th=T, taps=KT, tb=1, tc=-1)
