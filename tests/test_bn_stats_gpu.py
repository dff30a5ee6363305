"""BatchNorm batch statistics against float64 when the channels carry an offset.

A. The input stage (block.data_bn, block.patch_input) takes raw sensor units -- metres, pixels, an accelerometer's gravity -- so its
   statistics must not depend on a channel's mean / std ratio r.  Truth is nn.BatchNorm1d in float64 on the CPU; the yardstick is the
   same module in float32 on the CPU on the same inputs (error e_ref).  Every quantity is held to max(floor, 8 e_ref), per group of
   channels that share an r (a norm over all channels would let the r = 3000 channels' magnitude hide the others): the factor 8
   allows for another fixed summation order and cannot admit an r^2 term.  Constant channels must come out with variance zero.
B. The inner producers (GEMM / halo-conv / pointwise / spatial epilogues, col_moments) sum x and x^2 in float32 per row tile; their
   inputs are convolution outputs with modest offsets, and they are held to the r^2 law of that arithmetic: truth is the float64
   moments of the float32 tensor the kernel itself wrote, so the math mode of the products does not enter."""
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2

import guarded
from guarded import guarded_allocations  # noqa: F401  (the fixture)

# every test runs on guarded allocations: NaN around each tensor the host layer creates, margins verified at teardown (tests/guarded.py)
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]

DEV = "cuda:0"
EPS = 1e-5
OFFSETS = (0.0, 3.0, -3.0, 30.0, -30.0, 300.0, -300.0, 3000.0, -3000.0)        # mean / std of a channel group
CONSTS = (0.0, 1.0, 0.1, 1234.5, -3.3e4)                                         # constant channels
# the tolerances tests/test_kernels_gpu.py::test_data_bn_matches_batchnorm1d holds the same quantities to (rstd: a forward quantity)
FLOOR = {"out": 2e-6, "running_mean": 2e-6, "running_var": 2e-6, "rstd": 2e-6, "dgamma": 1e-5, "dbeta": 1e-5, "dx": 2e-5}


# ---- A. the input stage ----------------------------------------------------------------------------------------------------------
def _layout(ch):
    """-> (group index per channel, indices of the constant channels): groups interleaved over the channels, five constants spread
    over the range (at most 5 of at least 60 channels)."""
    assert ch >= 60
    group = np.arange(ch) % len(OFFSETS)
    const = np.array([1, ch // 4, ch // 2, 3 * ch // 4, ch - 2])
    assert len(set(const.tolist())) == len(CONSTS)
    return group, const


def _by_channel(a, dims):
    """(N, M, T, V, C)-ordered values -> (N * T, M * V * C): a column per BatchNorm channel"""
    N, M, T, V, C = dims
    return np.asarray(a, dtype=np.float64).reshape(N, M, T, V, C).transpose(0, 2, 1, 3, 4).reshape(N * T, M * V * C)


def _make_input(dims, seed):
    """float32 (N, M, T, V, C): channel ch = sigma[ch] * (unit noise + r[ch]), the constant channels overwritten"""
    N, M, T, V, C = dims
    ch = M * V * C
    group, const = _layout(ch)
    g = torch.Generator().manual_seed(seed)
    sigma = torch.rand(ch, generator=g, dtype=torch.float64) * 1.5 + 0.5
    r = torch.tensor(OFFSETS, dtype=torch.float64)[torch.from_numpy(group)]
    cols = (torch.randn(N * T, ch, generator=g, dtype=torch.float64) + r) * sigma
    cols[:, torch.from_numpy(const)] = torch.tensor(CONSTS, dtype=torch.float64)
    return cols.reshape(N, T, M, V, C).permute(0, 2, 1, 3, 4).contiguous().float()


def _fresh_bn(ch, seed, dtype=torch.float32):
    bn = torch.nn.BatchNorm1d(ch, eps=EPS, momentum=1.0)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(ch, generator=g) + 0.5), bn.bias.copy_(torch.rand(ch, generator=g) - 0.5)
        bn.running_mean.copy_(torch.rand(ch, generator=g) * 0.6 - 0.3), bn.running_var.copy_(torch.rand(ch, generator=g) * 1.5 + 0.5)
    return bn.to(dtype)


def _torch_step(bn, x32, probe, train):
    """The reference's data_bn (permute / view / nn.BatchNorm1d / view / permute) in the module's dtype on the CPU -> the quantities
    by name, output and dx as a column per channel."""
    N, M, T, V, C = x32.shape
    dims, ch, dt = tuple(x32.shape), M * V * C, bn.weight.dtype
    bn.train(train)
    bn.zero_grad()
    x = x32.detach().clone().to(dt).requires_grad_(True)
    flat = x.permute(0, 1, 3, 4, 2).contiguous().view(N, ch, T)
    if train:           # the batch statistics the module is about to use, in its own arithmetic
        _, _, rstd = torch.native_batch_norm(flat.detach(), bn.weight.detach(), bn.bias.detach(), None, None, True, 1.0, EPS)
        if dt == torch.float64:
            rstd = 1.0 / torch.sqrt(flat.detach().transpose(0, 1).reshape(ch, -1).var(1, unbiased=False) + EPS)
    h = bn(flat).view(N, M, V, C, T).permute(0, 1, 4, 2, 3)                       # (N, M, T, V, C)
    if not train:
        rstd = 1.0 / torch.sqrt(bn.running_var + EPS)
    (h * probe.to(dt)).sum().backward()
    return {"out": _by_channel(h.detach(), dims), "dx": _by_channel(x.grad, dims), "rstd": rstd.double().numpy(),
            "running_mean": bn.running_mean.double().numpy().copy(), "running_var": bn.running_var.double().numpy().copy(),
            "dgamma": bn.weight.grad.double().numpy(), "dbeta": bn.bias.grad.double().numpy()}


def _kernel_step(stage, bn, probe, train, dims):
    """One forward + backward of the input stage on the GPU: stage(bn) -> (output (N*M, T, V, Cp), x leaf or None)"""
    N, M, T, V, C = dims
    bn.train(train)
    bn.zero_grad()
    out, leaf = stage(bn)
    vec = out.grad_fn.saved_tensors[1]                      # the (4, ch) coefficient vector the stage computed: mean, rstd, scale, shift
    assert tuple(vec.shape) == (4, M * V * C)
    rstd = vec[1].double().cpu().numpy()
    assert out.shape == (N * M, T, V, (C + 3) // 4 * 4) and float(out[..., C:].abs().sum()) == 0.0
    pad = torch.zeros(out.shape, dtype=torch.float32)
    pad[..., :C] = probe.reshape(N * M, T, V, C)
    (out * guarded.to(pad, DEV)).sum().backward()
    torch.cuda.synchronize()
    q = {"out": _by_channel(out[..., :C].detach().cpu(), dims), "rstd": rstd,
         "running_mean": bn.running_mean.double().cpu().numpy(), "running_var": bn.running_var.double().cpu().numpy(),
         "dgamma": bn.weight.grad.double().cpu().numpy(), "dbeta": bn.bias.grad.double().cpu().numpy()}
    if leaf is not None:
        q["dx"] = _by_channel(leaf.grad.cpu(), dims)
    raw = [out.detach().clone(), bn.running_mean.clone(), bn.running_var.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]
    if leaf is not None:
        raw.append(leaf.grad.clone())
    return q, raw


def _compare(tag, got, ref32, truth, ch, names):
    """Per quantity and channel group: err(kernel), e_ref = err(torch float32) against float64, the bound max(floor, 8 e_ref).
    The constant channels stay out of the output and dx norms only (there the float64 answer is ill-conditioned: zero times
    eps^-1/2).  Every figure is printed before anything is asserted."""
    group, const = _layout(ch)
    live = np.ones(ch, dtype=bool)
    live[const] = False
    bad = []
    for name in names:
        for gi, r in enumerate(OFFSETS):
            sel = group == gi
            if name in ("out", "dx"):
                sel = sel & live
            err = rel_l2(got[name][..., sel], truth[name][..., sel])
            e_ref = rel_l2(ref32[name][..., sel], truth[name][..., sel])
            bound = max(FLOOR[name], 8.0 * e_ref)
            print(f"{tag} {name:12s} r={r:7.0f}  kernel {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}{'  <-- FAIL' if not err <= bound else ''}")
            if not err <= bound:
                bad.append((name, r, err, e_ref, bound))
    return bad


def _check_constants(tag, got, ref32, ch, train):
    _, const = _layout(ch)
    bad = []
    assert np.isfinite(got["out"]).all(), f"{tag}: non-finite output"
    for idx, c in zip(const, CONSTS):
        c32 = float(np.float32(c))
        rstd, mean, var, var32 = got["rstd"][idx], got["running_mean"][idx], got["running_var"][idx], ref32["running_var"][idx]
        print(f"{tag} constant {c:10g}: rstd {rstd:.6e} (eps^-1/2 = {EPS ** -0.5:.6e})  mean - c {mean - c32:.3e}  running_var {var:.3e}"
              f"  torch float32 {var32:.3e}")
        if not abs(rstd * math.sqrt(EPS) - 1.0) <= 2e-6:
            bad.append(("rstd", c, rstd))
        if train and not abs(mean - c32) <= 2.0 ** -24 * abs(c32):                  # one float32 rounding
            bad.append(("running_mean", c, mean))
        if train and not abs(var - var32) <= (2.0 ** -23 * abs(c32)) ** 2:
            bad.append(("running_var", c, var, var32))
    return bad


def _input_stage_contract(dims, stage_of, seed, has_dx=True):
    """Train step (momentum 1.0, so the running statistics are the batch's), the same step again (same bits), then an eval forward
    and backward on the running statistics that train step left -- which is where a poisoned running_var would show."""
    N, M, T, V, C = dims
    ch = M * V * C
    x32 = _make_input(dims, seed)
    probe = torch.randn(N, M, T, V, C, generator=torch.Generator().manual_seed(seed + 1)).double()     # float32 values
    names = ["out", "running_mean", "running_var", "rstd", "dgamma", "dbeta"] + (["dx"] if has_dx else [])
    bn64, bn32, mine, twin = (_fresh_bn(ch, seed + 2, torch.float64), _fresh_bn(ch, seed + 2), guarded.to(_fresh_bn(ch, seed + 2), DEV),
                              guarded.to(_fresh_bn(ch, seed + 2), DEV))
    stage = stage_of(x32)
    bad = []
    for train in (True, False):
        tag = f"{dims} {'train' if train else 'eval after train'}"
        truth, ref32 = _torch_step(bn64, x32, probe, train), _torch_step(bn32, x32, probe, train)
        got, raw = _kernel_step(stage, mine, probe, train, dims)
        got2, raw2 = _kernel_step(stage, twin, probe, train, dims)
        for a, b in zip(raw, raw2):
            assert torch.equal(a, b), f"{tag}: a second identical call gave other bits"
        bad += _compare(tag, got, ref32, truth, ch, names)
        bad += _check_constants(tag, got, ref32, ch, train)
        assert int(mine.num_batches_tracked) == int(bn64.num_batches_tracked) == 1
    assert not bad, bad


def _data_bn_stage(x32):
    from fusion_gcn_amd.block import data_bn

    def stage(bn):
        leaf = guarded.to(x32, DEV).requires_grad_(True)
        return data_bn(leaf, bn), leaf
    return stage


DATA_BN_SHAPES = [(3, 2, 37, 25, 3), (2, 1, 8, 22, 9), (1, 1, 2, 20, 3),                                  # (the last: a count of 2)
                  (2, 1, 31, 20, 3), (2, 1, 32, 20, 3), (2, 1, 33, 20, 3), (2, 1, 65, 20, 3),            # the tails of the 32-frame tile
                  (2, 2, 33, 64, 3), (2, 2, 16, 32, 9),                                                    # 384 / 576 channels > 256 threads
                  (16, 1, 1, 12, 40), (2, 1, 1, 6, 50)]                                                    # the IMU layout: one sample per tile


@pytest.mark.parametrize("dims", DATA_BN_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_data_bn_statistics_are_flat_in_the_offset(dims):
    """block.data_bn on channels with mean / std ratios 0 .. 3000 in both signs and five constant channels, train and eval.

    Measured on the MI355X at (3, 2, 37, 25, 3), train: relative L2 of rstd per channel group against float64 --
        r        this kernel   torch float32 (e_ref)   float32 sums of x and x^2 per tile (the kernel before the pivot)
        0        2.4e-8        2.5e-8                  2.3e-8
        3 / -3   5.4e-8 / 2.7e-8   4.2e-8 / 2.8e-8     5.4e-8 / 5.7e-7
        30 / -30     5.4e-8 / 5.4e-8   4.2e-8 / 4.2e-8     2.4e-4 / 7.0e-1
        300 / -300   2.5e-8 / 2.8e-8   2.8e-8 / 3.4e-8     5.6e-3 / 5.5e-3
        3000 / -3000 2.6e-8 / 2.5e-8   2.7e-8 / 2.5e-8     9.0e+1 / 7.1e+1
    and the channel that is 1234.5 everywhere: variance 0 (rstd 316.23 = eps^-1/2) against 0.32 (rstd 1.77) before."""
    _input_stage_contract(dims, _data_bn_stage, seed=sum(dims))


def test_patch_input_statistics_are_flat_in_the_offset():
    """block.patch_input (the fused input stage: fgcn_patch_input_fwd leaves data_bn's partials) with offset skeleton and patch rows:
    concatenation with the identity reducer, so z = [s | p] is exact and the float64 truth is the BatchNorm of z."""
    from fusion_gcn_amd import ops
    from fusion_gcn_amd.block import patch_input
    N, M, T, V, Cs, P = 2, 2, 40, 20, 3, 4
    dims = (N, M, T, V, Cs + P)
    assert ops.paths().get("patch_input_fused", ops.get_math_mode())

    def stage_of(z32):
        s, p = guarded.to(z32[..., :Cs].contiguous(), DEV), guarded.to(z32[..., Cs:].contiguous(), DEV)

        def stage(bn):
            return patch_input(s, p, None, bn, V, "concatenate"), None
        return stage
    _input_stage_contract(dims, stage_of, seed=77, has_dx=False)


def test_data_bn_under_graph_capture_gives_eager_bits():
    """One torch.cuda.graph capture and replay of data_bn in train mode: the same bits as the eager call, running statistics
    included -- the stage has no host synchronisation (a capture would raise on one)."""
    from fusion_gcn_amd.block import data_bn
    dims = (3, 2, 37, 25, 3)
    ch = dims[1] * dims[3] * dims[4]
    x = guarded.to(_make_input(dims, seed=5), DEV)
    eager, warm, captured = (guarded.to(_fresh_bn(ch, 9), DEV).train() for _ in range(3))
    with torch.no_grad():
        want = data_bn(x, eager)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            data_bn(x, warm)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = data_bn(x, captured)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(captured.running_mean, eager.running_mean) and torch.equal(captured.running_var, eager.running_var)
    assert int(captured.num_batches_tracked) == int(eager.num_batches_tracked) == 1


# ---- B. the inner producers ------------------------------------------------------------------------------------------------------
B_, T_, V_, CIN, COUT = 2, 13, 25, 64, 64           # 650 rows: a ragged last tile at 64, 128 and 192 rows per tile and at whole frames
DRIVES = (("none", 0.0), ("bias", 3.0), ("bias", 30.0), ("data", 3.0), ("data", 30.0))


def _gpu(t):
    return guarded.put(t.float(), device=DEV)


def _nonneg(shape, q, gen):
    """non-negative values with mean / std = q: a constant plus uniform noise where that stays >= 0 (q >= sqrt(3)), else a
    Bernoulli(p) mask of uniform(0.5, 1.5) values (mean p, second moment 13 p / 12)"""
    u = torch.rand(shape, generator=gen, dtype=torch.float64)
    if q >= 1.74:
        return u - 0.5 + q / math.sqrt(12.0)
    p = (13.0 / 12.0) * q * q / (1.0 + q * q)
    return (torch.rand(shape, generator=gen, dtype=torch.float64) < p) * (u + 0.5)


def _operands(drive, r, k_eff, x_shape, w_shape, gen, center_tap=None):
    """-> (x, w, bias) float64.  "bias": unit-variance products, the offset r in the bias (alternating sign over the channels).
    "data": non-negative inputs times positive weights, no bias -- the offset is in the accumulators; the sum of k_eff such terms has
    mean / std ~ q sqrt(k_eff), so q = r / sqrt(k_eff).  A multi-tap conv gets its weight on the centre tap (1e-3 of it elsewhere):
    with zero padding the frames at a sample's ends would otherwise see fewer taps and their mean, not the noise, would be the spread."""
    n_out = w_shape[-1]
    if drive == "data":
        x = _nonneg(x_shape, r / math.sqrt(k_eff), gen)
        w = torch.rand(w_shape, generator=gen, dtype=torch.float64) + 0.5
        if center_tap is not None:
            w[:center_tap] *= 1e-3
            w[center_tap + 1:] *= 1e-3
        # unit output spread: std = std(x) * sqrt(sum w^2) per output channel
        w = w / (x.std() * math.sqrt(k_eff) * math.sqrt(13.0 / 12.0))
        return x, w, None
    x = torch.randn(x_shape, generator=gen, dtype=torch.float64)
    w = torch.randn(w_shape, generator=gen, dtype=torch.float64) / math.sqrt(k_eff)
    bias = r * (1.0 - 2.0 * (torch.arange(n_out) % 2).double()) + 0.1 * torch.randn(n_out, generator=gen, dtype=torch.float64)
    return x, w, bias


def _temporal(kind, kt, s):
    def run(drive, r, gen):
        from fusion_gcn_amd import ops
        from fusion_gcn_amd.block import temporal_fwd
        Tp = (T_ - 1) // s + 1
        x, w, bias = _operands(drive, r, CIN if drive == "data" else kt * CIN, (B_, T_, V_, CIN), (kt, CIN, COUT), gen,
                               center_tap=(kt - 1) // 2 if kt > 1 else None)
        out = torch.full((B_, Tp, V_, COUT), 3.0, device=DEV)
        bg = None if bias is None else _gpu(bias)
        if kind == "rows":
            part = ops.rows_gemm(_gpu(x), _gpu(w), out, K=CIN, N=COUT, tmap=ops.conv_tmap(kt, s), bias=bg, stats=True)
        else:
            wg = _gpu(w)
            W = {"t4": ops.pack_conv(wg)} if s == 1 else {f"t4_{tag}": ops.pack_conv(wg[par::2].contiguous()) for par, tag in ((0, "e"), (1, "o"))}
            if bg is None:
                bg = torch.zeros(COUT, device=DEV)
            part = temporal_fwd(_gpu(x), out, W, bg, kt, s, stats=True, route="halo" if s == 1 else "halo_parity")
        return out, part
    return run


def _pointwise(drive, r, gen):
    from fusion_gcn_amd import ops
    x, w, bias = _operands(drive, r, CIN, (B_ * T_ * V_, 1, 1, CIN), (1, CIN, COUT), gen)
    out = torch.full((B_ * T_ * V_, 1, 1, COUT), 3.0, device=DEV)
    part = ops.pw_gemm(_gpu(x), ops.pack_conv(_gpu(w)), out, bias=None if bias is None else _gpu(bias), stats=True)
    return out, part


def _spatial(tile):
    def run(drive, r, gen):
        from fusion_gcn_amd import ops
        # y = sum_k (x . A_k) . W_k: every x[v, c] enters once per output (through sum_k A_k[v, w] W_k[c, o]): V * Cin terms
        x, w, bias = _operands(drive, r, V_ * CIN, (B_, T_, V_, CIN), (3, CIN, COUT), gen)
        if drive == "data":     # positive adjacency, every column of every subset summing to 1 / 3: the same mean at every joint
            a = torch.rand(B_, 3, V_, V_, generator=gen, dtype=torch.float64) + 0.5
            a = a / a.sum(2, keepdim=True) / 3.0
            w = w * V_          # each x[v, c] arrives with a weight ~ W / V: unit spread again
        else:
            a = torch.randn(B_, 3, V_, V_, generator=gen, dtype=torch.float64) / math.sqrt(3.0)
        bg = None if bias is None else _gpu(bias)
        if tile:
            assert ops.spatial_fwd_tile_available(V_, CIN, COUT)
            w3 = ops.pack_split3(_gpu(w.reshape(1, 3 * CIN, COUT)))
            return ops.spatial_fwd_tile(_gpu(x), _gpu(a), w3, bg, Cin=CIN, Cout=COUT, stats=True)
        return ops.spatial_fwd(_gpu(x), _gpu(a), ops.pack_spatial(_gpu(w.reshape(3 * CIN, COUT)), CIN), bg, Cin=CIN, Cout=COUT, stats=True)
    return run


def _moments(drive, r, gen):
    from fusion_gcn_amd import ops
    shape = (1, B_ * T_ * V_, 1, COUT)
    if drive == "data":
        x = _nonneg(shape, r, gen)
        x = x / x.std()
    else:
        x = torch.randn(shape, generator=gen, dtype=torch.float64) + r * (1.0 - 2.0 * (torch.arange(COUT) % 2).double())
    xg = _gpu(x)
    return xg, ops.col_moments(xg)


PRODUCERS = [("rows_gemm-1x1-s1", "f32", _temporal("rows", 1, 1)), ("rows_gemm-1x1-s2", "f32", _temporal("rows", 1, 2)),
             ("rows_gemm-9x1-s1", "f32", _temporal("rows", 9, 1)), ("rows_gemm-9x1-s2", "f32", _temporal("rows", 9, 2)),
             ("tconv_halo-s1", "f32", _temporal("halo", 9, 1)), ("tconv_halo-s1", "bf16x3", _temporal("halo", 9, 1)),
             ("tconv_halo-parity-s2", "f32", _temporal("halo", 9, 2)), ("tconv_halo-parity-s2", "bf16x3", _temporal("halo", 9, 2)),
             ("pw_gemm", "bf16x3", _pointwise), ("spatial_fwd", "f32", _spatial(False)), ("spatial_fwd", "bf16x3", _spatial(False)),
             ("spatial_fwd_tile", "bf16x3", _spatial(True)), ("col_moments", "f32", _moments)]


@pytest.mark.parametrize("name,mode,run", PRODUCERS, ids=[f"{n}-{m}" for n, m, _ in PRODUCERS])
def test_inner_producer_statistics_follow_the_r2_law(name, mode, run):
    """Each producer's BatchNorm partials, finalised by ops.bn_finalize, against the float64 moments of the float32 tensor it wrote,
    with the offset r = |mean| / std driven through the conv bias and through the data (r = 0, 3, 30):
        |mean - mean64| <= 2e-6 std + 2^-23 |mean|        |rstd / rstd64 - 1| <= 2e-6 + 2 sqrt(n_t) 2^-24 (1 + r^2)
    n_t = the rows of a partial tile (the library's tile count for these rows).  The second term is the float32 rounding of a sum of
    n_t non-negative terms (x^2), sqrt(n_t) 2^-24 relative in the typical case, with 4x slack, as it reaches var = E x^2 - mean^2
    (amplified by E x^2 / var = 1 + r^2) and then rstd (half of var's relative error); r is the channel's own, from the float64
    moments.  A dropped tail row or a tile counted twice is outside it at every r."""
    from fusion_gcn_amd import ops
    bad = []
    with ops.math_mode(mode):
        for i, (drive, r_nominal) in enumerate(DRIVES):
            gen = torch.Generator().manual_seed(1000 + i)
            out, part = run(drive, r_nominal, gen)
            assert out.dtype == torch.float32 and part.shape[1:] == (2, COUT)
            y = out.reshape(-1, COUT).double().cpu()
            rows = y.shape[0]
            n_t = -(-rows // part.shape[0])
            gamma, beta = torch.ones(COUT, device=DEV), torch.zeros(COUT, device=DEV)
            vec = ops.bn_finalize(part, rows, gamma, beta).double().cpu()
            mean64, var64 = y.mean(0), y.var(0, unbiased=False)
            std64, rstd64 = var64.sqrt(), 1.0 / torch.sqrt(var64 + EPS)
            r = mean64.abs() / std64
            e_mean = (vec[0] - mean64).abs()
            b_mean = 2e-6 * std64 + 2.0 ** -23 * mean64.abs()
            e_rstd = (vec[1] / rstd64 - 1.0).abs()
            b_rstd = 2e-6 + 2.0 * math.sqrt(n_t) * 2.0 ** -24 * (1.0 + r * r)
            km, kr = int((e_mean / b_mean).argmax()), int((e_rstd / b_rstd).argmax())
            print(f"{name} {mode} {drive} r={r_nominal:g}: rows {rows} tiles {part.shape[0]} n_t {n_t}  r of the output {float(r.min()):.2f} .. "
                  f"{float(r.max()):.2f}  std {float(std64.median()):.3f}  worst mean err {float(e_mean[km]):.3e} (bound {float(b_mean[km]):.3e})"
                  f"  worst rstd err {float(e_rstd[kr]):.3e} (bound {float(b_rstd[kr]):.3e})")
            if drive != "none":         # the case is what it says: the offset reached the output
                assert float(r.median()) >= 0.5 * r_nominal, (name, drive, r_nominal, float(r.median()))
            if not bool((e_mean <= b_mean).all()):
                bad.append((drive, r_nominal, "mean", float(e_mean[km]), float(b_mean[km])))
            if not bool((e_rstd <= b_rstd).all()):
                bad.append((drive, r_nominal, "rstd", float(e_rstd[kr]), float(b_rstd[kr])))
    assert not bad, bad
