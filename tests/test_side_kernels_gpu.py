"""Direct tests of entry points that so far ran only inside whole-model comparisons: fgcn_transpose (ops.transpose / transpose_into),
fgcn_row_softmax_fwd / _bwd, fgcn_reduce_multi in its two per-item forms (ops.ReduceBatch, ops._reduce_slabs, ops.reduce_sum), the tails of
ops.group_mean / ops.col_sum, and the elementwise reductions past the 1024-tile cap of fgcn_elem_tiles -- against float64 torch, in math mode f32, on guarded allocations (tests/guarded.py): every input and output has
NaN in front of its first and behind its last element, and the margins are verified at teardown."""
import pytest
import torch

import guarded
from conftest import rel_l2
from guarded import guarded_allocations  # noqa: F401  (the fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("guarded_allocations")]

RED_TOL = 2e-5          # the reduction tolerance of tests/test_kernels_gpu.py
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


def put(t):
    return guarded.put(t.float(), device=dev())


# ---- fgcn_transpose --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,R,C,ld_out", [(3, 25, 64, 32), (2, 33, 5, 64), (2, 70, 96, 128), (1, 32, 32, 32), (5, 1, 1, 4), (1, 652, 3, 704)])
def test_transpose_and_its_inverse(B, R, C, ld_out):
    """out[b, c, r] == x[b, r, c] exactly, the columns [R, ld_out) exactly +0.0, and transpose_into (input rows wider than its columns:
    ld_in = ld_out > R) gives x back bit for bit.  (ops.transpose itself offers no input row stride: its ld_in is C.)"""
    from fusion_gcn_amd import ops
    x = rnd(B, R, C, seed=R * 131 + C)
    xg = put(x)
    out = ops.transpose(xg, ld_out)
    assert tuple(out.shape) == (B, C, ld_out) and out.is_contiguous()
    got = out.cpu()
    assert torch.equal(got[:, :, :R], x.transpose(1, 2))
    pad = got[:, :, R:]
    assert bool((pad == 0).all()) and not bool(torch.signbit(pad).any())
    back = ops.transpose_into(out, R)
    assert tuple(back.shape) == (B, R, C) and torch.equal(back.cpu(), x)
    tight = ops.transpose(xg)                        # ld_out = R: no padding column
    assert tuple(tight.shape) == (B, C, R) and torch.equal(tight.cpu(), x.transpose(1, 2))


# ---- fgcn_row_softmax_fwd / _bwd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,V,ld,std", [(2, 3, 25, 28, 1), (2, 3, 65, 68, 60), (1, 1, 64, 64, 60), (2, 3, 300, 304, 60), (1, 3, 652, 656, 200),
                                          (2, 3, 1, 4, 60)])
def test_row_softmax_forward_and_backward(B, K, V, ld, std):
    """c = softmax(scale * st[..., :V]) over the last axis, a = c + adj_t, ds by autograd, against float64 of the float32-rounded inputs at the
    column softmax's tolerances (test_joint_gram_and_adjacency_softmax): rel-L2 < 1e-5 for c and a, < 2e-5 for ds, row sums within 1e-5 of 1.
    The padding columns [V, ld) of the INPUTS hold NaN (the kernels must not read them), those of c, a and ds must be exactly zero."""
    from fusion_gcn_amd import ops
    scale = 1.0 / 16
    st = torch.full((B, K, V, ld), NAN)
    adj = torch.full((K, V, ld), NAN)
    da = torch.full((B, K, V, ld), NAN)
    st[..., :V] = rnd(B, K, V, V, seed=V, scale=std)
    adj[..., :V] = rnd(K, V, V, seed=V + 1, scale=0.2)
    da[..., :V] = rnd(B, K, V, V, seed=V + 2)
    s64 = st[..., :V].double().requires_grad_(True)
    c_want = torch.softmax(scale * s64, dim=-1)
    a_want = c_want + adj[..., :V].double()
    ds_want, = torch.autograd.grad((a_want * da[..., :V].double()).sum(), s64)
    c, a = ops.row_softmax_fwd(put(st), put(adj), V, scale)
    ds = ops.row_softmax_bwd(put(da), c, V, scale)
    c, a, ds = c.cpu(), a.cpu(), ds.cpu()
    for t in (c, a, ds):
        assert tuple(t.shape) == (B, K, V, ld) and bool(torch.isfinite(t).all())
        assert bool((t[..., V:] == 0).all())
    errs = (rel_l2(c[..., :V].numpy(), c_want.detach().numpy()), rel_l2(a[..., :V].numpy(), a_want.detach().numpy()))
    sums = float((c[..., :V].double().sum(-1) - 1).abs().max())
    print(f"row_softmax V={V} std={std}: c {errs[0]:.2e} a {errs[1]:.2e} row sums {sums:.2e}")
    assert errs[0] < 1e-5 and errs[1] < 1e-5 and sums <= 1e-5
    if V == 1:
        assert bool((c[..., :V] == 1).all()) and bool((ds == 0).all())
    else:
        e_ds = rel_l2(ds[..., :V].numpy(), ds_want.numpy())
        print(f"    ds {e_ds:.2e}")
        assert e_ds < 2e-5


# ---- fgcn_reduce_multi -----------------------------------------------------------------------------------------------------------------------
def takes_vec_form(S, taps, K, N, src) -> bool:
    """the host's selection rule of fgcn_reduce_multi, restated: the four-elements-per-thread form, else the 16-lane form.  The form is INFERRED
    from this copy of the rule, not observed: it only places the items on both sides of each clause as the rule stands in fgcn_gemm.hip today.
    If the rule there moves, every result is still compared with float64, but an item may then run in the other form than its label says."""
    count = taps * K * N
    return S <= 128 and N % 4 == 0 and count >= 4096 and count % 4 == 0 and src.data_ptr() % 16 == 0


class Item:
    """One synthetic slab sum: src (S, taps, K, N), a destination pre-filled with a sentinel (accumulate: with known values) that is larger than
    what the item addresses, and the float64 expectation.  layout: "plain" (taps, K, N) | "conv" = conv_param=(1, K_dst), the parameter layout
    (N, K_dst, taps, 1) | "groups" = conv_param=(taps, K_dst): (taps, N, K_dst, 1, 1), as ops._reduce_slabs builds them"""
    SENTINEL = -3.5
    TAIL = 24                  # elements behind the last addressed one that must stay as they are

    def __init__(self, S, taps, K, N, K_dst=None, layout="plain", accumulate=False, offset=0, seed=0):
        self.S, self.taps, self.K, self.N, self.accumulate = S, taps, K, N, accumulate
        self.K_dst = K_dst = K if K_dst is None else K_dst
        count = taps * K * N
        src = rnd(S * count + offset, seed=1000 + seed)
        self.src_all = put(src)
        self.src = self.src_all[offset:].view(S, taps, K, N)          # offset = 1: a source that is not 16-byte aligned
        if layout == "plain":
            self.strides, size = (K * N, N, 1), taps * K * N          # (rows K_dst..K of every tap are not addressed)
        elif layout == "conv":
            self.strides, size = (1, taps, K_dst * taps), N * K_dst * taps
        else:
            self.strides, size = (N * K_dst, 1, K_dst), taps * N * K_dst
        t, k, n = torch.meshgrid(torch.arange(taps), torch.arange(K_dst), torch.arange(N), indexing="ij")
        self.idx = (t * self.strides[0] + k * self.strides[1] + n * self.strides[2]).flatten()
        assert int(self.idx.max()) < size and self.idx.unique().numel() == self.idx.numel()
        self.prefill = rnd(size + self.TAIL, seed=2000 + seed) if accumulate else torch.full((size + self.TAIL,), self.SENTINEL)
        self.dst = put(self.prefill)
        total = src[offset:].view(S, taps, K, N).double().sum(0)[:, :K_dst, :].flatten()
        self.want = total + (self.prefill[self.idx].double() if accumulate else 0)
        self.untouched = torch.ones(size + self.TAIL, dtype=torch.bool)
        self.untouched[self.idx] = False
        self.vec = takes_vec_form(S, taps, K, N, self.src)

    def add_to(self, batch):
        batch.add(self.dst, self.src, self.S, self.taps, self.K, self.N, self.K_dst, *self.strides, self.accumulate)

    def verify(self, tag=""):
        got = self.dst.cpu()
        err = rel_l2(got[self.idx].numpy(), self.want.numpy())
        print(f"reduce_multi {tag} S={self.S} ({self.taps}, {self.K}, {self.N}) K_dst={self.K_dst} {'vec' if self.vec else 'lane'} form"
              f"{' accumulate' if self.accumulate else ''}: {err:.2e}")
        assert bool(torch.isfinite(got).all()), tag
        assert torch.equal(got[self.untouched], self.prefill[self.untouched]), f"{tag}: an element the item does not address changed"
        assert bool((got[self.idx] != self.prefill[self.idx]).all()), f"{tag}: an addressed element was left as it was"
        assert err < RED_TOL, (tag, err)
        return got


def flush_twice(items):
    """one batch (one launch per eight items), verified; then the destinations restored and the same items once more: the same bits"""
    from fusion_gcn_amd import ops
    first = []
    for rep in range(2):
        batch = ops.ReduceBatch()
        for it in items:
            if rep:
                it.dst.copy_(it.prefill)
            it.add_to(batch)
        batch.flush()
        batch.release()
        if rep == 0:
            first = [it.verify(f"item {i}") for i, it in enumerate(items)]
        else:
            for i, it in enumerate(items):
                assert torch.equal(it.dst.cpu(), first[i]), f"item {i}: the second flush differs from the first"


@pytest.mark.parametrize("S", [1, 7, 8, 9, 16, 17, 112, 113, 129, 300])
def test_reduce_multi_slab_counts(S):
    """Both unroll boundaries (s + 8 <= S in the four-per-thread form, s + 7 * 16 < S in the 16-lane form): one item of each form per launch"""
    a, b = Item(S, 1, 64, 64, seed=S), Item(S, 1, 66, 62, accumulate=True, seed=S + 1)
    assert a.vec == (S <= 128) and not b.vec
    flush_twice([a, b])


@pytest.mark.parametrize("accumulate", [False, True])
def test_reduce_multi_on_both_sides_of_the_selection_rule(accumulate):
    """S <= 128 && N % 4 == 0 && count >= 4096 && count % 4 == 0 && aligned16(src), each clause from both sides"""
    kw = dict(accumulate=accumulate)
    cases = [(Item(16, 1, 64, 64, seed=1, **kw), True), (Item(16, 1, 1023, 4, seed=2, **kw), False),         # count = 4096 / 4092
             (Item(16, 1, 68, 62, seed=3, **kw), False),                                                      # N = 62 (count 4216, % 4 == 0)
             (Item(128, 1, 64, 64, seed=4, **kw), True), (Item(129, 1, 64, 64, seed=5, **kw), False),         # S = 128 / 129
             (Item(16, 1, 64, 64, offset=1, seed=6, **kw), False),                                            # src one float off 16 bytes
             (Item(16, 2, 40, 64, K_dst=33, seed=7, **kw), True), (Item(16, 2, 40, 62, K_dst=33, seed=8, **kw), False)]      # K_dst < K
    for it, vec in cases:
        assert it.vec == vec, (it.S, it.taps, it.K, it.N)
        flush_twice([it])


def test_reduce_multi_eight_items_in_one_launch_and_nine_in_two():
    items = [Item(16, 9, 24, 32, K_dst=20, layout="conv", seed=11),                          # conv_param=(1, 20), nine taps: vec form (6912)
             Item(5, 9, 7, 6, K_dst=5, layout="conv", accumulate=True, seed=12),             # ... lane form
             Item(32, 3, 32, 64, K_dst=30, layout="groups", seed=13),                        # conv_param=(3, 30): vec form (6144)
             Item(130, 3, 8, 10, K_dst=8, layout="groups", accumulate=True, seed=14),        # ... lane form
             Item(64, 1, 1, 4096, seed=15),                                                   # reduce_sum(leaf=True)'s shape: vec
             Item(300, 1, 1, 100, accumulate=True, seed=16),                                  # ... lane
             Item(8, 2, 40, 64, K_dst=33, seed=17), Item(1, 1, 3, 5, seed=18),
             Item(24, 9, 24, 32, layout="conv", accumulate=True, seed=19)]
    assert sum(it.vec for it in items[:8]) == 4 and items[8].vec
    flush_twice(items[:8])
    for it in items:
        it.dst.copy_(it.prefill)
    flush_twice(items)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("slabs,taps,K,N,conv_param", [(16, 9, 64, 96, (1, 64)), (16, 9, 8, 96, (1, 3)), (7, 9, 6, 10, (1, 5)),
                                                        (32, 1, 96, 64, (3, 30)), (9, 1, 12, 6, (3, 3)), (16, 3, 40, 64, None)])
def test_reduce_slabs_parameter_layouts(slabs, taps, K, N, conv_param, accumulate):
    """ops._reduce_slabs itself (it computes the strides): the default (taps, K, N) result and the two parameter layouts, padded input
    channels dropped, with and without accumulation, alone and inside a deferred batch"""
    from fusion_gcn_amd import ops
    partial = rnd(slabs, taps, K, N, seed=slabs + K)
    total = partial.double().sum(0)
    if conv_param is None:
        want = total
    elif conv_param[0] == 1:
        want = total[:, :conv_param[1], :].permute(2, 1, 0).unsqueeze(-1)                                     # (N, K_true, taps, 1)
    else:
        g, kt = conv_param
        want = total[0].reshape(g, K // g, N)[:, :kt, :].permute(0, 2, 1).reshape(g, N, kt, 1, 1)
    base = rnd(*want.shape, seed=77)
    pg = put(partial)
    for deferred in (False, True):
        out = put(base) if accumulate else None
        if deferred:
            with ops.deferred_reductions() as batch:
                got = ops._reduce_slabs(pg, taps, K, N, out, accumulate, conv_param)
                batch.flush()
        else:
            got = ops._reduce_slabs(pg, taps, K, N, out, accumulate, conv_param)
        assert tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
        ref = want + base.double() if accumulate else want
        err = rel_l2(got.cpu().numpy(), ref.numpy())
        print(f"_reduce_slabs {conv_param} deferred={deferred} accumulate={accumulate}: {err:.2e}")
        assert err < RED_TOL


@pytest.mark.parametrize("S,shape", [(1, (5,)), (17, (3, 7)), (64, (64, 64)), (129, (1024, 4)), (300, (33,))])
def test_reduce_sum_alone_and_as_a_leaf(S, shape):
    from fusion_gcn_amd import ops
    src = rnd(S, *shape, seed=S)
    base = rnd(*shape, seed=S + 1)
    want = src.double().sum(0)
    sg = put(src)
    for accumulate in (False, True):
        ref = want + base.double() if accumulate else want
        alone = ops.reduce_sum(sg, put(base), accumulate=accumulate)
        with ops.deferred_reductions() as batch:
            leaf = ops.reduce_sum(sg, put(base), accumulate=accumulate, leaf=True)
            batch.flush()
        for name, got in (("alone", alone), ("leaf", leaf)):
            err = rel_l2(got.cpu().numpy(), ref.numpy())
            assert err < RED_TOL, (name, accumulate, err)


# ---- tails of group_mean and col_sum ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,C", [(1, 1, 4), (3, 50, 68), (2, 129, 64), (5, 300, 256)])
def test_group_mean_tails(G, R, C):
    from fusion_gcn_amd import _lib, ops
    if (G, R) == (2, 129):
        assert _lib.load().fgcn_group_mean_splits(2, 127) == 1 and _lib.load().fgcn_group_mean_splits(G, R) == 2
    x = rnd(G, R, C, seed=R + C) + 0.5
    got = ops.group_mean(put(x))
    assert tuple(got.shape) == (G, C)
    err = rel_l2(got.cpu().numpy(), x.double().mean(1).numpy())
    print(f"group_mean ({G}, {R}, {C}): {err:.2e}")
    assert err < RED_TOL
    assert torch.equal(got, ops.group_mean(put(x)))


@pytest.mark.parametrize("rows,ld,C,coff", [(777, 32, 30, 0), (777, 96, 32, 64), (130, 1028, 1028, 0), (1, 4, 1, 0)])
def test_col_sum_tails(rows, ld, C, coff):
    """a ragged channel count, a channel window of wider rows, and the wrapper's split above 1024 channels.  The channels outside the window
    hold NaN where the kernel's 16-byte loads do not have to touch them (whole four-channel groups outside [coff, coff + C))"""
    from fusion_gcn_amd import ops
    x = rnd(rows, ld, seed=rows + ld) + 0.25
    lo, hi = coff, (coff + C + 3) // 4 * 4
    x[:, :lo] = NAN
    x[:, hi:] = NAN
    got = ops.col_sum(put(x), C, coff)
    assert tuple(got.shape) == (C,)
    err = rel_l2(got.cpu().numpy(), x[:, coff:coff + C].double().sum(0).numpy())
    print(f"col_sum rows={rows} ld={ld} C={C} coff={coff}: {err:.2e}")
    assert err < RED_TOL


# ---- the elementwise reductions past the tile cap --------------------------------------------------------------------------------------------
def bn_vec(C, seed):
    """(4, C) BatchNorm vector as fgcn_bn_finalize lays it out: mean, rstd, scale = gamma * rstd, shift = beta - mean * scale"""
    mean, rstd = rnd(C, seed=seed) * 0.3, rnd(C, seed=seed + 1).abs() + 0.5
    gamma, beta = rnd(C, seed=seed + 2).abs() + 0.5, rnd(C, seed=seed + 3) * 0.3
    return torch.stack([mean, rstd, gamma * rstd, beta - mean * gamma * rstd])


@pytest.mark.parametrize("rows,C", [(65537, 4), (65537, 12), (65537, 64), (70001, 4), (70001, 12), (70001, 64), (200000, 4), (200000, 12)])
def test_elementwise_reductions_past_the_tile_cap(rows, C):
    """fgcn_elem_tiles gives 64 rows per tile up to 1024 tiles and ceil(rows / 1024) rows per tile beyond: col_sum_kernel, the bn_act
    backward reduce (gate from the sign image where rows * C is a multiple of 8, from the output tensor else; the three shortcut kinds; a
    full-size and a per-group gradient whose groups of 50 rows end inside the tiles) and fgcn_bn_bwd_reduce_ld then walk 65 .. 196 rows
    per tile where the other tests stop at 64.  At 70001 rows the tiles 1015 .. 1023 hold no row and must still write zero partials: the
    partial buffers are guarded allocations (NaN until written), so a tile that is skipped fails the comparison.  Against float64 sums."""
    from fusion_gcn_amd import _lib, ops
    lib = _lib.load()
    per_tile = -(-rows // 1024)
    assert lib.fgcn_elem_tiles(rows) == 1024 and per_tile > 64
    if rows == 70001:
        assert 1023 * per_tile > rows                       # trailing tiles without a row
    x = rnd(rows, C + 8, seed=rows + C) + 0.25
    xg = put(x)
    for name, got, want in (("all", ops.col_sum(xg, C + 8), x.double().sum(0)), ("window", ops.col_sum(xg, C, 4), x[:, 4:4 + C].double().sum(0))):
        err = rel_l2(got.cpu().numpy(), want.numpy())
        print(f"col_sum {name} rows={rows} C={C}: {err:.2e}")
        assert err < RED_TOL
    a, b, dout = rnd(rows, C, seed=rows + 1) * 1.7 + 0.3, rnd(rows, C, seed=rows + 2), rnd(rows, C, seed=rows + 3) + 0.25
    vec_a, vec_b = bn_vec(C, 900), bn_vec(C, 910)
    a_hat, b_hat = (a.double() - vec_a[0].double()) * vec_a[1].double(), (b.double() - vec_b[0].double()) * vec_b[1].double()
    ag, bg, dg, vag, vbg = put(a), put(b), put(dout), put(vec_a), put(vec_b)
    groups = [0] + ([50] if rows % 50 == 0 else [])         # (65537 and 70001 are primes: only 200000 rows divide into groups)
    assert groups == [0] or per_tile % 50                   # the groups end inside the tiles
    for res_mode in (0, 1, 2):
        rb, rvb = (bg if res_mode else None), (vbg if res_mode == 2 else None)
        out, mask = ops.bn_act(ag, vag, rb, rvb, relu=True, sign_mask=True)
        assert (mask is not None) == ((rows * C) % 8 == 0)
        gate = (out.cpu() > 0).double()
        for grp in groups:
            d = dout[:rows // grp] if grp else dout
            dp = (d.double().repeat_interleave(grp, dim=0) if grp else d.double()) * gate
            want = torch.stack([dp.sum(0), (dp * a_hat).sum(0), (dp * b_hat).sum(0)])[:3 if res_mode == 2 else 2]
            _, _, sums = ops.bn_act_bwd(put(d) if grp else dg, None if mask is not None else out, ag, vag, rb, rvb, res_mode=res_mode, relu=True,
                                        train=True, sign_mask=mask, grp_rows=grp)
            err = rel_l2(sums[:want.shape[0]].cpu().numpy(), want.numpy())
            print(f"bn_act_bwd_reduce rows={rows} C={C} res_mode={res_mode} grp_rows={grp}: {err:.2e}")
            assert err < RED_TOL, (res_mode, grp)
    wide = rnd(rows, C + 8, seed=rows + 4) + 0.25
    _, sums = ops.bn_bwd_window(put(wide), 4, ag, vag, train=True)
    dw = wide[:, 4:4 + C].double()
    err = rel_l2(sums[:2].cpu().numpy(), torch.stack([dw.sum(0), (dw * a_hat).sum(0)]).numpy())
    print(f"bn_bwd_reduce_ld rows={rows} C={C}: {err:.2e}")
    assert err < RED_TOL


@pytest.mark.parametrize("G,R,pool_splits,mean_splits", [(2, 4096, 64, 32), (512, 256, 2, 1)])
def test_pooling_row_splits(G, R, pool_splits, mean_splits):
    """ops.bn_act_pool / ops.group_mean with the largest split counts of their heuristics (64 and 32 workgroups per group: two long
    groups) and with many short groups (two splits and one), asserted through the exported split functions; against float64 means"""
    from fusion_gcn_amd import _lib, ops
    lib, C = _lib.load(), 16
    assert lib.fgcn_bn_act_pool_splits(G, R) == pool_splits and lib.fgcn_group_mean_splits(G, R) == mean_splits
    a, b, vec = rnd(G, R, C, seed=G + R) + 0.2, rnd(G, R, C, seed=G + R + 1), bn_vec(C, 920)
    want = torch.relu(a.double() * vec[2].double() + vec[3].double() + b.double())
    pooled, mask = ops.bn_act_pool(put(a), put(vec), put(b), None, G)
    e_pool = rel_l2(pooled.cpu().numpy(), want.mean(1).numpy())
    out, mask_ref = ops.bn_act(put(a), put(vec), put(b), None, relu=True, sign_mask=True)
    assert torch.equal(mask, mask_ref)
    e_mean = rel_l2(ops.group_mean(out).cpu().numpy(), want.mean(1).numpy())
    print(f"bn_act_pool ({G}, {R}): {e_pool:.2e}; group_mean: {e_mean:.2e}")
    assert e_pool < RED_TOL and e_mean < RED_TOL
