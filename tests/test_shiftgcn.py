"""Host-side checks of ``model: shiftgcn``: it resolves, its state dict is the stated one with the stated initial values, the float64
restatement tests/shiftgcn_ref.py agrees with itself (two writings of each shift operation), with autograd's numerical check and with the
right-derivative rule at integer positions, its salt rule finds an input for every GPU case, stock float32 torch stays within the flip cap
on the model input, and every fgcn_shift_* entry point refuses what it does not take before any launch."""
import ctypes as C

import pytest
import torch

import shiftgcn_ref as R
from oracle import filler

SHAPE, CLASSES = (2, 16, 25, 3), 7
BADARG, ALIGN = -1, -2


def _graph():
    from fusion_gcn_amd.datasets.ntu_rgb_d import constants as ntu
    from fusion_gcn_amd.util import Graph
    return Graph(ntu.skeleton_edges, center_joint=ntu.center_joint)


def _model(**kw):
    from fusion_gcn_amd.util.dynamic_import import import_model
    return import_model("shiftgcn")({"skeleton": SHAPE}, CLASSES, _graph(), **kw)


def test_import_model_resolves_shiftgcn():
    from fusion_gcn_amd.models.shiftgcn.shiftgcn import Model
    from fusion_gcn_amd.util.dynamic_import import import_model
    assert import_model("shiftgcn") is Model


def test_state_dict_keys_order_shapes_and_initial_values():
    torch.manual_seed(3)
    model = _model()
    sd = model.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == R.expected_keys(SHAPE, CLASSES)
    for i, (cin, cout, stride, residual) in enumerate(R.layer_plan(3, 64), start=1):
        g, t = f"l{i}.gcn1.", f"l{i}.tcn1."
        w = sd[g + "Linear_weight"]
        std = (1.0 / cout) ** 0.5
        assert w.numel() < 2000 or 0.9 * std < float(w.std()) < 1.1 * std, (g, float(w.std()), std)
        assert float(w.abs().max()) > 0 and float(sd[g + "Linear_bias"].abs().max()) == 0.0 and float(sd[g + "Feature_Mask"].abs().max()) == 0.0, g
        assert torch.all(sd[g + "bn.weight"] == 1e-6) and torch.all(sd[g + "bn.bias"] == 0), g
        assert (g + "down.0.weight" in sd) == (i in (1, 5, 8)) and (f"l{i}.residual.conv.weight" in sd) == (i in (5, 8))
        for key in ("shift_in.ypos", "shift_out.ypos"):
            p = sd[t + key]
            assert -1.0 <= float(p.min()) and float(p.max()) <= 1.0 and 0.4 < float(p.std()) < 0.75, (t + key, float(p.std()))     # uniform(-1, 1): 0.577
        assert torch.all(sd[t + "bn.weight"] == 1) and torch.all(sd[t + "bn2.weight"] == 1) and float(sd[t + "temporal_linear.bias"].abs().max()) == 0.0
    for k, v in sd.items():
        if v.dim() == 4:                             # a convolution: kaiming normal over its fan-out, zero bias
            assert float(sd[k[:-6] + "bias"].abs().max()) == 0.0, k
            std = (2.0 / v.shape[0]) ** 0.5
            assert v.numel() < 2000 or 0.85 * std < float(v.std()) < 1.15 * std, (k, float(v.std()), std)
    assert 0.8 * (2 / CLASSES) ** 0.5 < float(sd["fc.weight"].std()) < 1.2 * (2 / CLASSES) ** 0.5
    # the reference modules carry the same keys: a product state dict loads into them (what the GPU tests rely on)
    ref = R.RefModel(SHAPE, CLASSES)
    assert list(ref.state_dict()) == list(sd)
    ref.load_state_dict(sd)


def test_state_dict_round_trips():
    a = _model()
    R.fill(a, 1)
    b = _model()
    b.load_state_dict(a.state_dict())
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    sd = b.state_dict()                               # (the filler's values, not the initial ones)
    assert float(sd["l3.tcn1.shift_in.ypos"].abs().max()) > 1.0 and float(sd["l3.gcn1.Feature_Mask"].abs().max()) > 0.5


def test_model_takes_a_graph_of_up_to_64_joints_and_has_no_joint_by_joint_parameter():
    from fusion_gcn_amd.util.dynamic_import import import_model
    model = import_model("shiftgcn")({"skeleton": (1, 8, 64, 3)}, 5, None)
    assert model.l2.gcn1.bn.num_features == 64 * 64
    assert [tuple(v.shape) for k, v in model.state_dict().items()] == [s for _, s in R.expected_keys((1, 8, 64, 3), 5)]
    # (upstream's xpos and its two index tables are neither parameters nor buffers)
    assert {k.rsplit(".", 1)[-1] for k in model.state_dict()} == {"weight", "bias", "running_mean", "running_var", "num_batches_tracked", "Linear_weight",
                                                                   "Linear_bias", "Feature_Mask", "ypos"}


# ---- the two writings of each operation -----------------------------------------------------------------------------------------------------
def _agree(a, b, what):
    assert a.shape == b.shape, what
    a, b = a.detach(), b.detach()
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), what


@pytest.mark.parametrize("direction", (1, -1))
@pytest.mark.parametrize("dims", ((2, 3, 25, 64), (2, 2, 7, 16), (1, 3, 5, 3), (2, 2, 1, 8)), ids=R.tag_of)
def test_the_two_writings_of_the_joint_shift_agree(dims, direction):
    B, T, V, Cc = dims
    x0 = torch.from_numpy(filler.bellish("x.two.joint", dims)).double()
    m0 = torch.from_numpy(filler.uniform("mask.two.joint", (V, Cc), -1.5, 1.5)).double()
    probe = torch.from_numpy(filler.uniform("probe.two.joint", dims, -1, 1)).double()
    for gate in (False, True):
        x, m = x0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
        y_cl = R.joint_shift_cl(x, m if gate else None, direction)
        g_cl = torch.autograd.grad((y_cl * probe).sum(), [x, m] if gate else [x])
        y_nchw = R.joint_shift_nchw(x.permute(0, 3, 1, 2), m if gate else None, direction).permute(0, 2, 3, 1)
        g_nchw = torch.autograd.grad((y_nchw * probe).sum(), [x, m] if gate else [x])
        _agree(y_cl, y_nchw, "out")
        for a, b, k in zip(g_cl, g_nchw, ("dx", "dmask")):
            _agree(a, b, k)
            assert float(b.abs().max()) > 0, k
    # the formulas of the contract, element by element (a true modulo of a negative number)
    y = R.joint_shift_cl(x0, m0, direction)
    for v, c in ((0, 0), (3 % V, Cc - 1), (V - 1, Cc // 2)):
        want = x0[1 % B, 1 % T, (v + direction * c) % V, c] * (torch.tanh(m0[v, c]) + 1)
        assert float((y[1 % B, 1 % T, v, c] - want).abs()) < 1e-15


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("stride", (1, 2))
def test_the_two_writings_of_the_frame_shift_agree(stride, relu):
    B, T, V, Cc = 2, 7, 3, 24
    x0 = torch.from_numpy(filler.bellish("x.two.frame", (B, T, V, Cc))).double()
    pos0 = torch.from_numpy(filler.uniform("pos.two.frame", (Cc,), -2, 2)).double()
    pos0[:16] = torch.tensor([0.0, 1.0, -1.0, T - 1.0, 1.0 - T, T, -T, T + 0.5, -T - 0.5, 0.25, -0.25, -0.75, 1e-8, -1e-8, 1e9, -1e9], dtype=torch.float64)
    probe = torch.from_numpy(filler.uniform("probe.two.frame", (B, R.out_frames(T, stride), V, Cc), -1, 1)).double()
    x, pos = x0.clone().requires_grad_(True), pos0.clone().requires_grad_(True)
    y_cl = R.frame_shift_cl(x, pos, stride, relu)
    g_cl = torch.autograd.grad((y_cl * probe).sum(), [x, pos])
    y_nchw = R.frame_shift_nchw(x.permute(0, 3, 1, 2), pos, stride, relu).permute(0, 2, 3, 1)
    g_nchw = torch.autograd.grad((y_nchw * probe).sum(), [x, pos])
    _agree(y_cl, y_nchw, "out")
    for a, b, k in zip(g_cl, g_nchw, ("dx", "dpos")):
        _agree(a, b, k)
        assert float(b.abs().max()) > 0, k
    # positions beyond the clip: all-zero output and a zero gradient, not undefined behaviour
    assert float(y_cl[..., 14:16].abs().max()) == 0.0 and float(g_cl[1][14:16].abs().max()) == 0.0
    assert float(y_cl[..., 7:9].abs().max()) == 0.0                       # +-(T + 0.5): both taps outside
    # the gather form of dx stated in the contract, element by element
    dout = probe
    k = torch.floor(pos0).long()
    f = pos0 - k
    for (b, t, v, c) in ((0, 0, 0, 9), (1, 3, 2, 11), (1, T - 1, 1, 17), (0, 2, 1, 1), (1, 4, 0, 2)):
        want = 0.0
        for e, wgt in ((0, 1 - f[c]), (1, f[c])):
            n = t - int(k[c]) - e
            if n % stride == 0 and 0 <= n // stride < dout.shape[1]:
                want = want + wgt * dout[b, n // stride, v, c]
        if relu and not float(x0[b, t, v, c]) > 0:
            want = 0.0
        assert abs(float(g_cl[0][b, t, v, c]) - float(want)) < 1e-14, (b, t, v, c)


def test_a_nan_position_makes_its_channel_nan_and_no_other():
    x = torch.from_numpy(filler.bellish("x.nanpos", (2, 5, 3, 8))).double()
    pos = torch.tensor([0.3, float("nan"), -1.2, 0.0, 2.5, float("nan"), 1.0, -0.5], dtype=torch.float64)
    for y in (R.frame_shift_cl(x, pos), R.frame_shift_nchw(x.permute(0, 3, 1, 2), pos).permute(0, 2, 3, 1)):
        bad = torch.isnan(y)
        assert bool(bad[..., [1, 5]].all()) and not bool(bad[..., [0, 2, 3, 4, 6, 7]].any())


def test_both_operations_pass_gradcheck():
    """positions at least 1e-3 from an integer: the derivative with k held constant is then the derivative"""
    B, T, V, Cc = 2, 5, 4, 6
    x = torch.from_numpy(filler.bellish("x.gradcheck.shift", (B, T, V, Cc))).double().requires_grad_(True)
    mask = torch.from_numpy(filler.uniform("mask.gradcheck.shift", (V, Cc), -1, 1)).double().requires_grad_(True)
    pos = torch.from_numpy(filler.uniform("pos.gradcheck.shift", (Cc,), -2.5, 2.5)).double()
    near = (pos - torch.round(pos)).abs() < 1e-3
    pos = torch.where(near, pos + 0.01, pos).requires_grad_(True)
    assert float((pos - torch.round(pos)).abs().min()) >= 1e-3
    for direction in (1, -1):
        assert torch.autograd.gradcheck(lambda a, m: R.joint_shift_cl(a, m, direction), (x, mask), eps=1e-6, atol=1e-7, rtol=1e-5)
    for stride in (1, 2):
        # (no ReLU in the numerical check: its kink is KinkReLU's business; the filler's x is nowhere within 1e-6 of zero anyway)
        assert torch.autograd.gradcheck(lambda a, p: R.frame_shift_cl(a, p, stride, False), (x, pos), eps=1e-6, atol=1e-7, rtol=1e-5)
        assert float(x.detach().abs().min()) > 1e-5
        assert torch.autograd.gradcheck(lambda a, p: R.frame_shift_cl(a, p, stride, True), (x, pos), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_the_gradient_at_an_integer_position_is_the_right_derivative():
    B, T, V, Cc = 2, 6, 3, 5
    x = torch.from_numpy(filler.bellish("x.right", (B, T, V, Cc))).double()
    probe = torch.from_numpy(filler.uniform("probe.right", (B, T, V, Cc), -1, 1)).double()
    pos = torch.tensor([0.0, 1.0, -1.0, 2.0, -3.0], dtype=torch.float64, requires_grad=True)
    loss = lambda p: (R.frame_shift_cl(x, p) * probe).sum()  # noqa: E731
    g, = torch.autograd.grad(loss(pos), pos)
    h = 1e-6
    right = torch.stack([(loss(pos.detach() + h * torch.eye(Cc, dtype=torch.float64)[c]) - loss(pos.detach())) / h for c in range(Cc)])
    left = torch.stack([(loss(pos.detach()) - loss(pos.detach() - h * torch.eye(Cc, dtype=torch.float64)[c])) / h for c in range(Cc)])
    assert float((g - right).abs().max()) < 1e-8 * max(1.0, float(g.abs().max()))
    assert float((g - left).abs().min()) > 1e-3                        # (and the left derivative is another number, in every channel)


# ---- the salt rule finds an input for every GPU case ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", (1, -1))
@pytest.mark.parametrize("case", R.JOINT_CASES, ids=R.tag_of)
def test_a_salt_exists_for_every_joint_shift_case(case, direction):
    salt = R.joint_salt(case, direction)
    ref = R.joint_case(case, direction, "random")
    print(f"{case} dir {direction:+d}: salt {salt}, Feature_Mask terms cancel {ref['cond']:.1f}-fold")
    assert salt < R.MAX_SALT and ref["cond"] < R.COND_MAX and float(ref["dmask"].abs().max()) > 0
    if case[3] == 4:
        assert float(ref["out"][..., 3].abs().max()) == 0.0 and float(ref["dx"][..., 3].abs().max()) == 0.0


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("case", R.FRAME_CASES, ids=R.tag_of)
def test_a_salt_exists_for_every_frame_shift_case(case, relu):
    salt = R.frame_salt(case, relu)
    ref = R.frame_case(case, relu)
    print(f"{case} relu {relu}: salt {salt}, ypos terms cancel {ref['cond']:.1f}-fold")
    assert salt < R.MAX_SALT and ref["cond"] < R.COND_MAX
    assert float(ref["dpos"][14:16].abs().max()) == 0.0 and float(ref["out"][..., 14:16].abs().max()) == 0.0      # +-1e9


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=[c.name for c in R.BLOCK_CASES])
@pytest.mark.parametrize("kind", R.KINDS)
def test_a_salt_exists_for_every_unit_and_block_case(kind, case):
    salt = R.block_salt(kind, case)
    refs = [R.block_ref(kind, case, train) for train in (True, False)]
    print(f"{kind} {case.name}: salt {salt}, least |pre-activation| {min(r['least'] for r in refs):.1e}, terms cancel {max(r['cond'] for r in refs):.1f}-fold")
    assert salt < R.MAX_SALT
    for r in refs:
        assert r["least"] >= R.KINK_EPS and r["cond"] < R.COND_MAX
        zero = [k for k in r["grads"] if k.endswith(("Linear_bias", "down.0.bias", "residual.conv.bias"))]
        scale = max(float(g.abs().max()) for g in r["grads"].values())
    for k in zero:                                   # biases in front of a train-mode BatchNorm: a zero gradient
        assert float(refs[0]["grads"][k].abs().max()) <= 1e-9 * scale, k


def test_stock_float32_stays_within_the_flip_cap_on_the_model_input():
    """the cap the GPU run is asked to meet is met by the reference side alone: the same modules and values in float32 on the CPU take
    at most FLIP_CAP of the float64 reference's ReLU decisions differently"""
    ref = R.model_ref()
    lo = R.model_float32_decisions()
    assert len(lo) == len(ref["masks"]) == 30
    flips = sum(int((a != b).sum()) for a, b in zip(lo, ref["masks"]))
    print(f"{flips} of {ref['decisions']} ReLU decisions differ between float32 and float64 on the CPU; {ref['near']} pre-activations lie within KINK_EPS")
    assert ref["decisions"] > 1_000_000 and flips <= R.FLIP_CAP * ref["decisions"]
    forced = R.model_forced(lo)
    assert forced["flips"] == flips and forced["close"] < 10 * R.KINK_EPS, (forced["flips"], forced["close"])


# ---- the C entry points -------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_refuses_what_it_does_not_take():
    from fusion_gcn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16

    def joint(rows=6, V=25, Cc=64, ld=None, direction=1, src=0, ptrs=None):
        a = ptrs or [p, p, None, p, None]
        return lib.fgcn_shift_joint(*a, rows, V, Cc, Cc if ld is None else ld, direction, src, None)

    def frame(B=2, T=4, V=25, Cc=64, stride=1, ptrs=None):
        return lib.fgcn_shift_frame(*(ptrs or [p] * 4), B, T, V, Cc, stride, 1, None)

    def frame_bwd(B=2, T=4, V=25, Cc=64, stride=1, ptrs=None):
        return lib.fgcn_shift_frame_bwd(*(ptrs or [p] * 5), B, T, V, Cc, stride, 1, None)
    # each limit
    for kw in (dict(V=65), dict(V=0), dict(rows=0), dict(Cc=96), dict(Cc=576), dict(Cc=8), dict(Cc=3), dict(direction=0), dict(direction=2),
               dict(rows=(1 << 31) // (25 * 64)), dict(ld=32), dict(Cc=4, ld=2)):
        assert joint(**kw) == BADARG, kw
    assert joint(rows=(1 << 31) // (25 * 64) - 1, ptrs=[None, p, None, p, None]) == BADARG           # (the largest size passes the size check)
    assert b"null pointer" in lib.fgcn_last_error()
    for kw in (dict(V=65), dict(Cc=96), dict(Cc=576), dict(Cc=4), dict(stride=3), dict(stride=0), dict(T=0), dict(B=65536), dict(B=1 << 12, T=1 << 12, V=64, Cc=512)):
        assert frame(**kw) == BADARG and frame_bwd(**kw) == BADARG, kw
    assert b"31 bits" in lib.fgcn_last_error()
    # the mask-gradient terms come with x, the mask and the source gate together
    assert joint(src=1, ptrs=[p, p, p, p, None]) == BADARG and joint(src=1, ptrs=[p, p, None, p, p]) == BADARG
    assert joint(src=0, ptrs=[p, p, p, p, p]) == BADARG and joint(src=1, ptrs=[p, None, p, p, p]) == BADARG
    # null pointers, each in turn
    for i in (0, 3):
        ptrs = [p, p, None, p, None]
        ptrs[i] = None
        assert joint(ptrs=ptrs) == BADARG and b"null pointer" in lib.fgcn_last_error()
    for fn, n in ((frame, 4), (frame_bwd, 5)):
        for i in range(n):
            if fn is frame and i == 3:
                continue                              # (the partial sums are optional)
            ptrs = [p] * n
            ptrs[i] = None
            assert fn(ptrs=ptrs) == BADARG and b"null pointer" in lib.fgcn_last_error(), (fn.__name__, i)
    for i in range(3):
        ptrs = [p] * 3
        ptrs[i] = None
        assert lib.fgcn_shift_dmask(*ptrs, 25, 64, 64, 1, None) == BADARG and b"null pointer" in lib.fgcn_last_error()
    assert lib.fgcn_shift_dmask(p, p, p, 65, 64, 64, 1, None) == BADARG and lib.fgcn_shift_dmask(p, p, p, 25, 64, 64, 0, None) == BADARG
    assert lib.fgcn_shift_dmask(p, p, p, 25, 4, 5, 1, None) == BADARG
    # tensors read or written in 16-byte groups
    assert joint(ptrs=[p + 4, p, None, p, None]) == ALIGN and joint(ptrs=[p, p, None, p + 4, None]) == ALIGN
    assert joint(src=1, ptrs=[p, p, p, p, p + 8]) == ALIGN and b"aligned" in lib.fgcn_last_error()
    # the host geometry queries
    assert lib.fgcn_shift_joint_rows(0, 25, 64) == 0 and lib.fgcn_shift_joint_rows(6, 65, 64) == 0 and lib.fgcn_shift_joint_rows(6, 25, 96) == 0
    assert lib.fgcn_shift_joint_stage(65) == 0 and lib.fgcn_shift_joint_stage(0) == 0 and lib.fgcn_shift_joint_stage(64) == 2
    assert lib.fgcn_shift_frame_split(2, 4, 65, 64, 1) == 0 and lib.fgcn_shift_frame_split(2, 4, 25, 96, 1) == 0 and lib.fgcn_shift_frame_split(2, 4, 25, 64, 3) == 0
    for rows, V, Cc in ((1, 1, 64), (19, 40, 64), (8192, 25, 64), (8192, 25, 4), (2048, 64, 512), (100000, 25, 256)):
        rpw = lib.fgcn_shift_joint_rows(rows, V, Cc)
        assert 1 <= rpw <= rows and (rows + rpw - 1) // rpw <= 65535 and lib.fgcn_shift_joint_stage(V) * V <= 128, (rows, V, Cc, rpw)
    for B, T, V, Cc, s in ((1, 1, 25, 64, 1), (1, 21, 5, 64, 2), (128, 64, 25, 64, 1), (128, 16, 25, 256, 2), (1, 100000, 5, 64, 1)):
        fps = lib.fgcn_shift_frame_split(B, T, V, Cc, s)
        t_out = (T - 1) // s + 1
        assert 1 <= fps <= t_out and (t_out + fps - 1) // fps <= 65535, (B, T, V, Cc, s, fps)


def test_geometry_of_the_chunked_cases():
    """the GPU cases that are there for the multi-chunk and ragged paths reach them"""
    from fusion_gcn_amd import ops
    B, T, V, Cc = R.CHUNK_CASE
    chunks, rows, stage = ops.shift_geometry("joint", B, T, V, Cc)
    last = B * T - (chunks - 1) * rows
    assert chunks >= 3 and 0 < last < rows, (chunks, rows)                                   # three workgroup chunks, a ragged last one
    assert -(-rows // stage) >= 3 and rows % stage != 0, (rows, stage)                        # and a chunk is three LDS stages, the last one short
    for case in R.FRAME_SPLIT_CASES:
        B, T, V, Cc, s = case
        splits, fps, _ = ops.shift_geometry("frame", B, T, V, Cc, s)
        assert splits >= 3 and 0 < R.out_frames(T, s) - (splits - 1) * fps < fps, (case, splits, fps)
    with pytest.raises(Exception, match="no joint geometry"):
        ops.shift_geometry("joint", 2, 4, 65, 64)


def test_ops_fail_loudly_without_a_gpu():
    from fusion_gcn_amd import _lib, fops
    if torch.cuda.is_available():                     # (with a GPU the same calls are the GPU tests' business)
        return
    with pytest.raises(_lib.FgcnError):
        fops.joint_shift(torch.zeros(1, 2, 5, 64))
    with pytest.raises(_lib.FgcnError):
        fops.frame_shift(torch.zeros(1, 2, 5, 64), torch.zeros(64))
