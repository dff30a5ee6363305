"""Host-side references shared by tests/test_dropout.py and tests/test_dropout_gpu.py (no test in here).

* Philox4x32-10 in numpy, written from the paper's round function and independent of csrc/fgcn_rng.hpp, and the keep rule of
  include/fgcn.h on top of it: what fgcn_dropout_fwd must reproduce bit for bit.
* float64 restatements of the two layers that apply dropout -- the IMU graph convolution ``relu(mask s (conv(x) adj^T) + res)`` and the
  MS-G3D MLP layer ``act(BN(conv(mask s x)))`` -- as functions of a GIVEN kept-bit image, with their inputs and parameters.
"""
import numpy as np
import torch

M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) that broadcast, key: two ints -> (..., 4) uint32."""
    c = [np.asarray(v, dtype=np.uint64) for v in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    m0, m1, lo = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(M32)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                                   # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, -1).astype(np.uint32)


def threshold(p):
    return int(float(np.float32(p)) * 4294967296.0)


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep(n, p, seed, site, step):
    """(n,) bool: element i is kept iff word i & 3 of philox({i >> 2, site, lo32(step), hi32(step)}, {lo32(seed), hi32(seed)}) >= thr"""
    assert n % 4 == 0
    g = np.arange(n // 4, dtype=np.uint64)
    words = philox4x32_10((g, site & M32, step & M32, (step >> 32) & M32), (seed & M32, (seed >> 32) & M32))
    return words.reshape(-1) >= np.uint32(threshold(p))


def pack(bits):
    """bit i & 7 of byte i >> 3, unused tail bits zero"""
    return np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little")


def unpack(image, n):
    return np.unpackbits(np.asarray(image, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---- the IMU graph convolution -------------------------------------------------------------------------------------------------------
B, V = 2, 12
GC_CASES = {"none": (1, 8, False), "identity": (8, 8, True), "conv": (8, 16, True)}        # res_kind: (in, out, residual)
GC_P, GC_SEED = 0.5, 20261


def ring_adjacency(v=V):
    """self loops + both ring neighbours + one chord, row-normalised: 3-4 non-zeros per row (the sparse route has something to skip)"""
    a = np.eye(v)
    for i in range(v):
        a[i, (i + 1) % v] = a[i, (i - 1) % v] = 1.0
    a[0, v // 2] = a[v // 2, 0] = 1.0
    return torch.from_numpy(a / a.sum(1, keepdims=True)).double()


def gc_case(kind):
    """-> dict(x (B, V, Fin), probe (B, V, O), params {state-dict key: float64 tensor}) of a layer case, deterministic"""
    fin, o, _ = GC_CASES[kind]
    s = 100 * (1 + list(GC_CASES).index(kind))
    params = {"conv.weight": rnd(o, fin, 1, seed=s + 1) * 0.7, "conv.bias": rnd(o, seed=s + 2) * 0.3}
    if kind == "conv":
        params.update({"residual.0.weight": rnd(o, fin, 1, seed=s + 3) * 0.7, "residual.0.bias": rnd(o, seed=s + 4) * 0.3,
                       "residual.1.weight": 1.0 + 0.3 * rnd(o, seed=s + 5), "residual.1.bias": 0.3 * rnd(o, seed=s + 6)})
    return {"x": rnd(B, V, fin, seed=s + 7), "probe": rnd(B, V, o, seed=s + 8), "params": params}


def gc_forward(kind, x, params, adj, kept, p, eps=1e-5):
    """float64 layer in train mode -> (out, pre-ReLU values); kept: (B, V, O) bool in the node-major order of the layer's mask"""
    w = params["conv.weight"][:, :, 0]
    support = x @ w.t() + params["conv.bias"]                                  # (B, V, O)
    main = torch.einsum("vu,buo->bvo", adj, support)                           # (conv(x) . adj^T), node-major
    main = main * torch.from_numpy(np.asarray(kept)).double() * float(scale(p))
    if kind == "identity":
        main = main + x
    elif kind == "conv":
        r = x @ params["residual.0.weight"][:, :, 0].t() + params["residual.0.bias"]
        mean, var = r.mean((0, 1)), r.var((0, 1), unbiased=False)
        main = main + (r - mean) / torch.sqrt(var + eps) * params["residual.1.weight"] + params["residual.1.bias"]
    return torch.relu(main), main


def gc_reference(kind, kept, p=GC_P):
    """-> dict(out, pre, gx, grads {key: tensor}) for loss = sum(out * probe)"""
    case = gc_case(kind)
    x = case["x"].clone().requires_grad_(True)
    params = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    out, pre = gc_forward(kind, x, params, ring_adjacency(), kept, p)
    grads = torch.autograd.grad((out * case["probe"]).sum(), [x] + list(params.values()))
    return {"out": out.detach(), "pre": pre.detach(), "gx": grads[0], "grads": dict(zip(params, grads[1:]))}


def off_the_kink(pre, kept=None):
    """smallest |pre-ReLU value|; with ``kept``: over the kept elements only -- a dropped element of a layer WITHOUT residual is exactly
    zero in the reference and in the kernel alike, its output is 0 and its gradient 0 on either side of the kink"""
    a = pre.abs()
    if kept is not None:
        a = a[torch.from_numpy(np.asarray(kept))]
    return float(a.min())


# ---- the MS-G3D MLP layer ------------------------------------------------------------------------------------------------------------
MLP_SHAPE, MLP_OUT, MLP_P, MLP_SEED = (2, 4, 5, 16), 32, 0.25, 20262


def mlp_case():
    c = MLP_SHAPE[-1]
    return {"x": rnd(*MLP_SHAPE, seed=11), "probe": rnd(*MLP_SHAPE[:-1], MLP_OUT, seed=12),
            "params": {"weight": rnd(MLP_OUT, c, 1, 1, seed=13) * 0.4, "bias": rnd(MLP_OUT, seed=14) * 0.3,
                       "gamma": 1.0 + 0.3 * rnd(MLP_OUT, seed=15), "beta": 0.3 * rnd(MLP_OUT, seed=16)}}


def mlp_forward(x, params, kept, p, eps=1e-5):
    """float64 [Dropout, Conv2d 1x1, BatchNorm2d (batch statistics), ReLU] on channels-last x; kept: x's shape -> (out, pre-ReLU)"""
    xd = x * torch.from_numpy(np.asarray(kept)).double() * float(scale(p))
    y = xd @ params["weight"].reshape(params["weight"].shape[0], -1).t() + params["bias"]
    flat = y.reshape(-1, y.shape[-1])
    pre = (y - flat.mean(0)) / torch.sqrt(flat.var(0, unbiased=False) + eps) * params["gamma"] + params["beta"]
    return torch.relu(pre), pre


def mlp_reference(kept, p=MLP_P):
    case = mlp_case()
    x = case["x"].clone().requires_grad_(True)
    params = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    out, pre = mlp_forward(x, params, kept, p)
    grads = torch.autograd.grad((out * case["probe"]).sum(), [x] + list(params.values()))
    return {"out": out.detach(), "pre": pre.detach(), "gx": grads[0], "grads": dict(zip(params, grads[1:]))}


# ---- MultiScale_GraphConv(dropout=): aggregate over the k-hop stack, Dropout, scale-major 1x1 conv, BatchNorm, ReLU -----------------
GCN_SHAPE, GCN_SCALES, GCN_OUT, GCN_P, GCN_SEED = (2, 4, 6, 3), 2, 8, 0.25, 20263        # (B, T, V, C): 3 channels travel as 4


def chain_graph(v=GCN_SHAPE[2]):
    a = np.zeros((v, v))
    a[np.arange(v - 1), np.arange(1, v)] = a[np.arange(1, v), np.arange(v - 1)] = 1.0
    return a


def msgcn_case():
    b, t, v, c = GCN_SHAPE
    return {"x": rnd(b, t, v, c, seed=21), "probe": rnd(b, t, v, GCN_OUT, seed=22),
            "params": {"A_res": 0.05 * rnd(GCN_SCALES * v, v, seed=23), "weight": rnd(GCN_OUT, GCN_SCALES * c, 1, 1, seed=24) * 0.5,
                       "bias": rnd(GCN_OUT, seed=25) * 0.3, "gamma": 1.0 + 0.3 * rnd(GCN_OUT, seed=26), "beta": 0.3 * rnd(GCN_OUT, seed=27)}}


def msgcn_forward(x, params, a_powers, kept, p, eps=1e-5):
    """x (B, T, V, 3); a_powers (S*V, V) the module's constant stack; kept (B, T, V, S*4): the image of the aggregate as the module lays
    it out, channel s*4 + c with c == 3 a zero pad channel -> (out, pre-ReLU, dropped aggregate (B, T, V, S*4))"""
    b, t, v, c = x.shape
    s_ = GCN_SCALES
    a = (a_powers + params["A_res"]).view(s_, v, v)
    agg = torch.einsum("svu,btuc->btvsc", a, torch.nn.functional.pad(x, (0, 1)))                  # (B, T, V, S, 4)
    dropped = agg * torch.from_numpy(np.asarray(kept)).double().view(b, t, v, s_, c + 1) * float(scale(p))
    y = dropped[..., :c].reshape(b, t, v, s_ * c) @ params["weight"].reshape(GCN_OUT, -1).t() + params["bias"]
    flat = y.reshape(-1, GCN_OUT)
    pre = (y - flat.mean(0)) / torch.sqrt(flat.var(0, unbiased=False) + eps) * params["gamma"] + params["beta"]
    return torch.relu(pre), pre, dropped.reshape(b, t, v, s_ * (c + 1))


def msgcn_reference(a_powers, kept, p=GCN_P):
    case = msgcn_case()
    x = case["x"].clone().requires_grad_(True)
    params = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
    out, pre, dropped = msgcn_forward(x, params, a_powers, kept, p)
    grads = torch.autograd.grad((out * case["probe"]).sum(), [x] + list(params.values()))
    return {"out": out.detach(), "pre": pre.detach(), "dropped": dropped.detach(), "gx": grads[0], "grads": dict(zip(params, grads[1:]))}
