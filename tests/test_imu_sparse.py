"""The sparse aggregation route of the static-adjacency IMU graph convolution (``sparse=True``, ops.graph_spmm), host side: the CSR
builder, the C ABI surface, the unchanged state-dict surface of a ``sparse=True`` model and the path options.  GPU side:
tests/test_imu_sparse_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

from test_imu_gcn import CASES, GOLD, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STGCN = [t for t in CASES if CASES[t][3]["gc_model"] == "stgcn"]


def scatter(csr, shape):
    row_ptr, col, val = (t.cpu() for t in csr)
    a = torch.zeros(shape, dtype=torch.float32)
    for v in range(shape[0]):
        lo, hi = int(row_ptr[v]), int(row_ptr[v + 1])
        a[v, col[lo:hi].long()] = val[lo:hi]
    return a


def check_csr(adj):
    from fusion_gcn_amd import ops
    adj = adj.to(torch.float32)
    V = adj.shape[0]
    for tr, dense in ((False, adj), (True, adj.t().contiguous())):
        row_ptr, col, val = ops.csr_from_dense(adj, transpose=tr)
        assert row_ptr.dtype == torch.int32 and col.dtype == torch.int32 and val.dtype == torch.float32      # no field narrower than a dword
        assert row_ptr.shape == (V + 1,) and int(row_ptr[0]) == 0 and col.shape == val.shape == (int(row_ptr[-1]),)
        assert int(row_ptr[-1]) == int((dense != 0).sum()) and bool((val != 0).all())                          # explicit zeros dropped
        assert torch.equal(scatter((row_ptr, col, val), dense.shape), dense)                                   # bit for bit
        for v in range(V):
            c = col[int(row_ptr[v]):int(row_ptr[v + 1])]
            assert bool((c[1:] > c[:-1]).all()) and (c.numel() == 0 or (0 <= int(c[0]) and int(c[-1]) < dense.shape[1]))
        if tr:                                           # the transposed form IS the form of adj.T
            for got, want in zip((row_ptr, col, val), ops.csr_from_dense(adj.t().contiguous())):
                assert torch.equal(got, want)
        # the padding fgcn_graph_spmm asks for: readable entries behind the views
        assert ops._csr_padded(col) and ops._csr_padded(val)
    return ops.csr_from_dense(adj)


@pytest.mark.parametrize("name", ["adj.row_t1", "adj.column_t2_inter", "adj.symmetric_sensor"])
def test_csr_of_the_golden_adjacencies(name):
    check_csr(torch.from_numpy(GOLD[name]).float())


def test_csr_of_the_config_graph():
    from fusion_gcn_amd.models.mmargcn.imu_feature_models import build_imu_graph_adjacency
    adj = build_imu_graph_adjacency((326, 6), 0, "stgcn", False, "column", 1, False)
    assert adj.shape == (1956, 1956)
    row_ptr, _, _ = check_csr(adj)
    per_row = (row_ptr[1:] - row_ptr[:-1]).tolist()
    assert per_row[:6] == [7] * 6 and per_row[-6:] == [7] * 6 and per_row[6:-6] == [8] * 1944
    assert build_imu_graph_adjacency((326, 6), 0, "stgcn", True, "column", 1, False).layout == torch.strided    # sparse=True: still dense
    dense2 = build_imu_graph_adjacency((326, 6), 0, "stgcn", False, "column", 2, True)
    assert int((dense2 != 0).sum(1).max()) == 30


def test_csr_with_empty_rows_and_of_an_all_zero_matrix():
    g = torch.Generator().manual_seed(3)
    a = torch.randn(37, 37, generator=g) * (torch.rand(37, 37, generator=g) < 0.1)
    a[[0, 5, 36]] = 0
    a[:, 7] = 0
    check_csr(a)
    row_ptr, col, val = check_csr(torch.zeros(9, 9))
    assert int(row_ptr.abs().sum()) == 0 and col.numel() == 0 and val.numel() == 0


def test_entry_point_is_declared_and_bound():
    from fusion_gcn_amd import _lib
    header = open(os.path.join(ROOT, "include", "fgcn.h")).read()
    assert re.search(r"\bint\s+fgcn_graph_spmm\s*\(", header)
    res, args = _lib.SIGNATURES["fgcn_graph_spmm"]
    decl = re.search(r"int\s+fgcn_graph_spmm\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(args) == len(decl.split(","))


@pytest.mark.parametrize("tag", STGCN)
def test_sparse_model_has_the_dense_state_dict_surface(tag):
    from fusion_gcn_amd.models.mmargcn.graph_convolution import STGCNGraphConvolution
    shape, classes, _, kw = CASES[tag]
    model, sd = build(tag, shape, classes, dict(kw, sparse=True), double=True)
    assert sorted(sd) == list(GOLD[f"{tag}.keys"])
    dense, _ = build(tag, double=True)
    assert list(model.state_dict()) == list(dense.state_dict())                                    # same keys in the same order
    adj = sd["gcn.gc1.adj"]
    assert adj.layout == torch.strided and np.abs(adj.numpy() - GOLD[f"{tag}.adj"]).max() < 1e-7
    layers = [m for m in model.modules() if isinstance(m, STGCNGraphConvolution)]
    assert layers and all(m.sparse and m.takes_sparse_route() for m in layers)
    assert not any(m.sparse for m in dense.modules() if isinstance(m, STGCNGraphConvolution))
    dense.load_state_dict(model.state_dict())                                                       # a checkpoint moves between the routes


def test_path_options_parse_graph_spmm_auto():
    from fusion_gcn_amd.paths import PathOptions
    assert PathOptions().graph_spmm_auto is False
    po = PathOptions().update_from("graph_spmm_auto=1,graph_spmm_auto_density_ppm=20000")
    assert po.graph_spmm_auto is True and po.graph_spmm_auto_density_ppm == 20000
    assert po.copy().graph_spmm_auto is True


def test_graph_spmm_rejects_bad_arguments_on_the_host():
    """Validation precedes the launch: no GPU needed (as tests/test_abi.py::test_host_side_validation)."""
    import ctypes as C
    from fusion_gcn_amd import _lib, build as B
    B.build()
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p16 = (C.addressof(buf) + 15) // 16 * 16

    def call(inp=p16, row_ptr=p16, col=p16, val=p16, b=None, vec_b=None, out=p16, mask=None, B_=1, V=2, C_=8, ld_in=8, ld_b=8, ld_out=8,
             res_mode=0, relu=0):
        return lib.fgcn_graph_spmm(inp, row_ptr, col, val, b, vec_b, out, mask, B_, V, C_, ld_in, ld_b, ld_out, res_mode, relu, None)
    assert call(C_=6, ld_in=6, ld_out=6) == -1 and b"multiple of 4" in lib.fgcn_last_error()
    for name in ("row_ptr", "col", "val"):
        assert call(**{name: None}) == -1 and b"null CSR array" in lib.fgcn_last_error()
    assert call(inp=None) == -1 and call(out=None) == -1
    assert call(B_=1 << 15, V=1 << 15) == -1 and b"32-bit row math" in lib.fgcn_last_error()               # B * V rows
    assert call(B_=1, V=1 << 20, C_=8, ld_in=1 << 12) == -1 and b"32-bit byte offsets" in lib.fgcn_last_error()   # a row stride
    assert call(ld_in=4) == -1 and call(ld_out=4) == -1                                                     # strides that do not cover C
    assert call(res_mode=1) == -1 and call(res_mode=2, b=p16) == -1 and call(res_mode=3) == -1              # residual operands missing
    assert call(C_=4, ld_in=4, ld_out=4, mask=p16) == -1 and b"sign mask" in lib.fgcn_last_error()
    assert call(inp=p16 + 4) == -2                                                                           # alignment


def test_graph_spmm_argument_checks_under_sanitizers():
    """The new entry point's host code in the AddressSanitizer + UBSan build of the library (build.build_host_asan), as
    tests/test_abi.py::test_host_code_under_sanitizers drives the older entry points."""
    import subprocess
    import sys
    from fusion_gcn_amd import build as B
    asan_lib = B.build_host_asan()
    env = dict(os.environ, FGCN_LIB=asan_lib, LD_PRELOAD=B.asan_runtime(), ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_graph_spmm_rejects_bad_arguments_on_the_host"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    text = r.stdout + r.stderr
    assert r.returncode == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert "1 passed" in text
