"""Forced row splits of the weight-gradient kernels (a helper module: no test, no conftest), shared by tests/test_kernels_gpu.py and
tests/test_bf16_gpu.py.

ops.tconv_wgrad and the 1x1 form of ops.rows_wgrad (fgcn_tconv_wgrad / fgcn_pw_wgrad, twgrad_launch in fgcn_twgrad.hip) cut the stages of a
launch -- blocks of rows, never spanning two samples -- into ``nsplit`` consecutive shares, one per workgroup and tile.  At the kernel tests'
shapes the library's own count gives every workgroup one or two stages; forced to 1, 2 or 3 a workgroup walks several: the prefetch of the
next stage, the refill of the tap window at the first stage of a sample inside a share, its extension from stage to stage."""
WGRAD_SPLIT_SHAPES = [(3, 20, 25, 64, 64, 9, 1), (2, 21, 25, 64, 128, 9, 2), (2, 13, 18, 128, 256, 9, 1), (3, 10, 18, 128, 96, 1, 1),
                      (2, 20, 27, 128, 128, 5, 1)]           # (B, T, V, K, N, taps, stride)


def wgrad_shares(lib, mode, pointwise, B, rows, N, nsplit):
    """-> (stages per sample, [(first, end) stage of every workgroup's share]), restated from twgrad_launch: a stage is 64 rows per slab
    part in math mode f32 and 32 in the split-bf16 modes (bf16, bf16x3, f16x2).  The parts come from the exported slab count, so the wave
    arrangement the library picks is followed; the two constants are this copy's.  ``rows``: rows of one sample (output frames x joints)."""
    parts = (lib.fgcn_pw_wgrad_slabs if pointwise else lib.fgcn_tconv_wgrad_slabs)(N, 1)
    stage_rows = (64 if mode == "f32" else 32) * parts
    per_sample = -(-rows // stage_rows)
    total = B * per_sample
    per = -(-total // nsplit)
    return per_sample, [(i * per, min((i + 1) * per, total)) for i in range(nsplit) if i * per < total]


def assert_shares_iterate(lib, mode, pointwise, B, rows, N):
    """What the forced splits are for: every workgroup's stage loop runs at least 3 times at 1 and 2 splits; at 3 splits all but the last
    share do (the last one of the 64-row-stage forms is 2 stages at two of the shapes); and at 2 or 3 splits a share begins in the middle
    of a sample and crosses into the next."""
    crossing = False
    for nsplit in (1, 2, 3):
        per_sample, shares = wgrad_shares(lib, mode, pointwise, B, rows, N, nsplit)
        assert len(shares) == nsplit and min(e - b for b, e in shares[:-1] or shares) >= 3, (nsplit, shares)
        assert shares[-1][1] - shares[-1][0] >= (3 if nsplit < 3 else 2), (nsplit, shares)
        crossing |= any(b % per_sample and (e - 1) // per_sample > b // per_sample for b, e in shares)
    assert crossing, (mode, pointwise, B, rows, N)


def force_row_splits(m, lib, ops, nsplit, tiles_t, tiles_p, seen):
    """``ops`` takes its row-split count from the resident-workgroup limits (all-taps form: ``tiles_t`` tiles per split; 1x1 form:
    ``tiles_p``) and from ``_pick_nsplit`` (per-tap kernel): set them through the monkeypatch context ``m`` so that ``nsplit`` comes out,
    and record in ``seen`` what reaches the slab-count functions."""
    real_t, real_p = lib.fgcn_tconv_wgrad_slabs, lib.fgcn_pw_wgrad_slabs
    m.setattr(lib, "fgcn_tconv_wgrad_resident", lambda N: nsplit * tiles_t)
    m.setattr(lib, "fgcn_pw_wgrad_resident", lambda N: nsplit * tiles_p)
    m.setattr(lib, "fgcn_tconv_wgrad_slabs", lambda N, n: (seen.append(("taps", n)), real_t(N, n))[1])
    m.setattr(lib, "fgcn_pw_wgrad_slabs", lambda N, n: (seen.append(("1x1", n)), real_p(N, n))[1])
    m.setattr(ops, "_pick_nsplit", lambda M, K, N, taps: (seen.append(("rows", nsplit)), nsplit)[1])
