#!/usr/bin/env python3
"""Writes tests/golden/bodies.npz from the REFERENCE's own body selection (util/preprocessing/skeleton.py:body_score and the three lines of
datasets/ntu_rgb_d/io.py:SkeletonSample._filter_bodies that use it: the scores of all bodies, ``argsort()[::-1]``, the first M), CPU only,
on a machine that has the reference checked out (``FGCN_REFERENCE``).  Nothing of the reference is copied: the file holds the inputs this
script draws and the arrays the reference's function returns for them.

For every case (DESIGN.md section 8o lists them):

    <case>_x          the float32 input clip (Mr, T, V, C)
    <case>_scores     np.array([body_score(b) for b in x]) on the float32 array, as the reference calls it (numpy's std() of a float32
                      array returns float32)
    <case>_order      scores.argsort()[::-1], all Mr indices
    <case>_sel        x[order[:M]]
    <case>_tied       1 where the case holds tied bodies (identical arrays or all-zero bodies): the test then compares the selected arrays
                      and not the indices

Asserted while writing: (a) the reference's ``sum() != 0`` and the contract's "any value non-zero" agree on every frame of every input;
(b) in the cases meant to be untied, neighbouring float64 scores differ by at least 1e-3 relative; (c) the reference's float32-path
scores are within 1e-5 relative of the float64 restatement (tests/bodies_ref.py); (d) in tie cases the tied bodies are identical arrays.
The (4, 300, 25, 3) clip of the GPU test is drawn there from a seed and is not stored; (b) and (c) are asserted for such clips here too.

The reference module imports tqdm at the top for its progress bars; no value needs it, so it is stubbed when it is not installed.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("FGCN_REFERENCE") or sys.exit("set FGCN_REFERENCE to the reference's checkout")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
import bodies_ref  # noqa: E402

try:
    import tqdm  # noqa: F401
except ImportError:
    _t = types.ModuleType("tqdm")
    _t.tqdm = lambda it, **kw: it
    sys.modules["tqdm"] = _t
_spec = importlib.util.spec_from_file_location("ref_skeleton", os.path.join(REF, "util", "preprocessing", "skeleton.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)

OFFSET, AMPLITUDES = 3.0, (0.02, 0.2)
LARGE = (4, 300, 25, 3)


class TooClose(Exception):
    pass


def draw(rng, shape):
    """every body offset + amplitude * uniform(0.5, 3), the amplitudes spread over AMPLITUDES and permuted"""
    amp = rng.permutation(np.geomspace(*AMPLITUDES, shape[0]))
    return (OFFSET + amp[:, None, None, None] * rng.uniform(0.5, 3.0, shape)).astype(np.float32)


def null(x, body, frames):
    x[body, list(frames)] = 0
    return x


def cases(rng):
    """-> [(name, x, M, tied)]"""
    out = []
    A, B, W = (4, 13, 7, 3), (3, 5, 4, 2), (16, 9, 5, 3)
    out.append(("c01_m1", draw(rng, A), 1, False))
    out.append(("c02_m2", draw(rng, A), 2, False))
    out.append(("c03_all", draw(rng, A), 4, False))
    out.append(("c04_body_null", null(draw(rng, A), 1, range(13)), 2, False))
    out.append(("c05_leading_null", null(null(draw(rng, A), 0, range(4)), 2, (0,)), 2, False))
    out.append(("c06_interior_null", null(null(draw(rng, A), 3, (5, 6, 9)), 1, (2,)), 2, False))
    out.append(("c07_one_frame", null(draw(rng, A), 2, [t for t in range(13) if t != 7]), 3, False))
    x = draw(rng, A)
    x[3] = x[0]
    out.append(("c08_identical", x, 2, True))
    x = draw(rng, A)
    out.append(("c09_one_actor", null(null(null(x, 0, range(13)), 1, range(13)), 3, range(13)), 2, True))
    out.append(("c10_2d_m1", null(draw(rng, B), 1, (3, 4)), 1, False))
    out.append(("c11_2d_all", draw(rng, B), 3, False))
    out.append(("c12_wide_m2", null(draw(rng, W), 5, (0, 8)), 2, False))
    out.append(("c13_wide_all", draw(rng, W), 16, False))
    return out


def run_reference(x, tied):
    for body in x:                                                                  # (a)
        for frame in body:
            assert (frame.sum() != 0) == bool(frame.any()), "a frame whose non-zero values cancel"
    scores = np.array([ref.body_score(b) for b in x])
    order = scores.argsort()[::-1]
    restated = bodies_ref.scores(x)
    assert np.all(np.abs(scores - restated) <= 1e-5 * restated), (scores, restated)                       # (c)
    ranked = restated[bodies_ref.order(restated)]
    if tied:                                                                        # (d)
        for i, j in zip(*np.nonzero(restated[:, None] == restated[None, :])):
            assert np.array_equal(x[i], x[j]), "tied bodies that are not identical arrays"
    elif np.any(ranked[:-1] - ranked[1:] < 1e-3 * ranked[:-1]):                      # (b)
        raise TooClose(f"neighbouring scores closer than 1e-3 relative: {ranked}")
    return scores, order


def record(seed):
    rng = np.random.default_rng(seed)
    out = {"seed": np.int64(seed)}
    for name, x, M, tied in cases(rng):
        assert x.dtype == np.float32
        scores, order = run_reference(x, tied)
        if not tied:
            assert np.array_equal(order, bodies_ref.order(bodies_ref.scores(x))), name
        assert np.array_equal(x[order[:M]], bodies_ref.select(x, M)), name
        out[f"{name}_x"], out[f"{name}_scores"], out[f"{name}_order"] = x, scores, order.astype(np.int64)
        out[f"{name}_sel"], out[f"{name}_tied"] = x[order[:M]], np.int64(tied)
        print(f"{name}: {x.shape} M={M} order {order.tolist()}")
    for _ in range(4):                                      # clips as the GPU test draws its large one: (b) and (c) hold for them too
        run_reference(null(draw(rng, LARGE), 1, range(250, 300)), False)
    return out


def main():
    for seed in range(20261020, 20261020 + 64):             # the first seed whose draws keep every untied pair of scores 1e-3 apart
        try:
            out = record(seed)
            break
        except TooClose as e:
            print(f"seed {seed}: {e}; next seed")
    else:
        raise SystemExit("no seed found")
    path = os.path.join(REPO, "tests", "golden", "bodies.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 200 << 10


if __name__ == "__main__":
    main()
