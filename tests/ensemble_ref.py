"""Numpy restatement of the score fusion (include/fgcn.h, fgcn_score_fuse / fgcn_fuse_sweep), written from the header -- a helper module:
no test.  The fused value is the float64 loop of the header, rounded once to float32; the ranking rules are fgcn_classify_update's."""
import numpy as np

NONE, SOFTMAX = "none", "softmax"


def gt(a, b):
    """torch's order of floats: NaN above every number"""
    return (a > b) | (np.isnan(a) & ~np.isnan(b))


def eq(a, b):
    """... and equal to NaN"""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def transform(z, mode):
    """t_s of one stream: float32 (rows, classes)"""
    z = np.asarray(z, np.float32)
    if mode == NONE:
        return z
    assert mode == SOFTMAX
    with np.errstate(all="ignore"):
        z64 = z.astype(np.float64)
        m = np.fmax.reduce(z64, axis=1, keepdims=True, initial=-np.inf)         # NaN skipped; -inf for a row of NaN
        e = np.exp(z64 - m)
        return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def fuse(scores, weights, mode=NONE):
    """fused float32 (rows, classes): acc = +0.0; acc += float64(float32(w_s)) * float64(t_s) in stream order; one rounding"""
    w = np.asarray(weights, np.float64).astype(np.float32)
    assert len(scores) == w.shape[0]
    acc = np.zeros(np.asarray(scores[0]).shape, np.float64)
    with np.errstate(all="ignore"):
        for z, ws in zip(scores, w):
            acc = acc + np.float64(ws) * transform(z, mode).astype(np.float64)
        return acc.astype(np.float32)


def spacing_bound(scores, weights, mode):
    """the elementwise bound of the header for positive weights: sum_s |w_s| spacing(t_s) + spacing(fused)"""
    w = np.asarray(weights, np.float64).astype(np.float32).astype(np.float64)
    bound = np.spacing(np.abs(fuse(scores, weights, mode))).astype(np.float64)
    for z, ws in zip(scores, w):
        bound = bound + abs(ws) * np.spacing(np.abs(transform(z, mode))).astype(np.float64)
    return bound


def classify(fused, labels, k):
    """-> dict of examples, ignored, invalid, top1, topk (ints) and pred (int array, -1 for a row that is not an example)"""
    fused, labels = np.asarray(fused, np.float32), np.asarray(labels, np.int64)
    rows, classes = fused.shape
    valid = (labels >= 0) & (labels < classes)
    yi = np.where(valid, labels, 0)
    fy = fused[np.arange(rows), yi][:, None]
    col = np.arange(classes)[None, :]
    above = (gt(fused, fy) | ((col < yi[:, None]) & eq(fused, fy))).sum(axis=1)
    nan = np.isnan(fused)
    pred = np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, fused).argmax(axis=1))      # the FIRST index of the maximum
    top1 = valid & (above == 0)
    assert np.array_equal(top1, valid & (pred == yi))                  # the header: rank 0 is the same thing as pred == y
    return {"examples": int(valid.sum()), "ignored": int((labels == -100).sum()), "invalid": int((~valid & (labels != -100)).sum()),
            "top1": int(top1.sum()), "topk": int((valid & (above < k)).sum()), "pred": np.where(valid, pred, -1)}


def sweep(scores, candidates, labels, k, mode=NONE):
    """-> (header int64 (3,): examples, ignored, invalid; hits int64 (G, 2): top-1 and top-k per candidate)"""
    candidates = np.asarray(candidates)
    hits = np.zeros((candidates.shape[0], 2), np.int64)
    header = None
    for g, w in enumerate(candidates):
        c = classify(fuse(scores, w, mode), labels, k)
        hits[g] = c["top1"], c["topk"]
        header = np.asarray([c["examples"], c["ignored"], c["invalid"]], np.int64)
    return header, hits


def best(hits):
    """most top-1 hits, then most top-k hits, then the lowest row"""
    rows = sorted(range(len(hits)), key=lambda g: (-int(hits[g][0]), -int(hits[g][1]), g))
    return rows[0]
