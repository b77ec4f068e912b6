"""CPU restatement of lbvh_k_closest_points (include/lbvh.h): numpy float32, brute force over every (query, triangle) pair — no tree.
A helper module, not a test file.  Distances, boxes, activity, R and the candidate predicate are point_reference's, unchanged.

    reference(queries, a, b, c, box_lo, box_hi, k) -> Result(records, found, rejected, candidates)
        records     (len(queries), k) CLOSEST_POINT: per query the candidates by a STABLE sort on dist2 over the triangles in index
                    order (ties fall to the lower index), the first k of them, padded with point_reference.NONE
        found       uint32, min(k, number of candidates)
        rejected    the number of (active query, triangle) pairs with dist2 < R that the box rule turned down
        candidates  the number of candidates of each query, not capped at k
    truncate(result, k) -> the Result for a smaller k (the first k columns: the order does not depend on k)"""
from collections import namedtuple

import numpy as np

import point_reference as R

Result = namedtuple("Result", "records found rejected candidates")


def reference(queries, a, b, c, box_lo, box_hi, k, pairs_per_chunk=1 << 22):
    f = np.float32
    a, b, c = (np.ascontiguousarray(x, dtype=f) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=f), np.ascontiguousarray(box_hi, dtype=f)
    e1, e2 = b - a, c - a
    n, t = len(queries), len(a)
    records = np.empty((n, k), dtype=R.CLOSEST_POINT)
    records[:] = R.NONE
    candidates = np.zeros(n, dtype=np.int64)
    rejected = 0
    act = R.active(queries)
    big = R.radius2(queries)
    step = max(1, pairs_per_chunk // max(t, 1))
    m = min(k, t)
    for s in range(0, n, step):
        sel = np.nonzero(act[s:s + step])[0] + s
        if len(sel) == 0:
            continue
        p = queries["p"][sel][:, None, :]
        d, u, v = R.point_triangle(p, a[None], e1[None], e2[None])
        own = R.box_dist2(p, box_lo[None], box_hi[None])
        with np.errstate(invalid="ignore"):
            inside = d < big[sel][:, None]                     # False for NaN
            front = d < own
        rejected += int((inside & front).sum())
        cand = inside & ~front
        candidates[sel] = cand.sum(axis=1)
        key = np.where(cand, d, f(np.inf))                     # a candidate's dist2 is < R <= MAX_FLOAT: never inf
        order = np.argsort(key, axis=1, kind="stable")[:, :m]  # equal dist2: the lower index first
        rows = np.arange(len(sel))[:, None]
        has = cand[rows, order]
        block = np.empty((len(sel), m), dtype=R.CLOSEST_POINT)
        block[:] = R.NONE
        block["dist2"] = np.where(has, d[rows, order], R.NONE["dist2"])
        block["tri"] = np.where(has, order, 0)
        block["u"] = np.where(has, u[rows, order], f(0))
        block["v"] = np.where(has, v[rows, order], f(0))
        records[sel, :m] = block
    found = np.minimum(candidates, k).astype(np.uint32)
    return Result(records, found, rejected, candidates)


def truncate(result, k):
    assert k <= result.records.shape[1]
    return Result(np.ascontiguousarray(result.records[:, :k]), np.minimum(result.candidates, k).astype(np.uint32), result.rejected,
                  result.candidates)
