"""CPU restatement of lbvh_trace_k_closest (include/lbvh.h): numpy float32, brute force over every (ray, triangle) pair — no tree.
A helper module, not a test file.  The slab test, Moeller-Trumbore, activity, T and the candidate mask are ray_reference's, unchanged.

    reference(rays, a, b, c, box_lo, box_hi, k) -> Result(records, found, candidates)
        records     (len(rays), k) HIT: per ray the candidates by a STABLE sort on t over the triangles in index order (ties — -0
                    and +0 included, they compare equal — fall to the lower index), the first k of them, padded with
                    ray_reference.MISS
        found       uint32, min(k, number of candidates)
        candidates  the number of candidates of each ray, not capped at k (lbvh_count_hits' count)
    truncate(result, k) -> the Result for a smaller k (the first k columns: the order does not depend on k)"""
from collections import namedtuple

import numpy as np

import ray_reference as R

Result = namedtuple("Result", "records found candidates")


def reference(rays, a, b, c, box_lo, box_hi, k, pairs_per_chunk=1 << 22):
    f = np.float32
    assert rays.dtype == R.RAY
    a, b, c = (np.ascontiguousarray(x, dtype=f) for x in (a, b, c))
    lo, hi = np.ascontiguousarray(box_lo, dtype=f), np.ascontiguousarray(box_hi, dtype=f)
    e1, e2 = b - a, c - a
    n, t_count = len(rays), len(a)
    records = np.empty((n, k), dtype=R.HIT)
    records[:] = R.MISS
    candidates = np.zeros(n, dtype=np.int64)
    act = R.active(rays)
    with np.errstate(all="ignore"):
        inv_all = f(1) / rays["dir"].astype(f)
        big = np.minimum(rays["t_max"], R.MAX_FLOAT)
    step = max(1, pairs_per_chunk // max(t_count, 1))
    m = min(k, t_count)
    for s in range(0, n, step):
        sel = np.nonzero(act[s:s + step])[0] + s
        if len(sel) == 0:
            continue
        o = rays["origin"][sel][:, None, :]
        d = rays["dir"][sel][:, None, :]
        passes, entry = R.box_entry(o, inv_all[sel][:, None, :], lo[None], hi[None])
        t, u, v = R.ray_triangle(o, d, a[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = passes & ~(t < entry) & (t > rays["t_min"][sel][:, None]) & (t < big[sel][:, None])
        candidates[sel] = cand.sum(axis=1)
        key = np.where(cand, t, f(np.inf))                     # a candidate's t is < T <= MAX_FLOAT: never inf, never NaN
        order = np.argsort(key, axis=1, kind="stable")[:, :m]  # equal t: the lower index first
        rows = np.arange(len(sel))[:, None]
        has = cand[rows, order]
        block = np.empty((len(sel), m), dtype=R.HIT)
        block[:] = R.MISS
        block["t"] = np.where(has, t[rows, order], R.MISS["t"])
        block["tri"] = np.where(has, order, 0)
        block["u"] = np.where(has, u[rows, order], f(0))
        block["v"] = np.where(has, v[rows, order], f(0))
        records[sel, :m] = block
    found = np.minimum(candidates, k).astype(np.uint32)
    return Result(records, found, candidates)


def truncate(result, k):
    assert k <= result.records.shape[1]
    return Result(np.ascontiguousarray(result.records[:, :k]), np.minimum(result.candidates, k).astype(np.uint32), result.candidates)
