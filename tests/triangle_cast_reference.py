"""CPU restatement of the triangle casts of include/lbvh.h (lbvh_triangle_cast, lbvh_triangle_cast_any): numpy float32, one rounded
operation per step, brute force over every (cast, triangle) pair — no tree.  A helper module, not a test file.  The slab test is
ray_reference.box_entry and the six start tests are triangle_query_reference.pierce, imported, not written again.  pierce returns
only whether 0 <= t <= 1, and the fifteen features need the t (and the edge pairs the parallelogram's rejection), so `pierce_t`
here is the header's text once more with t, u and the `quad` mode; `pair_time` holds it to pierce on features 0 - 5 (the same P, D,
V, E1, E2: pierce passes exactly where pierce_t has 0 <= t <= 1).

    pierce_t(P, D, V, E1, E2, quad)        -> (t, u, v, det): t = LBVH_MAX_FLOAT on a rejection
    pair_time(qa, qb, qc, d, v0, e1, e2, start_allowed)  rows of pairs -> (t, feature, w); t = LBVH_MAX_FLOAT: no time
    grown_entry(casts, lo, hi)             (passes, entry) of every cast's ray (a, dir) against every box grown by the query's extent
    reference(casts, a, b, c, box_lo, box_hi) -> Result(records, flags, ties)
    driver_casts(lo, hi, count, seed, t_max)   the casts `lbvh_driver tricast` generates

`reference` takes the triangles' positions and their OWN boxes (the library's scene.triangle_aabb)."""
from collections import namedtuple

import numpy as np

import ray_reference as RR
import triangle_query_reference as TQ
from unitysimpleraytracing_amd.layouts import MAX_FLOAT, TRI_CAST_HIT, TRI_CAST_START, TRI_RAY

F = np.float32
NULL = 0xFFFFFFFF
MISS = np.array([(MAX_FLOAT, 0, 0, 0.0)], dtype=TRI_CAST_HIT)[0]

Result = namedtuple("Result", "records flags ties")


def make_casts(a, b, c, direction, t_max=F(np.inf), skip=NULL):
    q = np.zeros(len(a), dtype=TRI_RAY)
    q["a"], q["b"], q["c"], q["dir"], q["t_max"], q["skip"] = a, b, c, direction, t_max, skip
    return q


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def active(casts):
    with np.errstate(all="ignore"):
        d = casts["dir"].astype(F)
        return np.isfinite(casts["a"]).all(axis=1) & np.isfinite(casts["b"]).all(axis=1) & np.isfinite(casts["c"]).all(axis=1) & \
            np.isfinite(d).all(axis=1) & (_dot(d, d) > 0) & (casts["t_max"] > 0)


def limit(casts):
    """T = min(t_max, LBVH_MAX_FLOAT)"""
    return np.minimum(casts["t_max"], MAX_FLOAT)


def pierce_t(P, D, V, E1, E2, quad=False):
    """the header's pierce (quad: pierce_quad) with its numbers: (t, u, v, det), t = LBVH_MAX_FLOAT where a rejection applies; a
    comparison with a NaN is false, so a NaN u or v rejects nothing"""
    P, D, V, E1, E2 = (np.asarray(x, dtype=F) for x in (P, D, V, E1, E2))
    with np.errstate(all="ignore"):
        p = _cross(D, E2)
        det = _dot(E1, p)
        miss = (det < F(1e-8)) & (det > F(-1e-8))
        inv = F(1.0) / det
        s = P - V
        u = _dot(s, p) * inv
        miss |= (u < F(0.0)) | (u > F(1.0))
        q = _cross(s, E1)
        v = _dot(D, q) * inv
        miss |= (v < F(0.0)) | ((v if quad else u + v) > F(1.0))
        t = _dot(E2, q) * inv
    return np.where(miss, MAX_FLOAT, t).astype(F), u, v, det


def feature_tests(qa, qb, qc, d, v0, e1, e2):
    """[(P, D, V, E1, E2, quad) for feature 0 .. 14], every vector formed per component in fp32"""
    with np.errstate(all="ignore"):
        ab, bc, ca, ac = qb - qa, qc - qb, qa - qc, qc - qa
        v1, v2, e3 = v0 + e1, v0 + e2, e2 - e1
        back = -d
    tests = [(x, d, v0, e1, e2, False) for x in (qa, qb, qc)] + [(y, back, qa, ab, ac, False) for y in (v0, v1, v2)]
    for p, e in ((qa, ab), (qb, bc), (qc, ca)):
        for q, f in ((v0, e1), (v0, e2), (v1, e3)):
            tests.append((p, d, q, f, -e, True))
    return tests


def start_test(qa, qb, qc, v0, e1, e2):
    """the six edge tests of lbvh_triangle_intersections in its order -> the first passing j, -1 if none"""
    with np.errstate(all="ignore"):
        ab, bc, ca, ac = qb - qa, qc - qb, qa - qc, qc - qa
        passed = np.stack([TQ.pierce(qa, ab, v0, e1, e2), TQ.pierce(qb, bc, v0, e1, e2), TQ.pierce(qc, ca, v0, e1, e2),
                           TQ.pierce(v0, e1, qa, ab, ac), TQ.pierce(v0, e2, qa, ab, ac), TQ.pierce(v0 + e1, e2 - e1, qa, ab, ac)], axis=-1)
    return np.where(passed.any(axis=-1), passed.argmax(axis=-1), -1)


def pair_time(qa, qb, qc, d, v0, e1, e2, start_allowed, with_det=False):
    """rows of pairs, every vector (n, 3) float32; start_allowed: rule (2), the own box overlaps the query's -> (t, feature, w), and
    with_det the winning test's (det, |D| |E1| |E2|) in float64 for the conditioning of the float64 comparison"""
    for x in (qa, qb, qc, d, v0, e1, e2):
        assert x.dtype == F
    n = len(qa)
    best = np.full(n, MAX_FLOAT, dtype=F)
    feature = np.zeros(n, dtype=np.uint32)
    w = np.zeros(n, dtype=F)
    det_best, scale_best = np.zeros(n), np.ones(n)
    for j, (P, D, V, E1, E2, quad) in enumerate(feature_tests(qa, qb, qc, d, v0, e1, e2)):
        t, u, _, det = pierce_t(P, D, V, E1, E2, quad)
        if j < 6:                                                  # the imported pierce agrees on the same five vectors
            with np.errstate(invalid="ignore"):
                assert (TQ.pierce(P, D, V, E1, E2) == ((t < MAX_FLOAT) & (F(0) <= t) & (t <= F(1)))).all()
        with np.errstate(invalid="ignore"):
            better = (t >= F(0)) & (t < best)
        best = np.where(better, t, best)
        feature = np.where(better, j, feature).astype(np.uint32)
        w = np.where(better, u if quad else F(0), w).astype(F)
        if with_det:
            norm = lambda x: np.linalg.norm(x.astype(np.float64), axis=-1)
            det_best = np.where(better, det.astype(np.float64), det_best)
            scale_best = np.where(better, norm(D) * norm(E1) * norm(E2), scale_best)
    j0 = start_test(qa, qb, qc, v0, e1, e2)
    start = start_allowed & (j0 >= 0)
    best = np.where(start, F(0), best).astype(F)
    feature = np.where(start, TRI_CAST_START | np.maximum(j0, 0), feature).astype(np.uint32)
    w = np.where(start, F(0), w).astype(F)
    return (best, feature, w, det_best, scale_best) if with_det else (best, feature, w)


def grown_entry(casts, lo, hi):
    """(passes, entry), each (casts, triangles): the walkers' slab test of the ray (a, dir) against min - max(h1, h2, 0) and
    max - min(h1, h2, 0), h1 = b - a, h2 = c - a"""
    with np.errstate(all="ignore"):
        inv = F(1) / casts["dir"].astype(F)
        h1, h2 = casts["b"] - casts["a"], casts["c"] - casts["a"]
        under = np.fmax(np.fmax(h1, h2), F(0))[:, None, :]
        over = np.fmin(np.fmin(h1, h2), F(0))[:, None, :]
        return RR.box_entry(casts["a"][:, None, :], inv[:, None, :], lo[None] - under, hi[None] - over)


def own_box_overlaps(sub, qi, ti, lo, hi):
    """rule (2) of lbvh_triangle_intersections for the pairs (qi, ti)"""
    qa, qb, qc = sub["a"][qi], sub["b"][qi], sub["c"][qi]
    qlo, qhi = np.minimum(np.minimum(qa, qb), qc), np.maximum(np.maximum(qa, qb), qc)
    return ((qlo <= hi[ti]) & (lo[ti] <= qhi)).all(axis=1)


def reference(casts, a, b, c, box_lo, box_hi, casts_per_chunk=128):
    """Brute force in float32.  casts: TRI_RAY array; a, b, c: (T, 3) positions; box_lo, box_hi: (T, 3) the triangles' own boxes.
    records: the candidate with the least t, ties to the lower index, or the miss record; flags: 1 where a candidate exists; ties:
    how many candidates share the least t."""
    assert casts.dtype == TRI_RAY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    lo, hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a                                            # what the triangle line of the derived scene holds
    n, nt = len(casts), len(a)
    records = np.empty(n, dtype=TRI_CAST_HIT)
    records[:] = MISS
    flags = np.zeros(n, dtype=np.uint32)
    ties = np.zeros(n, dtype=np.uint32)
    act = active(casts)
    big = limit(casts)
    for first in range(0, n, casts_per_chunk):
        sel = np.nonzero(act[first:first + casts_per_chunk])[0] + first
        if len(sel) == 0:
            continue
        sub = casts[sel]
        passes, entry = grown_entry(sub, lo, hi)
        passes &= np.arange(nt, dtype=np.int64)[None] != sub["skip"].astype(np.int64)[:, None]
        qi, ti = np.nonzero(passes)
        t, feature, w = pair_time(sub["a"][qi], sub["b"][qi], sub["c"][qi], sub["dir"][qi], a[ti], e1[ti], e2[ti],
                                  own_box_overlaps(sub, qi, ti, lo, hi))
        with np.errstate(invalid="ignore"):
            cand = (t < big[sel][qi]) & ~(t < entry[qi, ti])
        key = np.full(passes.shape, F(np.inf))
        key[qi[cand], ti[cand]] = t[cand]
        pair = np.full(passes.shape, -1, dtype=np.int64)
        pair[qi, ti] = np.arange(len(qi))
        k = key.argmin(axis=1)                                      # the first (lowest-index) minimum; -0 and +0 compare equal
        rows = np.arange(len(sel))
        has = np.isfinite(key[rows, k])
        hit, kh, ph = sel[has], k[has], pair[rows, k][has]
        records["t"][hit], records["tri"][hit], records["feature"][hit], records["w"][hit] = t[ph], kh, feature[ph], w[ph]
        flags[hit] = 1
        ties[hit] = (key[has] == key[rows, k][has][:, None]).sum(axis=1)
    return Result(records, flags, ties)


def nearest(casts, a, b, c, casts_per_chunk=32):
    """(t, tri, feature, w, det, scale): the least time below T over ALL triangles in float32 with no box rule (the start tests
    allowed everywhere), the lowest index on a tie; t = +inf where there is none; det and scale of the winning test in float64"""
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    e1, e2 = b - a, c - a
    n, nt = len(casts), len(a)
    out = np.full(n, np.inf, dtype=F)
    tri, feat = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    wout, det, scale = np.zeros(n, dtype=F), np.zeros(n), np.ones(n)
    act = active(casts)
    big = limit(casts)
    for first in range(0, n, casts_per_chunk):
        sel = np.nonzero(act[first:first + casts_per_chunk])[0] + first
        if len(sel) == 0:
            continue
        sub = casts[sel]
        qi, ti = np.repeat(np.arange(len(sel)), nt), np.tile(np.arange(nt), len(sel))
        t, f, w, dt, sc = pair_time(sub["a"][qi], sub["b"][qi], sub["c"][qi], sub["dir"][qi], a[ti], e1[ti], e2[ti],
                                    np.ones(len(qi), dtype=bool), with_det=True)
        shape = (len(sel), nt)
        t = np.where(t < big[sel][qi], t, F(np.inf)).reshape(shape)
        k = t.argmin(axis=1)
        r = np.arange(len(sel))
        out[sel], tri[sel], feat[sel], wout[sel] = t[r, k], k, f.reshape(shape)[r, k], w.reshape(shape)[r, k]
        det[sel], scale[sel] = dt.reshape(shape)[r, k], sc.reshape(shape)[r, k]
    return out, tri, feat, wout, det, scale


# ---- the casts of `lbvh_driver tricast <n> [seed] [t_max]`: SplitMix64, every draw a scalar fp32 operation in the C++ order

def driver_casts(lo, hi, count, seed=5, t_max=2.0):
    """per cast and axis k: the vertex a around the mesh's box (as query_support.driver_rays draws an origin), b's and c's offsets
    uniform in [-3, 3], then dir = a target uniform in the box minus a"""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    casts = np.zeros(count, dtype=TRI_RAY)
    for i in range(count):
        for k in range(3):
            grow = F(0.25) * F(hi[k] - lo[k])
            av = uni(F(lo[k] - grow), F(hi[k] + grow))
            casts["a"][i, k] = av
            casts["b"][i, k] = F(av + uni(-3.0, 3.0))
            casts["c"][i, k] = F(av + uni(-3.0, 3.0))
            casts["dir"][i, k] = F(uni(lo[k], hi[k]) - av)
    casts["t_max"] = F(t_max)
    casts["skip"] = NULL
    return casts
