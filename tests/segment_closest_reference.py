"""CPU restatement of the segment queries of include/lbvh.h (lbvh_segment_closest_point, lbvh_segment_within_distance): numpy
float32, one rounded operation per step, no tree.  A helper module, not a test file.  The arithmetic is imported, not written
again: the derived triangles are capsule_reference.derived, dist2 with its barycentrics is point_reference.point_triangle, the box
distance point_reference.box_dist2, the pierce and its t triangle_query_reference.pierce and ray_reference.ray_triangle.  What is
here is the header's own text: the pierce first, the least d_j in the order of j, s from the winning j, the point test at
x = o + h*s, the box grown by the axis, the candidate rule and the order of the records.

    segment_triangle(o, h, a, e1, e2)             rows of pairs -> Pair(dist2, u, v, delta, s, which): which = the winning j, PIERCE
                                                  for the pierce
    grown_box2(queries, box_lo, box_hi)           box2g of every (query, triangle) pair
    reference(queries, a, b, c, box_lo, box_hi)   -> Result: records layouts.SEGMENT_CLOSEST[count], flags uint32[count], which per
                                                  query (-1: none), rejected, tested
    driver_segments(lo, hi, count, seed)          the segments `lbvh_driver segclosest` generates

box_lo / box_hi are the triangles' OWN boxes (the library's scene.triangle_aabb).

`reference` forms box2g of EVERY pair.  The nine point tests and the pierce it evaluates on the pairs the candidate rule itself
leaves open: a candidate has dist2 < R and !(dist2 < box2g), so a pair with box2g >= R is none, and once some candidate of a query
is known with the distance d, a pair with box2g > d cannot be a candidate at or below d — by the rule's own comparison, not by any
property of the arithmetic.  So each query is tested against its FIRST nearest boxes, and then against every pair with box2g <= the
least candidate distance found (R if none was): the record is the one a test of every pair would give."""
from collections import namedtuple

import numpy as np

import capsule_reference as CR
import point_reference as P
import ray_reference as RR
import triangle_query_reference as TQ
from unitysimpleraytracing_amd.layouts import MAX_FLOAT, SEGMENT_CLOSEST, SEGMENT_QUERY

F = np.float32
PIERCE = CR.PIERCE
FIRST = 24
NONE = np.zeros(1, dtype=SEGMENT_CLOSEST)[0]
NONE["dist2"] = MAX_FLOAT

Pair = namedtuple("Pair", "dist2 u v delta s which")
Result = namedtuple("Result", "records flags which rejected tested")


def make_queries(origin, axis, max_dist2):
    q = np.zeros(len(origin), dtype=SEGMENT_QUERY)
    q["origin"], q["axis"], q["max_dist2"] = origin, axis, max_dist2
    return q


def active(queries):
    with np.errstate(invalid="ignore"):
        return (queries["max_dist2"] > 0) & ~np.isnan(queries["origin"]).any(axis=1) & np.isfinite(queries["axis"]).all(axis=1)


def radius2(queries):
    """R = min(max_dist2, LBVH_MAX_FLOAT)"""
    return np.minimum(queries["max_dist2"], MAX_FLOAT)


def segment_triangle(o, h, a, e1, e2):
    """rows of pairs: o, h, a, e1, e2 (n, 3) float32"""
    n = len(o)
    with np.errstate(all="ignore"):
        # 1. the pierce first
        pierced = TQ.pierce(o, h, a, e1, e2)
        t_p = RR.ray_triangle(o, h, a, e1, e2)[0]
        # 2. the least d_j in the order of j, strictly less, and s from the winning j
        least = np.full(n, np.inf, dtype=F)
        which = np.zeros(n, dtype=np.int64)
        s = np.zeros(n, dtype=F)
        for j, (pj, e1j, e2j) in enumerate(CR.derived(a, e1, e2, h)):
            d, _, v1 = P.point_triangle(o, pj, e1j, e2j)
            better = d < least
            least = np.where(better, d, least)
            which = np.where(better, j, which)
            sj = F(0) if j == 0 else F(1) if j == 1 else (F(1) - v1 if j & 1 else v1)
            s = np.where(better, sj, s).astype(F)
        s = np.where(pierced, t_p, s).astype(F)
        which = np.where(pierced, PIERCE, which)
        # 3. on the scene triangle
        x = o + h * s[:, None]
        dist2, u, v = P.point_triangle(x, a, e1, e2)
        ap = x - a
        rv = ap - (e1 * u[:, None] + e2 * v[:, None])
        dist2 = np.where(pierced, F(0), dist2).astype(F)
        delta = np.where(pierced[:, None], F(0), rv).astype(F)
    assert dist2.dtype == F and u.dtype == F and s.dtype == F and delta.dtype == F
    return Pair(dist2, u, v, delta, s, which)


def grown_box2(queries, box_lo, box_hi):
    """(queries, triangles): point_box2 of the origin against lo - max(h, 0), hi - min(h, 0)"""
    with np.errstate(all="ignore"):
        h = queries["axis"][:, None, :]
        glo = box_lo[None] - np.maximum(h, F(0))
        ghi = box_hi[None] - np.minimum(h, F(0))
        assert glo.dtype == F and ghi.dtype == F
        return P.box_dist2(queries["origin"][:, None, :], glo, ghi)


def reference(queries, a, b, c, box_lo, box_hi, pairs_per_chunk=1 << 22):
    assert queries.dtype == SEGMENT_QUERY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a                                   # what the triangle line of the derived scene holds
    count, n = len(queries), len(a)
    records = np.empty(count, dtype=SEGMENT_CLOSEST)
    records[:] = NONE
    which = np.full(count, -1, dtype=np.int64)
    act = active(queries)
    big = radius2(queries)
    rejected = tested = 0
    step = max(1, pairs_per_chunk // max(n, 1))
    for first in range(0, count, step):
        sel = np.nonzero(act[first:first + step])[0] + first
        if len(sel) == 0:
            continue
        sub = queries[sel]
        own = grown_box2(sub, box_lo, box_hi)
        best = big[sel].copy()                              # the least candidate distance so far; R: none yet
        best_tri = np.full(len(sel), n, dtype=np.int64)
        done = np.zeros(own.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            open_ = own < best[:, None]                     # dist2 >= box2g for a candidate, and dist2 < R
        for rnd in range(2):
            if rnd == 0:                                    # the FIRST nearest boxes of each query
                k = min(FIRST, n)
                near = np.argpartition(np.where(open_, own, F(np.inf)), k - 1, axis=1)[:, :k]
                todo = np.zeros(own.shape, dtype=bool)
                np.put_along_axis(todo, near, True, axis=1)
                todo &= open_
            else:                                           # every pair the candidate found (or R) does not exclude
                with np.errstate(invalid="ignore"):
                    todo = open_ & ~done & (own <= best[:, None])
            rows, tri = np.nonzero(todo)                    # row-major: ascending triangle index inside each row
            done |= todo
            tested += len(rows)
            if len(rows) == 0:
                continue
            p = segment_triangle(sub["origin"][rows], sub["axis"][rows], a[tri], e1[tri], e2[tri])
            with np.errstate(invalid="ignore"):
                inside = p.dist2 < big[sel][rows]
                front = p.dist2 < own[rows, tri]
            rejected += int((inside & front).sum())
            cand = np.nonzero(inside & ~front)[0]
            # per query the least dist2, ties to the lower index: sort by (row, dist2, tri) and take each row's first
            order = cand[np.lexsort((tri[cand], p.dist2[cand], rows[cand]))]
            head = order[np.concatenate([[True], rows[order][1:] != rows[order][:-1]])] if len(order) else order
            r = rows[head]
            better = (p.dist2[head] < best[r]) | ((p.dist2[head] == best[r]) & (tri[head] < best_tri[r]))
            head, r = head[better], r[better]
            best[r], best_tri[r] = p.dist2[head], tri[head]
            q = sel[r]
            records["dist2"][q], records["tri"][q], records["u"][q], records["v"][q] = p.dist2[head], tri[head], p.u[head], p.v[head]
            records["delta"][q], records["s"][q] = p.delta[head], p.s[head]
            which[q] = p.which[head]
    flags = (records["dist2"] != MAX_FLOAT).astype(np.uint32)
    return Result(records, flags, which, rejected, tested)


def brute_force(queries, a, b, c, box_lo, box_hi):
    """The definition with nothing left out: the nine tests and the pierce of EVERY pair.  For small sets: what `reference` is
    held to."""
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a
    count, n = len(queries), len(a)
    records = np.empty(count, dtype=SEGMENT_CLOSEST)
    records[:] = NONE
    act, big = active(queries), radius2(queries)
    own = grown_box2(queries, box_lo, box_hi)
    rows, tri = (x.reshape(-1) for x in np.meshgrid(np.arange(count), np.arange(n), indexing="ij"))
    p = segment_triangle(queries["origin"][rows], queries["axis"][rows], a[tri], e1[tri], e2[tri])
    with np.errstate(invalid="ignore"):
        cand = ((p.dist2 < big[rows]) & ~(p.dist2 < own[rows, tri]) & act[rows]).reshape(count, n)
    key = np.where(cand, p.dist2.reshape(count, n), F(np.inf))
    k = key.argmin(axis=1)                                  # the first (lowest-index) minimum
    has = cand[np.arange(count), k]
    at = (np.arange(count) * n + k)[has]
    records["dist2"][has], records["tri"][has], records["u"][has], records["v"][has] = p.dist2[at], k[has], p.u[at], p.v[at]
    records["delta"][has], records["s"][has] = p.delta[at], p.s[at]
    return records


# ---- the segments of `lbvh_driver segclosest <n> [seed]`: SplitMix64, every draw a scalar fp32 operation in the C++ order ---------

def driver_segments(lo, hi, count, seed=15):
    """per segment and axis k: the origin in the mesh's box, then the axis component in [-6, 6]; max_dist2 = 9 for the even ones,
    +inf for the odd ones"""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    q = np.zeros(count, dtype=SEGMENT_QUERY)
    for i in range(count):
        for k in range(3):
            q["origin"][i, k] = uni(lo[k], hi[k])
            q["axis"][i, k] = uni(-6.0, 6.0)
    q["max_dist2"] = np.where(np.arange(count) & 1, F(np.inf), F(9.0))
    return q
