"""CPU restatement of the triangle distance queries of include/lbvh.h (lbvh_triangle_closest_point, lbvh_triangle_within_distance):
numpy float32, one rounded operation per step, no tree.  A helper module, not a test file.  The arithmetic is imported, not written
again: every edge test is segment_closest_reference.segment_triangle (the pierce first, the nine point tests, the residual), and
the six tests' operands are those of triangle_query_reference.pair_tests, in its order.  What is here is the header's own text: the
order rule over m, the sign of delta, box2q, the candidate rule with `skip`, and the order of the records.

    edge_tests(qa, qb, qc, v0, e1, e2)            the six (P, D, V, E1, E2) of rows of pairs, m = 0 .. 5
    triangle_triangle(qa, qb, qc, v0, e1, e2)     rows of pairs -> Pair(dist2, edge, s, delta)
    box2q(queries, box_lo, box_hi)                box2q of every (query, triangle) pair
    reference(queries, a, b, c, box_lo, box_hi)   -> Result: records layouts.TRI_CLOSEST[count], flags uint32[count], rejected, tested
    brute_force(queries, a, b, c, box_lo, box_hi) the six tests of EVERY pair: what `reference` is held to
    driver_triangles(lo, hi, count, seed)         the queries `lbvh_driver triclosest` generates

box_lo / box_hi are the triangles' OWN boxes (the library's scene.triangle_aabb).

`reference` forms box2q of EVERY pair and runs the six tests on the pairs the candidate rule itself leaves open, as
segment_closest_reference.reference does: a candidate has dist2 < R and !(dist2 < box2q), so a pair with box2q >= R is none, and
once some candidate of a query is known with the distance d, a pair with box2q > d cannot be a candidate at or below d — by the
rule's own comparison, not by any property of the arithmetic."""
from collections import namedtuple

import numpy as np

import segment_closest_reference as G
import triangle_query_reference as TQ
from unitysimpleraytracing_amd.layouts import MAX_FLOAT, TRI_CLOSEST, TRI_DISTANCE_QUERY

F = np.float32
NULL = TQ.NULL
FIRST = 16
NONE = np.zeros(1, dtype=TRI_CLOSEST)[0]
NONE["dist2"] = MAX_FLOAT

Pair = namedtuple("Pair", "dist2 edge s delta")
Result = namedtuple("Result", "records flags rejected tested")


def make_queries(a, b, c, max_dist2=np.inf, skip=NULL):
    q = np.zeros(len(a), dtype=TRI_DISTANCE_QUERY)
    q["a"], q["b"], q["c"], q["max_dist2"], q["skip"] = a, b, c, max_dist2, skip
    return q


def active(queries):
    with np.errstate(invalid="ignore"):
        return TQ.active(queries) & (queries["max_dist2"] > 0)


def radius2(queries):
    """R = min(max_dist2, LBVH_MAX_FLOAT)"""
    return np.minimum(queries["max_dist2"], MAX_FLOAT)


def edge_tests(qa, qb, qc, v0, e1, e2):
    """the operands of triangle_query_reference.pair_tests, in its order: the query's edges against the scene line, then the scene's
    edges against the query's line"""
    ab, ac = qb - qa, qc - qa
    return [(qa, ab, v0, e1, e2), (qb, qc - qb, v0, e1, e2), (qc, qa - qc, v0, e1, e2),
            (v0, e1, qa, ab, ac), (v0, e2, qa, ab, ac), (v0 + e1, e2 - e1, qa, ab, ac)]


def triangle_triangle(qa, qb, qc, v0, e1, e2):
    """rows of pairs, (n, 3) float32 each"""
    n = len(qa)
    with np.errstate(all="ignore"):
        least = np.full(n, np.inf, dtype=F)
        edge = np.zeros(n, dtype=np.uint32)
        s = np.zeros(n, dtype=F)
        delta = np.zeros((n, 3), dtype=F)
        for m, (p, d, v, f1, f2) in enumerate(edge_tests(qa, qb, qc, v0, e1, e2)):
            t = G.segment_triangle(p, d, v, f1, f2)
            pierced = t.which == G.PIERCE
            better = t.dist2 < least                            # strictly less; false for a NaN
            least = np.where(better, t.dist2, least)
            edge = np.where(better, np.uint32(m) | np.where(pierced, np.uint32(8), np.uint32(0)), edge).astype(np.uint32)
            s = np.where(better, t.s, s)
            rv = t.delta if m < 3 else np.where(pierced[:, None], F(0), -t.delta)      # from the scene to the query; +0 where pierced
            delta = np.where(better[:, None], rv, delta)
    assert least.dtype == F and s.dtype == F and delta.dtype == F
    return Pair(least, edge, s, delta)


def query_box(queries):
    qa, qb, qc = (queries[k] for k in "abc")
    with np.errstate(invalid="ignore"):
        return np.minimum(np.minimum(qa, qb), qc), np.maximum(np.maximum(qa, qb), qc)


def box2q(queries, box_lo, box_hi):
    """(queries, triangles): per axis g = max(max(B.lo - Q.max, Q.min - B.hi), 0), then (gx*gx + gy*gy) + gz*gz"""
    qlo, qhi = query_box(queries)
    with np.errstate(all="ignore"):
        g = np.maximum(np.maximum(box_lo[None] - qhi[:, None, :], qlo[:, None, :] - box_hi[None]), F(0))
        assert g.dtype == F
        return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def _store(records, q, p, at, tri):
    records["dist2"][q], records["tri"][q], records["edge"][q] = p.dist2[at], tri, p.edge[at]
    records["s"][q], records["delta"][q] = p.s[at], p.delta[at]


def reference(queries, a, b, c, box_lo, box_hi, pairs_per_chunk=1 << 22):
    assert queries.dtype == TRI_DISTANCE_QUERY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a                                   # what the triangle line of the derived scene holds
    count, n = len(queries), len(a)
    records = np.empty(count, dtype=TRI_CLOSEST)
    records[:] = NONE
    act = active(queries)
    big = radius2(queries)
    rejected = tested = 0
    step = max(1, pairs_per_chunk // max(n, 1))
    for first in range(0, count, step):
        sel = np.nonzero(act[first:first + step])[0] + first
        if len(sel) == 0:
            continue
        sub = queries[sel]
        own = box2q(sub, box_lo, box_hi)
        best = big[sel].copy()                              # the least candidate distance so far; R: none yet
        best_tri = np.full(len(sel), n, dtype=np.int64)
        done = np.zeros(own.shape, dtype=bool)
        with np.errstate(invalid="ignore"):
            open_ = own < best[:, None]                     # dist2 >= box2q for a candidate, and dist2 < R
        open_ &= np.arange(n)[None, :] != sub["skip"].astype(np.int64)[:, None]
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
            p = triangle_triangle(sub["a"][rows], sub["b"][rows], sub["c"][rows], a[tri], e1[tri], e2[tri])
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
            _store(records, sel[r], p, head, tri[head])
    flags = (records["dist2"] != MAX_FLOAT).astype(np.uint32)
    return Result(records, flags, rejected, tested)


def brute_force(queries, a, b, c, box_lo, box_hi):
    """The definition with nothing left out: the six tests of EVERY pair.  For small sets: what `reference` is held to."""
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a
    count, n = len(queries), len(a)
    records = np.empty(count, dtype=TRI_CLOSEST)
    records[:] = NONE
    act, big = active(queries), radius2(queries)
    own = box2q(queries, box_lo, box_hi)
    rows, tri = (x.reshape(-1) for x in np.meshgrid(np.arange(count), np.arange(n), indexing="ij"))
    p = triangle_triangle(queries["a"][rows], queries["b"][rows], queries["c"][rows], a[tri], e1[tri], e2[tri])
    with np.errstate(invalid="ignore"):
        cand = ((p.dist2 < big[rows]) & ~(p.dist2 < own[rows, tri]) & act[rows] & (tri != queries["skip"].astype(np.int64)[rows])).reshape(count, n)
    key = np.where(cand, p.dist2.reshape(count, n), F(np.inf))
    k = key.argmin(axis=1)                                  # the first (lowest-index) minimum
    has = cand[np.arange(count), k]
    at = (np.arange(count) * n + k)[has]
    _store(records, np.nonzero(has)[0], p, at, k[has])
    return records


# ---- the queries of `lbvh_driver triclosest <n> [seed]`: the triangles of `lbvh_driver tris` with a search radius -----------------

def driver_triangles(lo, hi, count, seed=21):
    """triangle_query_reference.driver_triangles' draws (SplitMix64, every draw a scalar fp32 operation in the C++ order); max_dist2 = 4
    for the even ones, +inf for the odd ones; skip = none"""
    qa, qb, qc = TQ.driver_triangles(lo, hi, count, seed)
    return make_queries(qa, qb, qc, np.where(np.arange(count) & 1, F(np.inf), F(4.0)))
