"""CPU restatement of lbvh_triangle_gather_within_distance (include/lbvh.h): every scene triangle within a distance of a triangle, as
a CSR list of layouts.TRI_CLOSEST records.  A helper module, not a test file.  It only JOINS the per-pair pieces of
tests/triangle_closest_reference.py — active, radius2, query_box / box2q, triangle_triangle, _store — and has no arithmetic of its
own: the header defines the call entirely by reference to lbvh_triangle_closest_point.

    reference(queries, a, b, c, box_lo, box_hi)   -> Result: offsets uint64[count + 1], records sorted by tri per segment, tested
    brute_force(queries, a, b, c, box_lo, box_hi) the six tests of EVERY pair: what `reference` is held to
    by_tri(offsets, records)                      any list in the order the two above return: each segment ascending in tri
    driver_triangles(lo, hi, count, seed)         the queries `lbvh_driver triprox` generates

box_lo / box_hi are the triangles' OWN boxes (the library's scene.triangle_aabb).

`reference` runs the six tests only on the pairs with box2q(own) < R, the slot test of the header at the leaf.  That prefilter is
exact: a pair with R <= box2q that had dist2 < R would have dist2 < box2q and be rejected by the accept rule."""
from collections import namedtuple

import numpy as np

import triangle_closest_reference as T
from unitysimpleraytracing_amd.layouts import TRI_CLOSEST, TRI_DISTANCE_QUERY

F = np.float32
Result = namedtuple("Result", "offsets records tested")


def _lists(count, rows, tri, p):
    """candidate pairs (rows ascending, tri ascending inside a row: np.nonzero's order) -> offsets and records"""
    records = np.zeros(len(rows), dtype=TRI_CLOSEST)
    T._store(records, np.arange(len(rows)), p, np.arange(len(rows)), tri)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(rows, minlength=count))
    return offsets, records


def _join(queries, a, b, c, box_lo, box_hi, prefilter, pairs_per_chunk=1 << 22):
    assert queries.dtype == TRI_DISTANCE_QUERY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a                                   # what the triangle line of the derived scene holds
    count, n = len(queries), len(a)
    act, big = T.active(queries), T.radius2(queries)
    all_rows, all_tri, parts = [], [], []
    tested = 0
    step = max(1, pairs_per_chunk // max(n, 1))
    for first in range(0, count, step):
        sel = np.nonzero(act[first:first + step])[0] + first
        if len(sel) == 0:
            continue
        sub = queries[sel]
        own = T.box2q(sub, box_lo, box_hi)
        todo = np.arange(n)[None, :] != sub["skip"].astype(np.int64)[:, None]
        if prefilter:
            with np.errstate(invalid="ignore"):
                todo &= own < big[sel][:, None]
        rows, tri = np.nonzero(todo)                        # row-major: ascending triangle index inside each row
        tested += len(rows)
        if len(rows) == 0:
            continue
        p = T.triangle_triangle(sub["a"][rows], sub["b"][rows], sub["c"][rows], a[tri], e1[tri], e2[tri])
        with np.errstate(invalid="ignore"):
            cand = np.nonzero((p.dist2 < big[sel][rows]) & ~(p.dist2 < own[rows, tri]))[0]
        all_rows.append(sel[rows[cand]])
        all_tri.append(tri[cand])
        parts.append(T.Pair(p.dist2[cand], p.edge[cand], p.s[cand], p.delta[cand]))
    if not parts:
        return Result(np.zeros(count + 1, dtype=np.uint64), np.zeros(0, dtype=TRI_CLOSEST), tested)
    p = T.Pair(*(np.concatenate([getattr(x, f) for x in parts]) for f in T.Pair._fields))
    offsets, records = _lists(count, np.concatenate(all_rows), np.concatenate(all_tri), p)
    return Result(offsets, records, tested)


def reference(queries, a, b, c, box_lo, box_hi):
    return _join(queries, a, b, c, box_lo, box_hi, True)


def brute_force(queries, a, b, c, box_lo, box_hi):
    """The definition with nothing left out: the six tests of EVERY pair (but `skip`).  For small sets."""
    return _join(queries, a, b, c, box_lo, box_hi, False)


def by_tri(offsets, records):
    """a copy of the records with every segment ascending in tri (each triangle appears once per segment: the order is total)"""
    segment = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets).astype(np.int64))
    return records[np.lexsort((records["tri"], segment))]


def driver_triangles(lo, hi, count, seed=21):
    """the draws of `lbvh_driver triclosest` (triangle_closest_reference.driver_triangles), every max_dist2 = 4"""
    q = T.driver_triangles(lo, hi, count, seed)
    q["max_dist2"] = F(4.0)
    return q
