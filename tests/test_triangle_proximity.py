"""lbvh_triangle_gather_within_distance: every scene triangle within a distance of a triangle, one 32-byte lbvh_tri_closest record per
pair, as a CSR list over the four-wide derived traversal scene.  The expectation is tests/triangle_proximity_reference.py, which only
joins the per-pair pieces of tests/triangle_closest_reference.py.  Records are compared on uint32 views after sorting each segment
by tri; the offsets word for word.
  CPU  the surface in every host; hand-made pairs with answers derivable on paper; the reference against the test of every pair;
       relations (a), (b), (c) in the reference; unique_self_pairs on a 2 x 2 grid of quads; the parity sets are not vacuous
  T1   parity of the full and the count-only form             T2  relations (a) - (d) against the three existing calls
  T3   query counts around a wave; wave caps (the lane refill)  T4  every way of being inactive
  T5   the entry-point contract on a context of its own; capacities; one unbounded query
  T6   a small LDS stack; the stack limit; statistics          T7  hostile walk shapes
  T8   .proximity_pairs; unique_self_pairs on the grid; lbvh_driver triprox: the C++ host end to end

The parity set is test_triangle_closest.parity_queries unchanged, its unbounded half given radii drawn as the bounded half's (own
seed), so that no query lists the whole mesh.  On grid_80x80 the range 0.5 .. 5 % of the extent meets every condition of
test_the_parity_sets_are_not_vacuous as drawn.  On cfg1_4096 (4 096 scattered triangles) it gave 20 segments of more than 8 records
and none of more than 64; the upper end was raised for that scene, 5 -> 10 -> 15 %, until the CPU reference alone met them
(474 and 36 at 15 %)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hostile_scenes
import triangle_closest_reference as T
import triangle_proximity_reference as X
import triangle_query_reference as TQ
from query_support import driver_mesh, H, L, library_boxes, N, pack, padded_boxes, positions, words
from test_shape_overlaps import extent_of, PARITY, scene
from test_triangle_closest import COUNT, OWN, gpu_scene, parity_queries, small_case, spoiled, tri_queries_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAME = "lbvh_triangle_gather_within_distance"
UPPER = {"grid_80x80": 0.05, "cfg1_4096": 0.15}           # the upper end of the radius range (see the module's docstring)
POISON = 0x7FC0DEAD


def rw(records):
    """layouts.TRI_CLOSEST records -> (rows, 8) words"""
    return words(records).reshape(-1, 8)


def proximity_queries(name, a, b, c):
    q, r = parity_queries(a, b, c)
    rng = np.random.default_rng(41 + len(a))
    fill = (extent_of(a, b, c) * rng.uniform(0.005, UPPER[name], len(q))).astype(F)
    r = np.where(np.isinf(r), fill, r).astype(F)
    q["max_dist2"] = r * r
    return q


def take(off, rec, rows, empty=()):
    """the list of the queries `rows` of a list sorted by tri, those at the positions `empty` (of rows) with nothing"""
    n = np.diff(off).astype(np.int64)[rows]
    n[list(empty)] = 0
    parts = [rec[int(off[k]):int(off[k]) + int(m)] for k, m in zip(rows, n)]
    out = np.zeros(len(rows) + 1, dtype=np.uint64)
    out[1:] = np.cumsum(n)
    return out, (np.concatenate(parts) if parts else rec[:0])


def assert_lists(got_off, got_rec, want_off, want_rec, what=""):
    """offsets word for word; records on uint32 views after sorting each segment by tri"""
    assert got_off.dtype == np.uint64 and (got_off == want_off).all(), (what, np.nonzero(got_off != want_off)[0][:5])
    total = int(want_off[-1])
    got = rw(X.by_tri(got_off, got_rec[:total]))
    bad = np.nonzero((got != rw(want_rec)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:3]], rw(want_rec)[bad[:3]])


_CPU = {}


def cpu_case(name):
    """(a, b, c, box_lo, box_hi, queries, reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        lo, hi = padded_boxes(a, b, c)
        q = proximity_queries(name, a, b, c)
        _CPU[name] = (a, b, c, lo, hi, q, X.reference(q, a, b, c, lo, hi))
    return _CPU[name]


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_the_surface_in_every_host():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"lbvh_status lbvh_triangle_gather_within_distance\(lbvh_context\* ctx, const lbvh_tri_distance_query\* d_queries, size_t count,\s+"
                     r"const lbvh_scene\* h_scene, uint64_t\* d_offsets, lbvh_tri_closest\* d_records,\s+uint64_t capacity\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert NAME in bounce
    text = h[h.index("Triangle proximity: EVERY scene triangle"):h.index("lbvh_status lbvh_triangle_gather_within_distance(")]
    text = re.sub(r"\s*\n \*\s+", " ", text)                            # (the comment's line breaks are not part of the wording)
    for must in ("!= skip", "dist2_i < R", "!(dist2_i < box2q(own AABB_i))", "were that triangle the only one", "box2q(slot) < R (false for a NaN)",
                 "box2q(ancestor) <= box2q(leaf) <= dist2 < R", "fixed bound", "each candidate appears exactly once", "Always written in full",
                 "NOT PART OF THE CONTRACT", "no record at index >= capacity is ever written", "capacity == 0", "d_records may be NULL",
                 "d_records == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG", "never waits on the host", "write the same bytes",
                 "An inactive query gets an empty segment", "(a) segment k is non-empty exactly when", "all eight words",
                 "dist2 == +0 and edge & 8 set", "The converse is NOT promised", "(d) the capacity == 0 form writes the same offsets",
                 "lists the whole mesh", "BOTH walks", "a device-side sort of 32-byte records", "the k nearest triangles of a triangle",
                 "two-tree", "(i, j) / (j, i) duplicates"):
        assert must in text, must
    closest = h[h.index("Triangle closest-point queries: HOW FAR"):h.index("lbvh_status lbvh_triangle_closest_point(")]
    assert "a gather of every triangle within the distance" not in closest and "Out of scope: the k nearest" in closest
    assert NAME in closest
    assert NAME in open(os.path.join(ROOT, "include", "lbvh_debug.h")).read()
    nat = N()
    res, args = nat.SIGNATURES[NAME]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
    assert hasattr(nat.lib, NAME) and nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_triangle_gather_within_distance\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, "
                     r"IntPtr \w+,\s+IntPtr \w+, ulong capacity\);", cs)
    tp = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "TriangleProximity.cs")).read())
    assert NAME in tp and "unsafe" not in tp
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void TriangleGatherWithinDistance(" in hpp
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"triprox", triprox_main}' in drv and "lbvh_driver triprox <n_queries> [seed]" in drv
    drawer = H().RaytracingMeshDrawer
    assert all(callable(getattr(drawer, m)) for m in ("triangle_gather_within_distance", "proximity_pairs"))
    assert callable(H().unique_self_pairs)


# ---- CPU: hand-made pairs with answers derivable on paper ----------------------------------------------------------------------

FLOOR = np.array([[(0, 0, 0), (4, 0, 0), (0, 4, 0)], [(4, 0, 0), (4, 4, 0), (0, 4, 0)]], dtype=F)       # two coplanar triangles


def hand(qa, qb, qc, max_dist2=np.inf, skip=T.NULL, tris=FLOOR):
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    q = T.make_queries(np.array([qa], dtype=F), np.array([qb], dtype=F), np.array([qc], dtype=F), F(max_dist2), skip)
    r = X.reference(q, a, b, c, *padded_boxes(a, b, c))
    bf = X.brute_force(q, a, b, c, *padded_boxes(a, b, c))
    assert (r.offsets == bf.offsets).all() and (rw(r.records) == rw(bf.records)).all()
    return r


def test_reference_a_parallel_triangle_above_two_coplanar_ones():
    # every point of the query is 0.75 above the square; it reaches over both triangles (the diagonal x + y = 4)
    tri = ((1, 1, 0.75), (3, 1, 0.75), (3, 3, 0.75))
    r = hand(*tri)
    assert r.offsets.tolist() == [0, 2] and r.records["tri"].tolist() == [0, 1] and (r.records["dist2"] == 0.5625).all()
    assert (r.records["_zero"] == 0).all() and (r.records["delta"] == (0, 0, 0.75)).all()
    # the radius is open: dist2 == max_dist2 lists none
    assert hand(*tri, 0.5625).offsets.tolist() == [0, 0] and hand(*tri, 0.5626).offsets.tolist() == [0, 2]
    # each record is what the closest call would write were that triangle the only one
    for k in range(2):
        one = FLOOR[k:k + 1]
        q = T.make_queries(*(np.array([v], dtype=F) for v in tri))
        alone = T.reference(q, one[:, 0], one[:, 1], one[:, 2], *padded_boxes(one[:, 0], one[:, 1], one[:, 2])).records
        alone["tri"] = k
        assert rw(alone).tolist() == rw(r.records[k:k + 1]).tolist()


def test_reference_a_pierced_triangle_is_listed_for_any_positive_radius():
    # the edge a-b goes through triangle 0 at (0.5, 0.5, 0); the query lies in the plane x = y on the side away from the diagonal of
    # the square, 1.5 * sqrt(2) from triangle 1
    r = hand((0.5, 0.5, -1), (0.5, 0.5, 3), (-9, -9, 1), 1e-30)
    assert r.offsets.tolist() == [0, 1] and r.records["tri"][0] == 0 and words(r.records["dist2"])[0] == 0
    assert r.records["edge"][0] == 8 and r.records["s"][0] == 0.25 and words(r.records["delta"]).reshape(-1).tolist() == [0, 0, 0]
    # with the third vertex beyond the diagonal, the diagonal — an edge of triangle 1 too — goes through the query's face: both are listed
    r = hand((1, 1, -1), (1, 1, 3), (9, 9, 1), 1e-30)
    assert r.records["tri"].tolist() == [0, 1] and (words(r.records["dist2"]) == 0).all() and (r.records["edge"] & 8 != 0).all()


def test_reference_skip_removes_its_triangle_only():
    tri = ((1, 1, 0.75), (3, 1, 0.75), (3, 3, 0.75))
    assert hand(*tri, skip=0).records["tri"].tolist() == [1] and hand(*tri, skip=1).records["tri"].tolist() == [0]
    assert hand(*tri, skip=2).records["tri"].tolist() == [0, 1]


def test_reference_inactive_queries_have_empty_segments():
    a, b, c = FLOOR[:, 0], FLOOR[:, 1], FLOOR[:, 2]
    v = np.tile(np.array([[(1, 1, 0.75), (3, 1, 0.75), (3, 3, 0.75)]], dtype=F), (6, 1, 1))
    q = T.make_queries(v[:, 0], v[:, 1], v[:, 2])
    q["a"][1, 0], q["c"][2, 2] = np.nan, np.inf
    q["max_dist2"][3:5] = (0, np.nan)
    r = X.reference(q, a, b, c, *padded_boxes(a, b, c))
    assert r.offsets.tolist() == [0, 2, 2, 2, 2, 2, 4]


# ---- CPU: the reference and the test of every pair; the relations; the sets -------------------------------------------------------

def test_the_reference_is_the_test_of_every_pair():
    for name in PARITY:
        a, b, c, lo, hi, q, ref = cpu_case(name)
        for rows in (np.arange(48), np.arange(COUNT - 16, COUNT)):
            bf = X.brute_force(q[rows], a, b, c, lo, hi)
            assert_lists(bf.offsets, bf.records, *take(ref.offsets, ref.records, rows), (name, int(rows[0])))
        assert ref.tested < 0.02 * COUNT * len(a)


def check_relations(q, off, rec, flags, closest, hit_off, hit_tris):
    """(a), (b), (c) for a list sorted or not -> (non-empty segments, listed intersections)"""
    n = np.diff(off).astype(np.int64)
    assert ((n > 0) == (flags == 1)).all()                                                      # (a)
    segment = np.repeat(np.arange(len(q)), n)
    order = np.lexsort((rec["tri"], rec["dist2"], segment))                                      # dist2 >= 0: the value order
    first = order[np.concatenate([[True], segment[order][1:] != segment[order][:-1]])] if len(order) else order
    assert (rw(rec[first]) == rw(closest[n > 0])).all()                                         # (b)
    assert (closest["dist2"][n == 0] == T.MAX_FLOAT).all()
    listed = 0
    for k in np.nonzero(np.diff(hit_off).astype(np.int64))[0]:                                    # (c)
        seg = rec[int(off[k]):int(off[k + 1])]
        for t in hit_tris[int(hit_off[k]):int(hit_off[k + 1])]:
            at = np.nonzero(seg["tri"] == t)[0]
            assert len(at) == 1 and words(seg["dist2"][at])[0] == 0 and seg["edge"][at[0]] & 8, (k, t)
            listed += 1
    return int((n > 0).sum()), listed


def test_relations_a_b_and_c_in_the_reference():
    for name in PARITY:
        a, b, c, lo, hi, q, ref = cpu_case(name)
        near = T.reference(q, a, b, c, lo, hi)
        hit = TQ.reference(tri_queries_of(q), a, b, c, lo, hi)
        nonempty, listed = check_relations(q, ref.offsets, ref.records, near.flags, near.records, hit.offsets, hit.tris)
        print(f"{name}: {nonempty} non-empty segments, {listed} intersections listed at +0")
        assert listed >= 100


def test_unique_self_pairs_on_a_two_by_two_grid_of_quads():
    """Vertices (i, j), i, j = 0 .. 2; quad (i, j) is cut along its diagonal (i, j) - (i + 1, j + 1) into triangle 2k (below it) and
    2k + 1 (above it), k = 2 j + i:
        0 (0,0) (1,0) (1,1)    1 (0,0) (1,1) (0,1)    2 (1,0) (2,0) (2,1)    3 (1,0) (2,1) (1,1)
        4 (0,1) (1,1) (1,2)    5 (0,1) (1,2) (0,2)    6 (1,1) (2,1) (2,2)    7 (1,1) (2,2) (1,2)
    Six hold the centre (1, 1) and share it pairwise.  Triangle 2 touches 0 and 3 at (1, 0), 3 and 6 at (2, 1); triangle 5 touches 1
    and 4 at (0, 1), 4 and 7 at (1, 2).  Of the 28 unordered pairs that leaves (0, 5), (1, 2), (2, 4), (2, 5), (2, 7), (3, 5), (5, 6)."""
    tri = []
    for j in range(2):
        for i in range(2):
            tri += [[(i, j, 0), (i + 1, j, 0), (i + 1, j + 1, 0)], [(i, j, 0), (i + 1, j + 1, 0), (i, j + 1, 0)]]
    v = np.array(tri, dtype=F)
    mesh = (v[:, 0], v[:, 1], v[:, 2])
    every = np.zeros(8 * 7, dtype=L().TRI_CLOSEST)
    every["tri"] = [t for k in range(8) for t in range(8) if t != k]
    off = np.arange(9, dtype=np.uint64) * 7
    pairs, kept = H().unique_self_pairs(off, every, mesh)
    flat = [[0, 5], [1, 2], [2, 4], [2, 5], [2, 7], [3, 5], [5, 6]]
    assert pairs.tolist() == flat and kept["tri"].tolist() == [j for i, j in flat]
    # triangles 0 and 7 lifted off the plane share nothing any more: every pair with them is kept as well
    w = v.copy()
    w[0, :, 2], w[7, :, 2] = 1, 2
    pairs, kept = H().unique_self_pairs(off, every, (w[:, 0], w[:, 1], w[:, 2]))
    assert pairs.tolist() == sorted(flat + [[0, t] for t in range(1, 8) if t != 5] + [[t, 7] for t in range(1, 7) if t != 2])
    assert kept["tri"].tolist() == pairs[:, 1].tolist()
    w[np.arange(8), :, 2] = np.arange(8, dtype=F)[:, None]
    pairs, kept = H().unique_self_pairs(off, every, pack(w[:, 0], w[:, 1], w[:, 2]))          # layouts.TRIANGLE is taken the same way
    assert pairs.tolist() == [[i, j] for i in range(8) for j in range(i + 1, 8)]
    # a partial list: the order is the list's, (j, i) alone is dropped
    some = every[[0, 10, 50]]                                             # (0, 1), (1, 4), (7, 1)
    pairs, kept = H().unique_self_pairs(np.array([0, 1, 2, 2, 2, 2, 2, 2, 3], dtype=np.uint64), some, (w[:, 0], w[:, 1], w[:, 2]))
    assert pairs.tolist() == [[0, 1], [1, 4]] and (rw(kept) == rw(some[:2])).all()


def edge_neighbours(a, b, c, k):
    """the triangles that share exactly two vertices (equal words) with triangle k"""
    v = np.stack([a, b, c], axis=1).view(np.uint32)
    same = (v[:, :, None, :] == v[k][None, None, :, :]).all(axis=3).any(axis=2).sum(axis=1)
    return np.nonzero(same == 2)[0]


def test_the_parity_sets_are_not_vacuous():
    for name in PARITY:
        a, b, c, lo, hi, q, ref = cpu_case(name)
        n = np.diff(ref.offsets).astype(np.int64)
        rec = ref.records
        by_m = np.bincount((rec["edge"] & 7).astype(np.int64), minlength=6)
        pierced = int((rec["edge"] & 8 != 0).sum())
        print(f"{name}: {int((n > 0).sum())} non-empty, {int((n == 0).sum())} empty, {int((n > 8).sum())} of more than 8, {int((n > 64).sum())} of more "
              f"than 64, longest {int(n.max())}, {int(n.sum())} records, {pierced} pierced, winning m {by_m.tolist()}, {ref.tested} pairs tested")
        assert len(q) == COUNT and T.active(q).all() and np.isfinite(q["max_dist2"]).all() and n.max() < len(a) // 8
        assert (n > 0).sum() >= 500 and (n == 0).sum() >= 100 and (n > 8).sum() >= 100 and (n > 64).sum() >= 1
        assert pierced >= 100 and (by_m >= 20).all()
        assert (q["skip"][-OWN:] == np.arange(OWN) * (len(a) // OWN)).all()
        segment = np.repeat(np.arange(COUNT), n)
        assert (rec["tri"] != q["skip"][segment]).all()
        if name == "grid_80x80":                                           # an own triangle lists its edge neighbours at +0
            three = 0
            for k in range(COUNT - OWN, COUNT):
                seg = rec[int(ref.offsets[k]):int(ref.offsets[k + 1])]
                beside = edge_neighbours(a, b, c, int(q["skip"][k]))
                three += len(beside) == 3
                assert 2 <= len(beside) <= 3 and all(words(seg["dist2"][seg["tri"] == t]).tolist() == [0] for t in beside), k
                assert (words(seg["dist2"]) == 0).sum() >= 3
            assert three >= OWN - 16                                         # (all but those on the rim of the grid)


def test_driver_generator_is_triclosest_with_one_radius():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    q, t = X.driver_triangles(lo, hi, 50, seed=5), T.driver_triangles(lo, hi, 50, seed=5)
    assert (q["max_dist2"] == 4).all() and all((words(q[k]) == words(t[k])).all() for k in ("a", "b", "c", "skip"))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Prox:
    """device buffers of one query set; count() / full() = one call each on caller-owned buffers, filled with poison before"""

    def __init__(self, ctx, drawer, queries, capacity=1):
        self.ctx, self.drawer, self.count_ = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, max(len(queries), 1), L().TRI_DISTANCE_QUERY)
        self.queries.local[:len(queries)] = queries
        self.queries.local[len(queries):]["max_dist2"] = 0
        self.queries.sync()
        self.offsets = H().DataBuffer(ctx, len(queries) + 1, np.uint64)
        self.records = H().DataBuffer(ctx, max(int(capacity), 1), L().TRI_CLOSEST)

    def count(self):
        self.offsets.fill_u32(POISON)
        self.drawer.triangle_gather_within_distance(self.queries, self.offsets)
        return self.offsets.get_data()[:self.count_ + 1].copy()

    def full(self):
        """-> (offsets, the WHOLE records buffer)"""
        self.offsets.fill_u32(POISON)
        self.records.fill_u32(POISON)
        self.drawer.triangle_gather_within_distance(self.queries, self.offsets, self.records)
        return self.offsets.get_data()[:self.count_ + 1].copy(), self.records.get_data().copy()

    def dispose(self):
        for b in (self.queries, self.offsets, self.records):
            b.dispose()


_REF = {}


def gpu_case(ctx, name):
    """(a, b, c, lo, hi, queries, reference with the library's boxes, drawer): the reference once per scene"""
    a, b, c, lo, hi, d = gpu_scene(ctx, name)
    if name not in _REF:
        q = proximity_queries(name, a, b, c)
        _REF[name] = (q, X.reference(q, a, b, c, lo, hi))
    return (a, b, c, lo, hi) + _REF[name] + (d,)


def run(ctx, d, queries, want_off, want_rec, what="", slack=5):
    """both forms of one set against an expected list; `slack` spare records must keep their poison -> (offsets, records)"""
    total = int(want_off[-1])
    p = Prox(ctx, d, queries, total + slack)
    try:
        only = p.count()
        off, rec = p.full()
    finally:
        p.dispose()
    assert (only == want_off).all(), (what, "count-only", np.nonzero(only != want_off)[0][:5])
    assert_lists(off, rec, want_off, want_rec, what)
    assert (words(rec[total:]) == POISON).all(), what
    return off, rec[:total]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_of_the_full_and_the_count_only_form(ctx, name):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, name)
    assert int(ref.offsets[-1]) >= 10000
    off, rec = run(ctx, d, queries, ref.offsets, ref.records, name)
    assert (rec["_zero"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t2_relations_a_to_d_on_the_device(ctx, name):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, name)
    total = int(ref.offsets[-1])
    p = Prox(ctx, d, queries, total)
    only = p.count()
    runs = [p.full() for _ in range(2)]
    assert (runs[0][0] == runs[1][0]).all() and (words(runs[0][1]) == words(runs[1][1])).all()    # two calls write the same bytes
    off, rec = runs[0]
    assert (only == off).all()                                                                  # (d)
    out = H().DataBuffer(ctx, COUNT, L().TRI_CLOSEST)
    flags = H().DataBuffer(ctx, COUNT, np.uint32)
    d.triangle_closest_points(p.queries, out)
    d.triangle_within_distance(p.queries, flags)
    tq = H().DataBuffer(ctx, COUNT, L().TRI_QUERY)
    tq.local[:] = tri_queries_of(queries)
    tq.sync()
    hit_off, hit_tris = d.intersections(tq)
    nonempty, listed = check_relations(queries, off, rec, flags.get_data()[:COUNT], out.get_data()[:COUNT], hit_off, hit_tris)
    print(f"{name}: {nonempty} non-empty segments, {listed} intersections listed at +0")
    assert nonempty >= 500 and listed >= 100
    for buf in (out, flags, tq):
        buf.dispose()
    p.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_t3_query_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    first = int(np.nonzero(np.diff(ref.offsets))[0][0])                 # (the single query is one with a list)
    rows = np.arange(first, first + count)
    run(ctx, d, queries[rows], *take(ref.offsets, ref.records, rows), count)


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t3_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 queries on 1, 2, 3 or 7 waves: runs of 1 500 .. 215, every lane refilled many times, lanes with lists of more than 64
    records beside lanes that take query after query"""
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:1500].copy()
    sub["b"][100:235, 0] = np.nan                                       # a block of inactive queries inside a run
    want = take(ref.offsets, ref.records, np.arange(1500), empty=range(100, 235))
    assert (np.diff(want[0]) > 64).sum() >= 100
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        run(ctx, d, sub, *want, waves)
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))


@pytest.mark.gpu
def test_t4_inactive_queries_among_active_ones(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub, places = spoiled(queries[:700])
    act = T.active(sub)
    assert (~act).sum() == len(places) and not act[places].any()
    want = take(ref.offsets, ref.records, np.arange(700), empty=places)
    # empty segments, complete offsets, the neighbours' segments what they were, poison beyond d_offsets[count] (run's slack)
    off, rec = run(ctx, d, sub, *want, "spoiled", slack=64)
    assert (np.diff(off)[places] == 0).all() and np.diff(off)[act].sum() == off[-1] > 0
    # an inactive query is never walked: the set of only them fetches no node
    idle = Prox(ctx, d, sub[~act], 8)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    stats.fill_u32(0)
    N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    try:
        only = idle.count()
        off, rec = idle.full()
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    st = stats.get_data()[0]
    assert (only == 0).all() and (off == 0).all() and (words(rec) == POISON).all()
    assert (st["rays"], st["node_fetches"], st["triangle_tests"]) == (0, 0, 0)
    stats.dispose()
    idle.dispose()


@pytest.mark.gpu
def test_t5_the_entry_contract_and_the_capacities():
    """the rows tests/test_query_entry_contract.py holds for the entry points it names, for this one, on a context of its own; then
    the capacities and one unbounded query"""
    tris, a, b, c, centre, queries = small_case()
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        ref = X.reference(queries, a, b, c, lo, hi)
        bf = X.brute_force(queries, a, b, c, lo, hi)
        assert (ref.offsets == bf.offsets).all() and (rw(ref.records) == rw(bf.records)).all()
        total = int(ref.offsets[-1])
        n = np.diff(ref.offsets).astype(np.int64)
        assert total >= 130 and (n == 0).any() and (n > 2).any()
        p = Prox(ctx, d, queries, total + 8)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        fn = getattr(lib, NAME)
        dq, do, dr = p.queries.device, p.offsets.device, p.records.device
        at = lambda buf, k: C.c_void_p(buf.device.value + k)
        st = np.zeros(130, dtype=L().PATH_STATE)
        st["origin"], st["dir"], st["alive"] = centre, (0.0, 0.0, -1.0), 1
        st["alive"][7::9] = 0
        states = H().DataBuffer(ctx, 130, L().PATH_STATE)
        states.local[:] = st
        states.sync()
        path_hits = H().DataBuffer(ctx, 130, L().HIT)

        def trace_rays():
            path_hits.fill_u32(POISON)
            N().check(h, lib.lbvh_trace_rays(h, states.device, 130, 0.0, C.byref(s), path_hits.device))
            return words(path_hits.get_data()).copy()
        expected_path = trace_rays()

        def poison():
            p.offsets.fill_u32(POISON)
            p.records.fill_u32(POISON)

        def untouched():
            return (words(p.offsets.get_data()) == POISON).all() and (words(p.records.get_data()) == POISON).all()

        def call(capacity):
            """the raw call with an explicit capacity on poisoned buffers -> (offsets, the whole records buffer)"""
            poison()
            assert fn(h, dq, 130, C.byref(s), do, dr if capacity else None, capacity) == 0
            return p.offsets.get_data()[:131].copy(), p.records.get_data().copy()

        poison()
        assert fn(h, dq, 0, C.byref(s), do, dr, total) == 0 and fn(h, None, 0, None, None, None, 0) == 0      # count == 0: a no-op
        assert untouched()                                                                    # d_offsets[0] included
        for args in ((None, 10, C.byref(s), do, dr, 8), (dq, 10, None, do, dr, 8), (dq, 10, C.byref(s), None, dr, 8),
                     (dq, 10, C.byref(s), do, None, 8),                                        # d_records == NULL with capacity > 0
                     (at(p.queries, 8), 10, C.byref(s), do, dr, 8), (at(p.queries, 4), 10, C.byref(s), do, dr, 8),
                     (dq, 10, C.byref(s), do, at(p.records, 8), 8), (dq, 10, C.byref(s), do, at(p.records, 4), 8),
                     (dq, 10, C.byref(s), at(p.offsets, 4), dr, 8), (dq, 1 << 32, C.byref(s), do, dr, 8)):
            assert fn(h, *args) == -1, args
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(NAME.encode() + b": ") and b"invalid argument" in msg, msg
        assert fn(None, dq, 10, C.byref(s), do, dr, 8) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        assert fn(h, dq, 130, C.byref(s), do, dr, total) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(NAME.encode() + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        assert (trace_rays() == expected_path).all()
        # each call drops the live-ray list the trace before it left: lbvh_trace_rays makes its own again
        for capacity in (0, total):
            off, rec = call(capacity)
            assert (off == ref.offsets).all()
            assert (trace_rays() == expected_path).all()
        # capacity = total exactly; NULL records with capacity 0 were the count-only form above
        off, rec = call(total)
        assert_lists(off, rec, ref.offsets, ref.records, "capacity = total")
        assert (words(rec[total:]) == POISON).all()
        # capacity = total - 1, and a capacity in the middle of a segment: nothing at or beyond it, complete offsets, every segment
        # that fits is the reference's
        k = int(np.nonzero(n > 2)[0][len(np.nonzero(n > 2)[0]) // 2])
        for capacity in (total - 1, int(ref.offsets[k]) + 1):
            off, rec = call(capacity)
            assert (off == ref.offsets).all() and (words(rec[capacity:]) == POISON).all(), capacity
            fits = np.nonzero(ref.offsets[1:] <= capacity)[0]
            assert 0 < len(fits) < 130
            got = take(off, rec, fits)
            assert_lists(got[0], X.by_tri(*got), *take(ref.offsets, ref.records, fits), capacity)
        # the plain and the counting instantiations write the same words; the poisoned stats block stays untouched with no target
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        stats.fill_u32(POISON)
        off, rec = call(total)
        assert (words(stats.get_data()) == POISON).all()
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            off2, rec2 = call(total)
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        assert (off2 == off).all() and (words(rec2) == words(rec)).all() and stats.get_data()[0]["rays"] == 2 * 130
        stats.dispose()
        p.dispose()
        # one unbounded query lists every triangle the accept rule admits: 64 minus `skip`
        one = queries[:1].copy()
        one["max_dist2"], one["skip"] = np.inf, 17
        want = X.brute_force(one, a, b, c, lo, hi)
        assert want.offsets.tolist() == [0, 63] and 17 not in want.records["tri"]
        run(ctx, d, one, want.offsets, want.records, "unbounded")
        for buf in (states, path_hits):
            buf.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t6_a_small_lds_stack_and_the_statistics(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))                   # the device-memory part of the stack: the same answers
    try:
        run(ctx, d, queries, ref.offsets, ref.records, "stack split 1")
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    total = int(ref.offsets[-1])
    p = Prox(ctx, d, queries, total)
    out = H().DataBuffer(ctx, COUNT, L().TRI_CLOSEST)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    seen = []
    try:
        for form in ("count", "full", "closest"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            if form == "count":
                assert (p.count() == ref.offsets).all()
            elif form == "full":
                assert_lists(*p.full(), ref.offsets, ref.records, "counting instantiations")
            else:
                d.triangle_closest_points(p.queries, out)
                out.get_data()
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("queries, node fetches, triangle lines: count-only %s, full %s, closest %s" % tuple(seen))
    assert seen[0][0] == COUNT and seen[1] == tuple(2 * x for x in seen[0])      # the same walk, the same decisions, twice
    assert seen[0][2] >= seen[2][2] > 0                                         # nothing shrinks here
    for buf in (out, stats):
        buf.dispose()
    p.dispose()


@pytest.mark.gpu
def test_t6_the_stack_limit_is_reported():
    """lbvh_debug_ray_stack_limit(1): a walk that needs more than one stack entry reports LBVH_FAULT_RAY_STACK (LBVH_ERR_HIP at the next
    sync), never a silently short list; with the limit lifted the lists are the reference's again.  On a context of its own."""
    tris, a, b, c, centre, queries = small_case()
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        d.build_fast_scene()
        ref = X.reference(queries, a, b, c, *library_boxes(d))
        p = Prox(ctx, d, queries, int(ref.offsets[-1]))
        h, lib = ctx.handle, N().lib
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        d.triangle_gather_within_distance(p.queries, p.offsets, p.records)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        p.dispose()
        run(ctx, d, queries, ref.offsets, ref.records, "after the limit")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pair", "triple", "one_cell", "copies", "outside", "fan"])
def test_t7_hostile_walk_shapes(ctx, name):
    """130 query triangles about the scene's vertices, a margin of 5 % of its extent, against the reference with the library's boxes.
    `slivers` is left out on purpose: its narrow phase on point and collinear triangles is the closest call's existing arithmetic."""
    tris = hostile_scenes.scene(name)
    a, b, c = positions(tris)
    ext = extent_of(a, b, c)
    rng = np.random.default_rng(77)
    pts = np.concatenate([a, b, c])
    centre = pts[rng.integers(0, len(pts), 130)] + (rng.normal(size=(130, 3)) * 0.02 * ext).astype(F)
    arms = (rng.normal(size=(3, 130, 3)) * 0.03 * ext).astype(F)
    margin = F(0.05 * ext)
    queries = T.make_queries(centre + arms[0], centre + arms[1], centre + arms[2], margin * margin)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    try:
        ref = X.reference(queries, a, b, c, *library_boxes(d))
        n = np.diff(ref.offsets).astype(np.int64)
        assert (n > 0).sum() >= 30, name
        off, rec = run(ctx, d, queries, ref.offsets, ref.records, name)
        if name == "copies":                                               # every listed triangle with all 8 of its stored indices
            group = hostile_scenes.copies_groups()
            for k in np.nonzero(n)[0]:
                per = np.bincount(group[rec["tri"][int(off[k]):int(off[k + 1])]], minlength=40)
                assert set(per.tolist()) <= {0, 8}, k
    finally:
        d.on_destroy()


@pytest.mark.gpu
def test_t8_proximity_pairs_of_a_tilted_fan_above_a_floor(ctx):
    """the floor and the fan of test_t7_mesh_distance_of_a_tilted_fan_above_a_floor.  The apex (1, 2, 0.75) is the nearest point of every
    fan triangle and lies above floor triangle 1 (y > x), 0.75 from it: dist2 = 0.5625 for all four.  Floor triangle 0 begins at the
    diagonal y = x, 1 / sqrt(2) to the side of the apex, and the fan rises towards it: its distances are 1.0416667, 1.0625, 0.8888889
    and 0.8888889 squared (the fp32 reference; e.g. the edge apex - (1, 0, 1.25) crosses the diagonal at the height 1, and the rim
    (3, 2, 1.75) - apex at the height 1.25, both a little farther than the nearest point of the face).  So a margin of 0.76 lists
    triangle 1 alone for all four, a margin of 1.1 lists both, triangle 1 first in (dist2, tri) order, and 0.75 lists nothing."""
    w = 20.0
    pos = np.array([((-w, -w, 0), (w, -w, 0), (w, w, 0)), ((-w, -w, 0), (w, w, 0), (-w, w, 0))], dtype=F)
    d = H().RaytracingMeshDrawer(ctx, pack(pos[:, 0], pos[:, 1], pos[:, 2])).awake()
    d.build_fast_scene()
    apex = np.array([1, 2, 0.75], dtype=F)
    rim = np.array([(3, 2, 1.75), (1, 4, 2.25), (-1, 2, 2.75), (1, 0, 1.25), (3, 2, 1.75)], dtype=F)
    fan = (rim[:4], np.tile(apex, (4, 1)), rim[1:])
    off, rec = d.proximity_pairs(fan, 0.76, sort=True)
    assert off.tolist() == [0, 1, 2, 3, 4] and rec["tri"].tolist() == [1] * 4 and (rec["dist2"] == F(0.5625)).all()
    off, rec = d.proximity_pairs(fan, 1.1, sort=True)
    assert off.tolist() == [0, 2, 4, 6, 8] and rec["tri"].tolist() == [1, 0] * 4 and (rec["dist2"][0::2] == F(0.5625)).all()
    want = X.reference(H().tri_distance_queries_from_mesh(fan, F(1.1) * F(1.1)), pos[:, 0], pos[:, 1], pos[:, 2], *library_boxes(d))
    assert_lists(off, rec, want.offsets, want.records, "fan")
    assert np.abs(want.records["dist2"][0::2] - np.array([25 / 24, 17 / 16, 8 / 9, 8 / 9])).max() < 1e-6
    off, rec = d.proximity_pairs(pack(*fan), 0.75)                          # the radius is open; layouts.TRIANGLE is taken the same way
    assert off.tolist() == [0] * 5 and len(rec) == 0
    q = H().tri_distance_queries_from_mesh(fan, F(0.76) * F(0.76))
    off, rec = d.proximity_pairs(q, None)                                   # layouts.TRI_DISTANCE_QUERY records are taken as they are
    assert off.tolist() == [0, 1, 2, 3, 4]
    assert d.proximity_pairs(q[:0], None)[0].tolist() == [0]
    d.on_destroy()


@pytest.mark.gpu
def test_t8_a_self_pass_on_the_grid_has_no_pair_below_one_cell(ctx):
    """self_skip=True on the 80 x 80 grid with a margin below one cell: every triangle lists its neighbours, all of which share a vertex
    with it, so unique_self_pairs keeps nothing; sort=True orders every segment by (dist2, tri)"""
    a, b, c, lo, hi, d = gpu_scene(ctx, "grid_80x80")
    v = np.stack([a, b, c], axis=1).astype(np.float64)
    cell = float(np.abs(v[:, 1, :2] - v[:, 0, :2]).max(axis=1).min())
    assert cell > 0
    off, rec = d.proximity_pairs((a, b, c), 0.45 * cell, self_skip=True, sort=True)
    n = np.diff(off).astype(np.int64)
    assert len(off) == len(a) + 1 and n.min() >= 3 and len(rec) == off[-1]
    segment = np.repeat(np.arange(len(a)), n)
    assert (rec["tri"] != segment).all()
    key = np.lexsort((rec["tri"], rec["dist2"], segment))
    assert (key == np.arange(len(rec))).all()
    pairs, kept = H().unique_self_pairs(off, rec, (a, b, c))
    assert pairs.shape == (0, 2) and len(kept) == 0


@pytest.mark.gpu
def test_t8_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver triprox 2000 21`: TriangleGatherWithinDistance of lbvh_host.hpp on the driver's own mesh and queries, against the
    reference on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "triprox", str(count), "21"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    boxes = library_boxes(d)
    d.on_destroy()
    r = X.reference(X.driver_triangles(lo, hi, count, seed=21), a, b, c, *boxes)
    n = np.diff(r.offsets).astype(np.int64)
    total = int(r.offsets[-1])
    assert total > 100 and 100 < (n > 0).sum() < count
    weigh = (rw(r.records).astype(np.uint64) * np.arange(1, 9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert (res["triangles"], res["queries"], res["total"], res["nonempty"], res["longest"]) == (4096, count, total, int((n > 0).sum()), int(n.max()))
    assert res["pierced"] == int((r.records["edge"] & 8 != 0).sum())
    assert res["word_sum"] == int((weigh * np.arange(1, total + 1, dtype=np.uint64)).sum(dtype=np.uint64))
