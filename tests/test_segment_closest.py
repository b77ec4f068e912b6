"""lbvh_segment_closest_point / lbvh_segment_within_distance: how far a segment (a capsule's axis) is from the mesh, where and in
which direction, as the nearest 32-byte record per segment and as one flag per segment, over the four-wide derived traversal scene.
The expectation is tests/segment_closest_reference.py: the header's definition in numpy float32 — no tree.
  CPU  the surface in every host; hand-made pairs with answers derivable on paper; the reference against the test of every pair;
       the reference against float64 geometry that shares no line with it; relations (b) and (c) in the reference; the parity sets
       are not vacuous
  T1   parity of both calls on grid_80x80 and cfg1_4096        T2  relations (a), (b) and (c) on the device
  T3   query counts around a wave; wave caps (the lane refill)  T4  inactive queries; every output word is written
  T5   count == 0, every rejection, a stale scene, the live-path list (the contract tests/test_query_entry_contract.py asserts for
       the entry points it names, for these two)
  T6   a small LDS stack; statistics against lbvh_capsule_deepest
  T7   .clearance on a capsule above a floor; lbvh_driver segclosest: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import contact_reference as K
import point_reference as P
import segment_closest_reference as G
import shape_overlap_reference as S
from query_support import driver_mesh, H, L, library_boxes, make_queries, N, pack, padded_boxes, positions, words
from test_shape_contacts import contact_shapes, nearest_pair64
from test_shape_overlaps import extent_of, K_EPS, PARITY, scene
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNT = 2000
NAMES = ("lbvh_segment_closest_point", "lbvh_segment_within_distance")
NONE_WORDS = [int(words(np.array([G.MAX_FLOAT], dtype=F))[0]), 0, 0, 0, 0, 0, 0, 0]


def rw(records):
    """layouts.SEGMENT_CLOSEST records -> (rows, 8) words"""
    return words(records).reshape(-1, 8)


def parity_queries(a, b, c, count=COUNT, seed=17):
    """-> (queries, r): the segments of test_shape_contacts.contact_shapes — its placement, its one-in-sixteen axis = 0 and its
    one-in-sixteen ten extents away —, every even one stretched about its middle to 10 .. 30 % of the extent (a segment as long as
    a few triangles has a nearest triangle that neither end has: test_the_parity_sets_are_not_vacuous), with a search radius r of
    0.5 .. 5 % of the extent, max_dist2 = r*r, for half of them and an unbounded search (r = +inf) for the others."""
    caps = contact_shapes(a, b, c, count=count, seed=seed)
    ext = extent_of(a, b, c)
    rng = np.random.default_rng(seed + 2000 + len(a))
    origin, axis = caps["origin"].copy(), caps["axis"].copy()
    i = np.arange(count)
    length = np.linalg.norm(axis.astype(np.float64), axis=1)
    stretch = (i % 2 == 0) & (length > 0)
    mid = origin.astype(np.float64) + 0.5 * axis
    longer = axis * (ext * rng.uniform(0.1, 0.3, count) / np.where(length > 0, length, 1.0))[:, None]
    axis[stretch] = longer[stretch].astype(F)
    origin[stretch] = (mid[stretch] - 0.5 * axis[stretch]).astype(F)
    r = (ext * rng.uniform(0.005, 0.05, count)).astype(F)
    r = np.where(rng.random(count) < 0.5, r, F(np.inf)).astype(F)
    return G.make_queries(origin, axis, r * r), r


_CPU = {}


def cpu_case(name):
    """(a, b, c, box_lo, box_hi, queries, r, reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        lo, hi = padded_boxes(a, b, c)
        q, r = parity_queries(a, b, c)
        _CPU[name] = (a, b, c, lo, hi, q, r, G.reference(q, a, b, c, lo, hi))
    return _CPU[name]


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_records_and_the_two_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_segment_query \{\s+float origin\[3\]; float max_dist2;[^}]*?float axis\[3\];\s+uint32_t _pad;[^}]*?\} lbvh_segment_query;", h)
    assert re.search(r"typedef struct lbvh_segment_closest \{\s+float\s+dist2;[^}]*?uint32_t tri;[^}]*?float\s+u, v;[^}]*?float\s+delta\[3\];[^}]*?float\s+s;[^}]*?\} lbvh_segment_closest;", h)
    assert re.search(r"lbvh_status lbvh_segment_closest_point\(lbvh_context\* ctx, const lbvh_segment_query\* d_queries, size_t count, const lbvh_scene\* h_scene,"
                     r"\s+lbvh_segment_closest\* d_out\);", h)
    assert re.search(r"lbvh_status lbvh_segment_within_distance\(lbvh_context\* ctx, const lbvh_segment_query\* d_queries, size_t count, const lbvh_scene\* h_scene,"
                     r"\s+uint32_t\* d_flags\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert all(n in bounce for n in NAMES)
    text = h[h.index("Segment closest-point queries: HOW FAR"):h.index("lbvh_status lbvh_segment_closest_point(")]
    for must in ("Pierce first", "strictly", "dist2 = +0", "lo_k - max(h_k, 0)", "hi_k - min(h_k, 0)", "the lower original triangle index",
                 "!(dist2_i < box2g(own AABB_i))", "box2g(ancestor) <= box2g(leaf) <= dist2", "(a) the flag is 1 exactly when",
                 "axis = (+0, +0, +0)", "depth == r - sqrtf(dist2)", "NOT promised", "Out of scope: the k nearest", "a unit\n * normal in the record"):
        assert must in text, must


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    for n in NAMES:
        res, args = nat.SIGNATURES[n]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
    assert all(hasattr(nat.lib, n) for n in NAMES)
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.SEGMENT_QUERY.itemsize == 32 and lay.SEGMENT_CLOSEST.itemsize == 32
    assert [lay.SEGMENT_CLOSEST.fields[f][1] for f in ("dist2", "tri", "u", "v", "delta", "s")] == [0, 4, 8, 12, 16, 28]
    assert [lay.SEGMENT_QUERY.fields[f][1] for f in ("origin", "max_dist2", "axis", "_pad")] == [0, 12, 16, 28]
    assert rw(np.array([G.NONE])).tolist() == [NONE_WORDS]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_segment_closest_point\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    assert re.search(r"public static extern int lbvh_segment_within_distance\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    assert "public struct SegmentQuery " in cs and "public struct SegmentClosest " in cs
    sq = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "SegmentQueries.cs")).read())
    assert all(n in sq for n in NAMES) and "unsafe" not in sq
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert all(f"void {m}(" in hpp for m in ("SegmentClosestPoints", "SegmentWithinDistance"))
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"segclosest", segclosest_main}' in drv and "lbvh_driver segclosest <n_segments> [seed]" in drv
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("segment_closest_points", "segment_within_distance", "clearance")) and callable(H().segment_queries)
    q = H().segment_queries([[1, 2, 3]], [0, 0, 1], 4.0)
    assert q.dtype == lay.SEGMENT_QUERY and q["origin"].tolist() == [[1, 2, 3]] and q["axis"].tolist() == [[0, 0, 1]] and q["max_dist2"][0] == 4


# ---- CPU: the restatement on pairs with answers derivable on paper -----------------------------------------------------------

TRI = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


def one_pair(origin, axis, max_dist2=np.inf, tri=TRI):
    """-> the record of one segment and one scene triangle, with `which` (-1: none)"""
    t = np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    q = G.make_queries(np.array([origin], dtype=F), np.array([axis], dtype=F), F(max_dist2))
    r = G.reference(q, a, b, c, *padded_boxes(a, b, c))
    assert rw(r.records).tolist() == rw(G.brute_force(q, a, b, c, *padded_boxes(a, b, c))).tolist()
    assert int(r.flags[0]) == int(r.which[0] >= 0)
    return r.records[0], int(r.which[0])


def test_reference_a_segment_above_the_face():
    # parallel to the face at the height z: every point is equally near; the order rule takes j = 0, so s = 0
    k, which = one_pair((1, 1, 0.75), (1, 0.5, 0))
    assert which == 0 and k["dist2"] == 0.5625 and k["s"] == 0 and k["delta"].tolist() == [0, 0, 0.75] and (k["u"], k["v"]) == (0.25, 0.25)
    # sloping away: the lower end is the nearest point, whichever end it is
    k, which = one_pair((1, 1, 0.5), (1, 0.5, 2))
    assert which == 0 and k["dist2"] == 0.25 and k["s"] == 0 and k["delta"].tolist() == [0, 0, 0.5]
    k, which = one_pair((2, 1.5, 2.5), (-1, -0.5, -2))
    assert which == 1 and k["dist2"] == 0.25 and k["s"] == 1 and k["delta"].tolist() == [0, 0, 0.5] and (k["u"], k["v"]) == (0.25, 0.25)
    # the search radius is open: dist2 == max_dist2 is none
    assert one_pair((1, 1, 0.5), (1, 0.5, 2), 0.25)[1] == -1 and one_pair((1, 1, 0.5), (1, 0.5, 2), 0.2500001)[1] == 0


def test_reference_a_segment_beside_an_edge():
    # a vertical segment 0.25 outside the edge y = 0 (z from -1 to 1): the interior of the segment against the interior of the edge
    k, which = one_pair((2, -0.25, -1), (0, 0, 2))
    assert which in (2, 3) and k["s"] == 0.5 and k["dist2"] == 0.0625 and k["delta"].tolist() == [0, -0.25, 0] and (k["u"], k["v"]) == (0.5, 0)
    # outside the edge x = 0 (the side C-A: j = 6 or 7), pointing down
    k, which = one_pair((-0.125, 1, 3), (0, 0, -4))
    assert which in (6, 7) and k["s"] == 0.75 and k["dist2"] == 0.015625 and k["delta"].tolist() == [-0.125, 0, 0] and (k["u"], k["v"]) == (0, 0.25)


def test_reference_a_segment_beyond_a_vertex():
    # pointing away from the vertex (0, 0, 0) along (-3, -4, 0), the near end 0.25 away; either end first
    k, which = one_pair((-0.15, -0.2, 0), (-3, -4, 0))
    assert k["s"] == 0 and (k["u"], k["v"]) == (0, 0) and abs(float(k["dist2"]) - 0.0625) < 1e-7
    assert np.allclose(k["delta"], (-0.15, -0.2, 0), atol=1e-7)
    k, which = one_pair((-3.15, -4.2, 0), (3, 4, 0))
    assert which == 1 and k["s"] == 1 and (k["u"], k["v"]) == (0, 0) and abs(float(k["dist2"]) - 0.0625) < 1e-6


def test_reference_a_segment_parallel_to_an_edge():
    # along the edge y = 0 at the distance 0.5 outside it, in the plane: a continuum of nearest pairs; the definition names one
    k, which = one_pair((1, -0.5, 0), (2, 0, 0))
    assert k["dist2"] == 0.25 and k["delta"].tolist() == [0, -0.5, 0] and 0 <= k["s"] <= 1 and k["v"] == 0
    assert k["u"] == (F(1) + F(2) * k["s"]) / F(4)
    # and lifted off the plane
    k, which = one_pair((1, -0.5, 0.5), (2, 0, 0))
    assert k["dist2"] == 0.5 and k["delta"].tolist() == [0, -0.5, 0.5]


def test_reference_a_segment_that_pierces_the_face():
    # through the face at (1, 1), z from -1 to 3: dist2 = +0, s = t_p = 0.25, delta = 0
    k, which = one_pair((1, 1, -1), (0, 0, 4))
    assert which == G.PIERCE and rw(np.array([k]))[0].tolist()[:2] == [0, 0] and k["s"] == 0.25 and (k["u"], k["v"]) == (0.25, 0.25)
    assert words(k["delta"]).tolist() == [0, 0, 0]
    k, which = one_pair((1, 1, 3), (0, 0, -4), 1e-30)                  # any positive radius finds a pierced triangle
    assert which == G.PIERCE and k["s"] == 0.75 and k["dist2"] == 0
    # an end ON the face without a pierce that passes (t_p = 0 passes; the end beyond does not): dist2 == 0 either way
    k, which = one_pair((1, 1, 0), (0, 0, 2))
    assert k["dist2"] == 0 and k["s"] == 0 and (k["u"], k["v"]) == (0.25, 0.25)


def test_reference_axis_zero_is_the_point_query():
    rng = np.random.default_rng(3)
    t = np.array(TRI, dtype=F)
    for p in rng.uniform(-1, 5, (40, 3)).astype(F) * np.array([1, 1, 0.1], dtype=F):
        d2, u, v = P.point_triangle(p[None], t[None, 0], (t[1] - t[0])[None], (t[2] - t[0])[None])
        k, which = one_pair(p, (0, 0, 0))
        assert which != G.PIERCE and 0 <= k["s"] <= 1
        assert (words(k["dist2"]), words(k["u"]), words(k["v"])) == (words(d2[0]), words(u[0]), words(v[0]))


def test_reference_inactive_queries_have_nothing():
    t = np.array(TRI, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    q = G.make_queries(np.tile(np.array([[1, 1, 0.5]], dtype=F), (7, 1)), np.tile(np.array([[0, 0, 1]], dtype=F), (7, 1)), F(np.inf))
    q["max_dist2"][1:4] = (0, -1, np.nan)
    q["origin"][4, 1] = np.nan
    q["axis"][5, 2] = np.inf
    q["axis"][6, 0] = np.nan
    assert G.active(q).tolist() == [True] + [False] * 6
    r = G.reference(q, a, b, c, *padded_boxes(a, b, c))
    assert r.flags.tolist() == [1, 0, 0, 0, 0, 0, 0] and (rw(r.records[1:]) == NONE_WORDS).all()


# ---- CPU: the reference and the test of every pair; float64; the relations; the sets ------------------------------------------

def test_the_reference_is_the_test_of_every_pair():
    """segment_closest_reference.reference leaves out the narrow phase of the pairs the candidate rule itself excludes; on the first 48
    queries of each parity set (a tenth of a second per query and scene) the record is the one the nine tests of EVERY pair give"""
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        assert (rw(G.brute_force(q[:48], a, b, c, lo, hi)) == rw(ref.records[:48])).all()
        assert ref.tested < 0.01 * COUNT * len(a)


def test_reference_agrees_with_an_independent_float64_evaluation():
    """Every record of the parity sets against the float64 segment-triangle geometry of tests/test_shape_contacts.py (nearest_pair64),
    with band = K_EPS * 2^-24 * extent, the band that file holds the same arithmetic to (DESIGN sections 34 and 35).  The extent is
    that of what the arithmetic sees, the mesh AND the segment: there no shape ten extents away touches anything, here an unbounded
    search from there has a record, formed from coordinates and differences ten times as large (for a segment inside the mesh's box
    it is the mesh's extent).
      per pair    |sqrt(dist2) - dist64(segment, winning triangle)| <= band; where float64 says the segment crosses the triangle and
                  fp32 does not (or the other way round: within the band of an edge), sqrt(dist2) <= band all the same
      the winner  on the first 64 queries of each set: no triangle is nearer in float64 than sqrt(dist2) - band, and where the
                  record is none, none is nearer than sqrt(R) - band
      delta       |delta - (x(s) - y(u, v))| <= band where the pierce did not give the record (s, u, v against float64 points are
                  test_shape_contacts' business: relation (c) makes them the same words)."""
    eps = 2.0 ** -24
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        pts = np.concatenate([a, b, c]).astype(np.float64)
        ends = np.stack([q["origin"].astype(np.float64), q["origin"].astype(np.float64) + q["axis"]])
        reach = (np.maximum(pts.max(axis=0), ends.max(axis=0)) - np.minimum(pts.min(axis=0), ends.min(axis=0))).max(axis=1)
        assert (reach >= extent_of(a, b, c)).all() and np.median(reach) <= 1.3 * extent_of(a, b, c)
        band_of = K_EPS * eps * reach
        found = np.nonzero(ref.flags == 1)[0]
        band = band_of[found]
        rec = ref.records[found]
        tri = rec["tri"].astype(np.int64)
        o, h = q["origin"][found].astype(np.float64), q["axis"][found].astype(np.float64)
        a64, b64, c64 = (x[tri].astype(np.float64) for x in (a, b, c))
        dist, _, _, crosses, _ = nearest_pair64(o, h, a64, b64, c64)
        got = np.sqrt(rec["dist2"].astype(np.float64))
        err = np.abs(got - dist)
        print(f"{name}: {len(found)} records, {int(crosses.sum())} cross in float64, {int((ref.which[found] == G.PIERCE).sum())} pierce in fp32, "
              f"distance error <= {(err / band).max():.3f} band")
        assert (err <= band).all(), (name, found[err > band][:5], (err / band).max())
        e1, e2 = (b - a)[tri].astype(np.float64), (c - a)[tri].astype(np.float64)
        x = o + h * rec["s"].astype(np.float64)[:, None]
        y = a64 + e1 * rec["u"].astype(np.float64)[:, None] + e2 * rec["v"].astype(np.float64)[:, None]
        plain = ref.which[found] != G.PIERCE
        assert (np.linalg.norm(rec["delta"].astype(np.float64) - (x - y), axis=1)[plain] <= band[plain]).all()
        # the winner among all triangles, float64, on the first 64 queries
        first = np.nonzero(G.active(q))[0][:64]
        rows, every = (v.reshape(-1) for v in np.meshgrid(first, np.arange(len(a)), indexing="ij"))
        d_all = nearest_pair64(q["origin"][rows].astype(np.float64), q["axis"][rows].astype(np.float64),
                               *(v[every].astype(np.float64) for v in (a, b, c)))[0].reshape(len(first), len(a))
        bound = np.where(ref.flags[first] == 1, np.sqrt(ref.records["dist2"][first].astype(np.float64)),
                         np.sqrt(G.radius2(q)[first].astype(np.float64)))
        assert (d_all.min(axis=1) >= bound - band_of[first]).all(), name


def test_relation_b_in_the_reference():
    """axis = (+0, +0, +0), the same point and max_dist2: the first four words are lbvh_closest_point_query's"""
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        z = q.copy()
        z["axis"] = 0
        z["origin"][1::2] += z["axis"][1::2]                               # (the far ends too)
        got = G.reference(z, a, b, c, lo, hi)
        want = P.reference(make_queries(z["origin"], z["max_dist2"]), a, b, c, lo, hi)
        assert (rw(got.records)[:, :4] == words(want.records).reshape(-1, 4)).all()
        assert (got.flags == want.flags).all() and int(got.flags.sum()) > COUNT // 4 and (got.which != G.PIERCE).all()
        assert (words(got.records["delta"])[got.flags == 0] == 0).all()


def capsules_of(q, r):
    return S.make_capsules(q["origin"], q["axis"], r)


def check_relation_c(q, r, records, offsets, contacts):
    """records: SEGMENT_CLOSEST per query; (offsets, contacts): lbvh_capsule_contacts of the capsules {origin, r, axis}.  -> how many
    winners the capsule lists, how many of those are no face contacts"""
    listed = plain = 0
    with np.errstate(all="ignore"):
        for k in np.nonzero((records["dist2"] != G.MAX_FLOAT) & np.isfinite(r))[0]:
            seg = contacts[int(offsets[k]):int(offsets[k + 1])]
            at = np.nonzero(seg["tri"] == records["tri"][k])[0]
            if len(at) == 0:
                continue
            con, rec = seg[at[0]], records[k]
            listed += 1
            assert (words(con["s"]), words(con["u"]), words(con["v"])) == (words(rec["s"]), words(rec["u"]), words(rec["v"])), k
            if rec["dist2"] > 0:                                           # not a face contact: neither pierced nor on the triangle
                plain += 1
                dist = np.sqrt(rec["dist2"])
                assert words(con["depth"]) == words(F(r[k] - dist)), k
                assert words(con["normal"]).tolist() == words((rec["delta"] / dist).astype(F)).tolist(), k
    return listed, plain


def test_relation_c_in_the_reference():
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        con = K.reference(capsules_of(q, r), a, b, c, lo, hi)
        listed, plain = check_relation_c(q, r, ref.records, con.offsets, con.contacts)
        print(f"{name}: {listed} winners listed by the capsule of the search radius, {plain} of them no face contacts")
        assert listed >= 200 and plain >= 100


def test_the_parity_sets_are_not_vacuous():
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        act = G.active(q)
        found = ref.flags == 1
        ends = [P.reference(make_queries(p, q["max_dist2"]), a, b, c, lo, hi) for p in (q["origin"], q["origin"] + q["axis"])]
        same = [(e.flags == 1) & (e.records["tri"] == ref.records["tri"]) for e in ends]
        other = found & ~same[0] & ~same[1]
        by_j = np.bincount(ref.which[found], minlength=9)
        print(f"{name}: {int(act.sum())} active, {int(found.sum())} with a record, {int(other.sum())} whose winner neither end has "
              f"({other.sum() / act.sum():.3f}), winning j {by_j[:8].tolist()}, pierce {int(by_j[8])}, {ref.tested} pairs tested")
        assert len(q) == COUNT and act.all() and other.sum() >= act.sum() / 4
        assert by_j[0] > 0 and by_j[1] > 0 and by_j[2:8].sum() > 0 and by_j[8] >= 20
        i = np.arange(COUNT)
        assert (q["axis"] == 0).all(axis=1).sum() == COUNT // 16 and found[(q["axis"] == 0).all(axis=1)].any()
        assert np.isinf(q["max_dist2"]).sum() > COUNT // 4 and (~np.isinf(q["max_dist2"])).sum() > COUNT // 4
        assert (~found[(i % 16 == 13) & ~np.isinf(q["max_dist2"])]).all() and (~found).sum() > 50 and found[i % 16 == 13].any()


def test_driver_generator_is_deterministic_and_inside_the_box():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    q, q2 = G.driver_segments(lo, hi, 50, seed=5), G.driver_segments(lo, hi, 50, seed=5)
    assert (words(q) == words(q2)).all() and (q["origin"] >= lo).all() and (q["origin"] <= hi).all()
    assert (np.abs(q["axis"]) <= 6).all() and (q["max_dist2"][0::2] == 9).all() and np.isinf(q["max_dist2"][1::2]).all() and G.active(q).all()
    assert (words(q) != words(G.driver_segments(lo, hi, 50, seed=6))).any()
    caps = K.driver_capsules(lo, hi, 50, seed=5)                           # the same draws as `lbvh_driver contacts`
    assert (words(q["origin"]) == words(caps["origin"])).all() and (words(q["axis"]) == words(caps["axis"])).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Segs:
    """device buffers of one query set; closest() / within() = one call each on caller-owned buffers"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer, self.count = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, max(len(queries), 1), L().SEGMENT_QUERY)
        self.queries.local[:len(queries)] = queries
        self.queries.sync()
        self.out = H().DataBuffer(ctx, max(len(queries), 1), L().SEGMENT_CLOSEST)
        self.flags = H().DataBuffer(ctx, max(len(queries), 1), np.uint32)

    def closest(self):
        self.out.fill_u32(0xDEADBEEF)
        self.drawer.segment_closest_points(self.queries, self.out)
        return self.out.get_data()[:self.count].copy()

    def within(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.segment_within_distance(self.queries, self.flags)
        return self.flags.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.queries, self.out, self.flags):
            b.dispose()


def assert_equal(got, flags, ref, what=""):
    bad = np.nonzero((rw(got) != rw(ref.records)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], ref.records[bad[:5]])
    assert (flags == ref.flags).all(), (what, np.nonzero(flags != ref.flags)[0][:10])


_GPU = {}


def gpu_scene(ctx, name):
    """(a, b, c, lo, hi, drawer): one drawer per scene; a context keeps one derived traversal scene, so it is derived again for the
    test that asks"""
    if name not in _GPU:
        tris = scene(name)
        a, b, c = positions(tris)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        _GPU[name] = (a, b, c, *library_boxes(d), d)
    _GPU[name][-1].build_fast_scene()
    return _GPU[name]


def gpu_case(ctx, name):
    """(a, b, c, lo, hi, queries, r, reference with the library's boxes, drawer): the reference once per scene"""
    a, b, c, lo, hi, d = gpu_scene(ctx, name)
    if ("ref", name) not in _GPU:
        q, r = parity_queries(a, b, c)
        _GPU["ref", name] = (q, r, G.reference(q, a, b, c, lo, hi))
    return (a, b, c, lo, hi) + _GPU["ref", name] + (d,)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, name)
    assert int(ref.flags.sum()) >= 1000
    q = Segs(ctx, d, queries)
    assert_equal(q.closest(), q.within(), ref)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t2_relations_a_b_and_c_on_the_device(ctx, name):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, name)
    q = Segs(ctx, d, queries)
    runs = [(words(q.closest()).copy(), q.within()) for _ in range(2)]
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all()       # two calls write the same bytes
    got, flags = q.closest(), q.within()
    assert ((got["dist2"] != G.MAX_FLOAT) == (flags == 1)).all() and set(flags.tolist()) == {0, 1}          # (a)
    q.dispose()
    # (b): axis = +0, at both ends of the segments, against lbvh_closest_point_query on the device
    z = queries.copy()
    z["origin"][1::2] += z["axis"][1::2]
    z["axis"] = 0
    zq = Segs(ctx, d, z)
    points = H().DataBuffer(ctx, COUNT, L().POINT_QUERY)
    points.local[:] = make_queries(z["origin"], z["max_dist2"])
    points.sync()
    nearest = H().DataBuffer(ctx, COUNT, L().CLOSEST_POINT)
    within = H().DataBuffer(ctx, COUNT, np.uint32)
    d.closest_points(points, nearest)
    d.within_distance(points, within)
    zero = zq.closest()
    assert (rw(zero)[:, :4] == words(nearest.get_data()).reshape(-1, 4)).all() and (zq.within() == within.get_data()).all()
    assert int((zero["dist2"] != G.MAX_FLOAT).sum()) > COUNT // 4
    for buf in (points, nearest, within):
        buf.dispose()
    zq.dispose()
    # (c): lbvh_capsule_contacts with r = the search radius
    shapes = H().DataBuffer(ctx, COUNT, L().CAPSULE)
    shapes.local[:] = capsules_of(queries, r)
    shapes.sync()
    off, recs = d.contacts(shapes)
    listed, plain = check_relation_c(queries, r, got, off, recs)
    print(f"{name}: {listed} winners listed by the capsule of the search radius, {plain} of them no face contacts")
    assert listed >= 200 and plain >= 100
    shapes.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_t3_query_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    first = int(np.nonzero(ref.flags)[0][0])                           # (the single query is one with a record)
    sub = queries[first:first + count]
    want = G.Result(ref.records[first:first + count], ref.flags[first:first + count], None, 0, 0)
    q = Segs(ctx, d, sub)
    assert_equal(q.closest(), q.within(), want, count)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t3_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 queries on 1, 2, 3 or 7 waves: runs of 1 500 .. 215, every lane refilled many times"""
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:1500].copy()
    sub["origin"][100:235, 0] = np.nan                                  # a block of inactive queries inside a run
    want = G.Result(ref.records[:1500].copy(), ref.flags[:1500].copy(), None, 0, 0)
    want.records[100:235] = G.NONE
    want.flags[100:235] = 0
    q = Segs(ctx, d, sub)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        got, flags = q.closest(), q.within()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal(got, flags, want, waves)
    q.dispose()


def spoiled(queries):
    """a copy with every way of being inactive, ten of each -> (queries, their places)"""
    sub = queries.copy()
    places = np.arange(50) * 13 + 7
    sub["origin"][places[0:10], np.arange(10) % 3] = np.nan
    sub["axis"][places[10:20], np.arange(10) % 3] = np.where(np.arange(10) % 2, np.inf, -np.inf).astype(F)
    sub["axis"][places[15:20], 0] = np.nan
    sub["max_dist2"][places[20:30]] = 0
    sub["max_dist2"][places[25:30]] = -0.0
    sub["max_dist2"][places[30:40]] = np.where(np.arange(10) % 2, -1.0, -np.inf).astype(F)
    sub["max_dist2"][places[40:50]] = np.nan
    return sub, places


@pytest.mark.gpu
def test_t4_inactive_queries_among_active_ones(ctx):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    sub, places = spoiled(queries[:700])
    act = G.active(sub)
    assert (~act).sum() == len(places) and not act[places].any()
    q = Segs(ctx, d, sub)
    got, flags = q.closest(), q.within()                                # (both buffers were filled with 0xDEADBEEF)
    assert (rw(got[~act]) == NONE_WORDS).all() and (flags[~act] == 0).all()
    # the neighbours are what they were in the full set: every output word is written, and none of another query
    assert (rw(got[act]) == rw(ref.records[:700][act])).all() and (flags[act] == ref.flags[:700][act]).all() and flags[act].sum() > 0
    q.dispose()
    # an inactive query is never walked: the set of only them fetches no node
    idle = Segs(ctx, d, sub[~act])
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    stats.fill_u32(0)
    N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    try:
        got, flags = idle.closest(), idle.within()
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    st = stats.get_data()[0]
    assert (rw(got) == NONE_WORDS).all() and (flags == 0).all()
    assert (st["rays"], st["node_fetches"], st["triangle_tests"]) == (0, 0, 0)
    stats.dispose()
    idle.dispose()


@pytest.mark.gpu
def test_t5_count_zero_rejections_a_stale_scene_and_the_live_path_list():
    """the rows tests/test_query_entry_contract.py has for the entry points it names, for these two: on a context of its own"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        centre = a[rng.integers(0, 64, 130)] + rng.normal(size=(130, 3)).astype(F) * F(2)
        queries = G.make_queries(centre, rng.normal(size=(130, 3)).astype(F), F(0.49))
        ref = G.reference(queries, a, b, c, lo, hi)
        assert (rw(ref.records) == rw(G.brute_force(queries, a, b, c, lo, hi))).all() and 0 < ref.flags.sum() < 130
        q = Segs(ctx, d, queries)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        one, any_ = lib.lbvh_segment_closest_point, lib.lbvh_segment_within_distance
        dq, do, df = q.queries.device, q.out.device, q.flags.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.out, q.flags)
        # what lbvh_trace_rays answers before any query has run: it leaves a live-ray list behind
        st = np.zeros(130, dtype=L().PATH_STATE)
        st["origin"], st["dir"], st["alive"] = centre, (0.0, 0.0, -1.0), 1
        st["alive"][7::9] = 0
        states = H().DataBuffer(ctx, 130, L().PATH_STATE)
        states.local[:] = st
        states.sync()
        path_hits = H().DataBuffer(ctx, 130, L().HIT)

        def trace_rays():
            path_hits.fill_u32(0x7FC0DEAD)
            N().check(h, lib.lbvh_trace_rays(h, states.device, 130, 0.0, C.byref(s), path_hits.device))
            return words(path_hits.get_data()).copy()
        expected_path = trace_rays()

        def poison():
            for buf in bufs:
                buf.fill_u32(0x7FC0DEAD)

        def untouched():
            return all((words(buf.get_data()) == 0x7FC0DEAD).all() for buf in bufs)

        poison()
        assert one(h, dq, 0, C.byref(s), do) == 0 and any_(h, dq, 0, C.byref(s), df) == 0                  # count == 0: a no-op
        assert one(h, None, 0, None, None) == 0 and any_(h, None, 0, None, None) == 0
        for fn, out, name in ((one, q.out, b"lbvh_segment_closest_point"), (any_, q.flags, b"lbvh_segment_within_distance")):
            dout, odd = out.device, 8 if fn is one else 2
            for args in ((None, 10, C.byref(s), dout), (dq, 10, None, dout), (dq, 10, C.byref(s), None), (at(q.queries, 8), 10, C.byref(s), dout),
                         (at(q.queries, 4), 10, C.byref(s), dout), (dq, 10, C.byref(s), at(out, odd)), (dq, 1 << 32, C.byref(s), dout)):
                assert fn(h, *args) == -1, (name, args)
                assert b"invalid argument" in lib.lbvh_last_error(h)
            assert fn(None, dq, 10, C.byref(s), dout) == -1
        assert any_(h, dq, 10, C.byref(s), at(q.flags, 4)) == 0          # flags need 4-byte alignment only
        q.flags.fill_u32(0x7FC0DEAD)
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        for fn, out, name in ((one, do, b"lbvh_segment_closest_point"), (any_, df, b"lbvh_segment_within_distance")):
            assert fn(h, dq, 130, C.byref(s), out) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        assert (trace_rays() == expected_path).all()
        # aligned sub-ranges are fine
        assert one(h, at(q.queries, 32), 10, C.byref(s), at(q.out, 32)) == 0 and any_(h, at(q.queries, 32), 10, C.byref(s), at(q.flags, 4)) == 0
        assert (rw(q.out.get_data()[1:11]) == rw(ref.records[1:11])).all() and (q.flags.get_data()[1:11] == ref.flags[1:11]).all()
        for form in (q.closest, q.within):
            # each call drops the live-ray list the trace before it left: lbvh_trace_rays makes its own again
            assert (trace_rays() == expected_path).all()
            form()
        assert (trace_rays() == expected_path).all()
        assert_equal(q.closest(), q.within(), ref)
        for buf in (states, path_hits):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t6_a_small_lds_stack_and_the_statistics(ctx):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    q = Segs(ctx, d, queries)
    h, lib = ctx.handle, N().lib
    # a small LDS part exercises the device-memory part of the stack: the same answers
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        got, flags = q.closest(), q.within()
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert_equal(got, flags, ref, "stack split 1")
    q.dispose()
    # statistics, on the queries with a finite search radius: the closest form, the flag form, and lbvh_capsule_deepest with
    # r*r = max_dist2 on the same shapes, which visits every triangle whose box the capsule's box reaches
    bounded = np.isfinite(r)
    sub = Segs(ctx, d, queries[bounded])
    shapes = H().DataBuffer(ctx, int(bounded.sum()), L().CAPSULE)
    shapes.local[:] = capsules_of(queries[bounded], r[bounded])
    shapes.sync()
    deepest = H().DataBuffer(ctx, int(bounded.sum()), L().CONTACT)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    want = G.Result(ref.records[bounded], ref.flags[bounded], None, 0, 0)
    seen = []
    try:
        for form in ("closest", "within", "deepest"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            if form == "closest":
                assert (rw(sub.closest()) == rw(want.records)).all()             # the counting instantiations write the same words
            elif form == "within":
                assert (sub.within() == want.flags).all()
            else:
                d.capsule_deepest(shapes, deepest)
                deepest.get_data()
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("queries, node fetches, triangle lines: closest %s, within %s, capsule_deepest %s" % tuple(seen))
    active = int(G.active(queries[bounded]).sum())
    assert seen[0][0] == seen[1][0] == seen[2][0] == active
    assert seen[1][1] <= seen[0][1] and seen[1][2] <= seen[0][2]            # the flag form: never more fetches or tests
    assert 0 < seen[0][2] < seen[2][2] and seen[0][1] <= seen[2][1]          # fewer triangle lines than the overlap walk
    for buf in (shapes, deepest, stats):
        buf.dispose()
    sub.dispose()


@pytest.mark.gpu
def test_t7_clearance_of_capsules_above_a_floor(ctx):
    """A floor z = 0 of two large triangles and capsules of radius 0.5 whose axes point up and sideways: the lower end is the nearest
    point, so the clearance is its height less the radius — exactly, the heights being dyadic — and negative for a sunk capsule"""
    w = 20.0
    pos = np.array([((-w, -w, 0), (w, -w, 0), (w, w, 0)), ((-w, -w, 0), (w, w, 0), (-w, w, 0))], dtype=F)
    d = H().RaytracingMeshDrawer(ctx, pack(pos[:, 0], pos[:, 1], pos[:, 2])).awake()
    d.build_fast_scene()
    height = np.array([3.0, 0.75, 0.25, 1.5, 8.0], dtype=F)
    origin = np.stack([np.array([1, -5, 7, 2, -3], dtype=F), np.array([2, 6, -4, -8, 1], dtype=F), height], axis=1)
    axis = np.array([(0.5, 0, 2), (0, 1, 1), (-1, 0.5, 3), (0, 0, 0), (2, 2, 0.5)], dtype=F)
    caps = H().capsule_shapes(origin, axis, 0.5)
    gap, rec = d.clearance(caps)
    assert gap.dtype == F and gap.tolist() == (height - F(0.5)).tolist() and gap[2] == -0.25
    # (u and v of the face case are rounded quotients: along the floor, delta is a rounding of coordinates of up to 40)
    assert (rec["s"] == 0).all() and (rec["delta"][:, 2] == height).all() and (np.abs(rec["delta"][:, :2]) <= 8 * 2.0 ** -24 * 40).all()
    assert (rec["tri"] <= 1).all()
    buf = H().DataBuffer(ctx, len(caps), L().CAPSULE)
    buf.local[:] = caps
    buf.sync()
    gap2, rec2 = d.clearance(buf)                                       # a DataBuffer is taken the same way
    assert (words(gap2) == words(gap)).all() and (rw(rec2) == rw(rec)).all()
    buf.dispose()
    d.on_destroy()


@pytest.mark.gpu
def test_t7_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver segclosest 2000 15`: SegmentClosestPoints and SegmentWithinDistance of lbvh_host.hpp on the driver's own mesh and
    segments, against the reference on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "segclosest", str(count), "15"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    boxes = library_boxes(d)
    d.on_destroy()
    r = G.reference(G.driver_segments(lo, hi, count, seed=15), a, b, c, *boxes)
    weigh = (rw(r.records).astype(np.uint64) * np.arange(1, 9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert 100 < int(r.flags.sum()) < count
    assert (res["triangles"], res["segments"], res["found"], res["within"]) == (4096, count, int(r.flags.sum()), int(r.flags.sum()))
    assert res["word_sum"] == int((weigh * np.arange(1, count + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    first = np.nonzero(r.flags)[0][:3]
    assert res["closest"] == [[int(k)] + rw(r.records[k:k + 1])[0].tolist() for k in first]
