"""lbvh_triangle_closest_point / lbvh_triangle_within_distance: how far a triangle is from the mesh, where and in which direction, as
the nearest 32-byte record per query triangle and as one flag per query, over the four-wide derived traversal scene.  The
expectation is tests/triangle_closest_reference.py: the header's definition in numpy float32 — no tree.
  CPU  the surface in every host; hand-made pairs with answers derivable on paper; the reference against the test of every pair;
       the reference against float64 geometry that shares no line with it; relations (b) and (c) in the reference; the parity sets
       are not vacuous
  T1   parity of both calls on grid_80x80 and cfg1_4096        T2  relations (a), (b) and (c) on the device
  T3   query counts around a wave; wave caps (the lane refill)  T4  inactive queries; every output word is written
  T5   count == 0, every rejection, a stale scene, the live-path list (the contract tests/test_query_entry_contract.py asserts for
       the entry points it names, for these two)
  T6   a small LDS stack; the stack limit; statistics against the three-edge workaround and lbvh_box_overlaps
  T7   .mesh_distance of a tilted fan above a floor; tri_closest_witness; lbvh_driver triclosest: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import point_reference as P
import segment_closest_reference as G
import triangle_closest_reference as T
import triangle_query_reference as TQ
from query_support import driver_mesh, H, L, library_boxes, make_queries, N, pack, padded_boxes, positions, words
from test_shape_overlaps import (extent_of, K_EPS, PARITY, point_triangle_distance64, scene, segment_segment_distance64,
                                 segment_triangle_distance64)
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNT = 2000
OWN = 256
NAMES = ("lbvh_triangle_closest_point", "lbvh_triangle_within_distance")
NONE_WORDS = [int(words(np.array([T.MAX_FLOAT], dtype=F))[0]), 0, 0, 0, 0, 0, 0, 0]


def rw(records):
    """layouts.TRI_CLOSEST records -> (rows, 8) words"""
    return words(records).reshape(-1, 8)


def parity_queries(a, b, c, count=COUNT, seed=23):
    """Query triangles of 0.5 .. 5 % of the scene's extent about points of the surface, moved off by up to one size (the square root of a uniform draw) along a random
    direction, the three vertices at the size's distance from that centre in random directions.  Two constructed kinds, one in
    eight each, are there for the edge tests m >= 3, which a query above the inside of a flat mesh never needs:
      face-on   the query lies in the plane at right angles to a random direction d, 0.1 .. 0.6 sizes beyond the mesh's outermost
                vertex along d: that vertex is nearest to the inside of the query's face (the three-edge workaround is farther);
      crossed   one edge of the query crosses in space, 0.1 .. 0.6 sizes off, past the middle third of a scene edge that lies on the
                mesh's silhouette (an edge of a triangle that has the outermost vertex along d, cycling through v0-v1, v0-v2,
                v1-v2), the third vertex one size farther out: edge against edge, which test m < 3 and a scene edge test both see.
    One in sixteen is degenerate (a == b == c, at the centre), one in sixteen is ten extents away; half have a search radius of
    0.5 .. 5 % of the extent (max_dist2 = r*r), half are unbounded.  The last OWN are the mesh's own triangles (every (n // OWN)-th)
    with skip = their own index."""
    rng = np.random.default_rng(seed + len(a))
    ext = extent_of(a, b, c)
    k = rng.integers(0, len(a), count)
    w = rng.dirichlet((1, 1, 1), count)
    target = a[k].astype(np.float64) * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
    size = ext * rng.uniform(0.005, 0.05, count)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = target + d * (size * np.sqrt(rng.uniform(0.0, 1.0, count)))[:, None]          # (more of them far than near)
    i = np.arange(count)
    centre[i % 16 == 13] += 10.0 * ext * d[i % 16 == 13]
    arms = rng.normal(size=(count, 3, 3))
    arms *= (size[:, None] / np.linalg.norm(arms, axis=2))[:, :, None]
    arms[i % 16 == 5] = 0.0
    verts = centre[:, None, :] + arms
    # the two constructed kinds
    pts = np.stack([a, b, c], axis=1).astype(np.float64)               # [triangle, vertex, axis]
    gap = size * rng.uniform(0.1, 0.6, count)
    turn = rng.uniform(0.0, 2.0 * np.pi, count)
    part = rng.uniform(1.0 / 3.0, 2.0 / 3.0, count)
    for j in np.nonzero(i % 8 == 2)[0]:
        at = np.unravel_index(np.argmax(pts @ d[j]), pts.shape[:2])
        u = np.cross(d[j], (1.0, 0.0, 0.0) if abs(d[j][0]) < 0.9 else (0.0, 1.0, 0.0))
        u /= np.linalg.norm(u)
        v = np.cross(d[j], u)
        mid = pts[at] + d[j] * gap[j] + 0.2 * size[j] * (u * np.cos(3 * turn[j]) + v * np.sin(5 * turn[j]))
        for n in range(3):
            ang = turn[j] + n * 2.0 * np.pi / 3.0
            verts[j, n] = mid + size[j] * (u * np.cos(ang) + v * np.sin(ang))
    for n, j in enumerate(np.nonzero(i % 8 == 6)[0]):
        t = np.unravel_index(np.argmax(pts @ d[j]), pts.shape[:2])[0]
        p0, p1 = ((0, 1), (0, 2), (1, 2))[n % 3]
        e0, e1 = pts[t, p0], pts[t, p1]
        along = e1 - e0
        out = d[j] - along * (d[j] @ along) / (along @ along)
        out /= np.linalg.norm(out)
        side = np.cross(along, out)
        side /= np.linalg.norm(side)
        foot = e0 + along * part[j] + out * gap[j]
        lean = 0.3 * np.cos(turn[j])
        verts[j, 0] = foot + 0.5 * size[j] * (side + lean * out)
        verts[j, 1] = foot - 0.5 * size[j] * (side + lean * out)
        verts[j, 2] = foot + out * size[j] + 0.3 * size[j] * np.sin(turn[j]) * along / np.linalg.norm(along)
    qa, qb, qc = (verts[:, j].astype(F) for j in range(3))
    r = (ext * rng.uniform(0.005, 0.05, count)).astype(F)
    r = np.where(rng.random(count) < 0.5, r, F(np.inf)).astype(F)
    q = T.make_queries(qa, qb, qc, r * r)
    own = np.arange(OWN) * (len(a) // OWN)
    q["a"][-OWN:], q["b"][-OWN:], q["c"][-OWN:], q["skip"][-OWN:] = a[own], b[own], c[own], own
    return q, r


def edge_segments(q, m):
    """layouts.SEGMENT_QUERY of edge m = 0, 1, 2 of every query, with its max_dist2: the operands of edge test m"""
    p, d = T.edge_tests(q["a"], q["b"], q["c"], q["a"], q["a"], q["a"])[m][:2]
    return G.make_queries(p, d, q["max_dist2"])


_CPU = {}


def cpu_case(name):
    """(a, b, c, box_lo, box_hi, queries, r, reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        lo, hi = padded_boxes(a, b, c)
        q, r = parity_queries(a, b, c)
        _CPU[name] = (a, b, c, lo, hi, q, r, T.reference(q, a, b, c, lo, hi))
    return _CPU[name]


def cpu_edges(name):
    """the three segment references of the parity set's query edges (the three-edge workaround), once per scene"""
    if ("edges", name) not in _CPU:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        _CPU["edges", name] = [G.reference(edge_segments(q, m), a, b, c, lo, hi) for m in range(3)]
    return _CPU["edges", name]


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_records_and_the_two_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_tri_distance_query \{\s+float a\[3\]; uint32_t skip;[^}]*?float b\[3\]; float max_dist2;[^}]*?"
                     r"float c\[3\]; uint32_t _pad;[^}]*?\} lbvh_tri_distance_query;", h)
    assert re.search(r"typedef struct lbvh_tri_closest \{\s+float\s+dist2;[^}]*?uint32_t tri;[^}]*?uint32_t edge;[^}]*?float\s+s;[^}]*?"
                     r"float\s+delta\[3\];[^}]*?uint32_t _zero;[^}]*?\} lbvh_tri_closest;", h)
    assert re.search(r"lbvh_status lbvh_triangle_closest_point\(lbvh_context\* ctx, const lbvh_tri_distance_query\* d_queries, size_t count, "
                     r"const lbvh_scene\* h_scene,\s+lbvh_tri_closest\* d_out\);", h)
    assert re.search(r"lbvh_status lbvh_triangle_within_distance\(lbvh_context\* ctx, const lbvh_tri_distance_query\* d_queries, size_t count, "
                     r"const lbvh_scene\* h_scene,\s+uint32_t\* d_flags\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    assert re.search(r"uint32_t _pad0;[^\n]*not read", h[h.index("typedef struct lbvh_tri_query {"):])          # (still without a meaning)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert all(n in bounce for n in NAMES)
    text = h[h.index("Triangle closest-point queries: HOW FAR"):h.index("lbvh_status lbvh_triangle_closest_point(")]
    for must in ("max_dist2 > 0 (false for NaN)", "exact, not padded", "m = 0, 1, 2", "m = 3, 4, 5", "strictly", "edge = m | (pierced ? 8 : 0)",
                 "-rv_m per component", "Early exit", "fmaxf(fmaxf(B.lo_k - Q.max_k, Q.min_k - B.hi_k), 0)", "!= skip",
                 "!(dist2_i < box2q(own AABB_i))", "the lower original triangle index", "box2q(ancestor) <= box2q(leaf) <= dist2",
                 "only if box2q > best, strictly", "(a) the flag is 1 exactly when", "tri <= the least listed index", "word for word",
                 "NOT promised", "up to six segment tests (54 point tests) per triangle line read", "Out of scope: the k nearest"):
        assert must in text, must
    dbg = open(os.path.join(ROOT, "include", "lbvh_debug.h")).read()
    assert "lbvh_triangle_closest_point / lbvh_triangle_within_distance" in dbg


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    for n in NAMES:
        res, args = nat.SIGNATURES[n]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
    assert all(hasattr(nat.lib, n) for n in NAMES)
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.TRI_DISTANCE_QUERY.itemsize == 48 and lay.TRI_CLOSEST.itemsize == 32
    assert [lay.TRI_CLOSEST.fields[f][1] for f in ("dist2", "tri", "edge", "s", "delta", "_zero")] == [0, 4, 8, 12, 16, 28]
    assert [lay.TRI_DISTANCE_QUERY.fields[f][1] for f in ("a", "skip", "b", "max_dist2", "c", "_pad")] == [0, 12, 16, 28, 32, 44]
    assert rw(np.array([T.NONE])).tolist() == [NONE_WORDS]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_triangle_closest_point\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    assert re.search(r"public static extern int lbvh_triangle_within_distance\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    assert "public struct TriDistanceQuery " in cs and "public struct TriClosest " in cs
    td = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "TriangleDistance.cs")).read())
    assert all(n in td for n in NAMES) and "unsafe" not in td
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert all(f"void {m}(" in hpp for m in ("TriangleClosestPoints", "TriangleWithinDistance"))
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"triclosest", triclosest_main}' in drv and "lbvh_driver triclosest <n_queries> [seed]" in drv
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("triangle_closest_points", "triangle_within_distance", "mesh_distance"))
    assert all(callable(getattr(H(), f)) for f in ("tri_distance_queries", "tri_distance_queries_from_mesh", "tri_closest_witness"))
    q = H().tri_distance_queries([[1, 2, 3]], [4, 5, 6], [7, 8, 9], 4.0)
    assert q.dtype == lay.TRI_DISTANCE_QUERY and q["a"].tolist() == [[1, 2, 3]] and q["c"].tolist() == [[7, 8, 9]] and q["max_dist2"][0] == 4
    assert q["skip"][0] == lay.NULL and H().tri_distance_queries([0, 0, 0], [1, 0, 0], [0, 1, 0], skip=7)["skip"][0] == 7
    mesh = (np.zeros((3, 3), dtype=F), np.ones((3, 3), dtype=F), np.full((3, 3), 2, dtype=F))
    q = H().tri_distance_queries_from_mesh(mesh, 2.25, self_skip=True)
    assert q["skip"].tolist() == [0, 1, 2] and (q["max_dist2"] == 2.25).all() and (q["b"] == 1).all()
    assert (H().tri_distance_queries_from_mesh(mesh, 2.25)["skip"] == lay.NULL).all()


# ---- CPU: the restatement on pairs with answers derivable on paper -----------------------------------------------------------

TRI = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


def one_pair(qa, qb, qc, max_dist2=np.inf, tri=TRI, skip=T.NULL):
    """-> the record of one query triangle and one scene triangle"""
    t = np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    q = T.make_queries(np.array([qa], dtype=F), np.array([qb], dtype=F), np.array([qc], dtype=F), F(max_dist2), skip)
    r = T.reference(q, a, b, c, *padded_boxes(a, b, c))
    assert rw(r.records).tolist() == rw(T.brute_force(q, a, b, c, *padded_boxes(a, b, c))).tolist()
    assert int(r.flags[0]) == int(r.records["dist2"][0] != T.MAX_FLOAT) and r.records["_zero"][0] == 0
    return r.records[0]


def witness(qa, qb, qc, rec, tri=TRI):
    t = np.array(tri, dtype=F)
    q = T.make_queries(np.array([qa], dtype=F), np.array([qb], dtype=F), np.array([qc], dtype=F))
    on_q, on_s = H().tri_closest_witness(q, (t[None, 0], t[None, 1], t[None, 2]), np.array([rec]))
    return on_q[0].tolist(), on_s[0].tolist()


def test_reference_a_parallel_triangle_above_the_face():
    # every point is 0.75 above the face: every m ties, and the order rule takes m = 0 (whose own order rule takes s = 0)
    tri = ((1, 1, 0.75), (2, 1, 0.75), (1, 2, 0.75))
    k = one_pair(*tri)
    assert k["dist2"] == 0.5625 and k["edge"] == 0 and k["s"] == 0 and k["delta"].tolist() == [0, 0, 0.75] and k["tri"] == 0
    assert witness(*tri, k) == ([1, 1, 0.75], [1, 1, 0])
    # the search radius is open: dist2 == max_dist2 is none
    assert rw(np.array([one_pair(*tri, 0.5625)])).tolist() == [NONE_WORDS] and one_pair(*tri, 0.5626)["edge"] == 0


def test_reference_a_large_query_face_on_above_one_scene_vertex():
    # a small scene triangle whose vertex v1 is the top, under the middle of a large level query: no query edge is near, and the
    # scene's edge v0-v1 (m = 3) holds the nearest point at s = 1; m = 5 starts there (s = 0) and is not strictly less
    small = [(0, 0, 0), (0.5, 0.5, 1), (1, 0, 0)]
    big = ((-10, -10, 1.5), (12, -10, 1.5), (-10, 12, 1.5))
    k = one_pair(*big, tri=small)
    assert k["edge"] == 3 and k["s"] == 1 and k["dist2"] == 0.25 and k["delta"].tolist() == [0, 0, 0.5]
    on_q, on_s = witness(*big, k, tri=small)
    assert on_s == [0.5, 0.5, 1] and on_q == [0.5, 0.5, 1.5]
    # the top at v2: the edge v0-v2 (m = 4); at v0: m = 3 at s = 0
    assert one_pair(*big, tri=[(0, 0, 0), (1, 0, 0), (0.5, 0.5, 1)])["edge"] == 4
    k = one_pair(*big, tri=[(0.5, 0.5, 1), (0, 0, 0), (1, 0, 0)])
    assert k["edge"] == 3 and k["s"] == 0 and k["delta"].tolist() == [0, 0, 0.5]
    # from below the sign is the same rule: delta points from the scene to the query
    k = one_pair((-10, -10, -1.5), (12, -10, -1.5), (-10, 12, -1.5), tri=[(0.5, 0.5, -1), (0, 0, 0), (1, 0, 0)])
    assert k["edge"] == 3 and k["delta"].tolist() == [0, 0, -0.5]


def test_reference_edge_edge_crossed_in_space():
    # the query's edge a-b runs along y at x = 2, 0.5 under the scene's edge y = 0 ... crossed: it passes under the edge (0,0,0)-(4,0,0)
    tri = ((2, -1, -0.5), (2, -0.25, -0.5), (2, -0.625, -3))
    k = one_pair(*tri)
    # nearest: the end b = (2, -0.25, -0.5) against the point (2, 0, 0) of the edge
    assert k["edge"] in (0, 1) and k["dist2"] == 0.3125 and k["delta"].tolist() == [0, -0.25, -0.5]
    # truly crossed: the query's edge a-b goes across the scene's edge y = 0 at the height 0.5, the third vertex far above
    tri = ((2, -1, 0.5), (2, 1, 0.5), (2, 0, 9))
    k = one_pair(*tri, tri=[(0, 0, 0), (4, 0, 0), (0, -4, -4)])
    assert k["edge"] == 0 and k["s"] == 0.5 and k["dist2"] == 0.25 and k["delta"].tolist() == [0, 0, 0.5]
    assert witness(*tri, k, tri=[(0, 0, 0), (4, 0, 0), (0, -4, -4)]) == ([2, 0, 0.5], [2, 0, 0])


def test_reference_vertex_vertex():
    # the query's vertex b = (5, 0, 0) beyond the scene's vertex (4, 0, 0), the rest farther out
    tri = ((7, 1, 0), (5, 0, 0), (7, -1, 0))
    k = one_pair(*tri)
    assert k["dist2"] == 1 and k["delta"].tolist() == [1, 0, 0] and (int(k["edge"]), float(k["s"])) in ((0, 1.0), (1, 0.0))
    assert witness(*tri, k) == ([5, 0, 0], [4, 0, 0])


def test_reference_a_query_that_pierces():
    # the edge a-b goes through the face at (1, 1), z from -1 to 3: m = 0 pierces at t = 0.25
    k = one_pair((1, 1, -1), (1, 1, 3), (9, 9, 1))
    assert k["edge"] == 8 and k["s"] == 0.25 and words(k["dist2"]) == 0 and words(k["delta"]).tolist() == [0, 0, 0]
    k = one_pair((9, 9, 1), (1, 1, -1), (1, 1, 3), 1e-30)                # any positive radius finds a pierced triangle: m = 1
    assert k["edge"] == 9 and k["s"] == 0.25 and words(k["dist2"]) == 0
    on_q, on_s = witness((9, 9, 1), (1, 1, -1), (1, 1, 3), k)
    assert on_q == on_s == [1, 1, 0]


def test_reference_a_scene_edge_piercing_the_querys_face():
    # a large level query at z = 1 through which the scene triangle's top (v2) pokes: no query edge reaches the scene triangle, its
    # edges v0-v2 (m = 4) and v1-v2 (m = 5) pierce the query's face, and m = 4 is first
    poke = [(0, 0, 0), (1, 0, 0), (0.5, 0.5, 2)]
    k = one_pair((-10, -10, 1), (12, -10, 1), (-10, 12, 1), tri=poke)
    assert k["edge"] == (4 | 8) and abs(float(k["s"]) - 0.5) <= 2.0 ** -23 and words(k["dist2"]) == 0 and words(k["delta"]).tolist() == [0, 0, 0]
    # the top at v1: m = 3
    assert one_pair((-10, -10, 1), (12, -10, 1), (-10, 12, 1), tri=[(0, 0, 0), (0.5, 0.5, 2), (1, 0, 0)])["edge"] == (3 | 8)


def test_reference_skip_removes_the_only_triangle():
    tri = ((1, 1, 0.75), (2, 1, 0.75), (1, 2, 0.75))
    assert rw(np.array([one_pair(*tri, skip=0)])).tolist() == [NONE_WORDS]
    assert one_pair(*tri, skip=1)["dist2"] == 0.5625


def test_reference_inactive_queries_have_nothing():
    t = np.array(TRI, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    base = np.array([[(1, 1, 0.75), (2, 1, 0.75), (1, 2, 0.75)]], dtype=F)
    n = 1 + 9 * 3 + 4
    v = np.tile(base, (n, 1, 1))
    q = T.make_queries(v[:, 0], v[:, 1], v[:, 2])
    at = 1
    for bad in (np.nan, np.inf, -np.inf):                               # each position
        for vert in "abc":
            for k in range(3):
                q[vert][at, k] = bad
                at += 1
    q["max_dist2"][at:at + 4] = (0, -0.0, -1, np.nan)
    assert at + 4 == n and T.active(q).tolist() == [True] + [False] * (n - 1)
    r = T.reference(q, a, b, c, *padded_boxes(a, b, c))
    assert r.flags.tolist() == [1] + [0] * (n - 1) and (rw(r.records[1:]) == NONE_WORDS).all()
    assert (rw(T.brute_force(q, a, b, c, *padded_boxes(a, b, c))) == rw(r.records)).all()


# ---- CPU: the reference and the test of every pair; float64; the relations; the sets ------------------------------------------

def test_the_reference_is_the_test_of_every_pair():
    """triangle_closest_reference.reference leaves out the narrow phase of the pairs the candidate rule itself excludes; on the first
    48 queries of each parity set, and on 16 of the mesh's own triangles with `skip`, the record is the one the six tests of EVERY pair
    give"""
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        assert (rw(T.brute_force(q[:48], a, b, c, lo, hi)) == rw(ref.records[:48])).all()
        assert (rw(T.brute_force(q[-16:], a, b, c, lo, hi)) == rw(ref.records[-16:])).all()
        assert ref.tested < 0.02 * COUNT * len(a)


def tri_tri_distance64(qa, qb, qc, a, b, c):
    """rows of triangle pairs, float64: 0 if an edge of one passes through the other, else the least of the nine edge-edge and the
    six vertex-triangle distances.  A degenerate triangle has no face: the tests against it give NaN and are left out (fmin)."""
    with np.errstate(all="ignore"):
        qs, ss = ((qa, qb), (qb, qc), (qc, qa)), ((a, b), (b, c), (c, a))
        best = np.full(len(qa), np.inf)
        for u, v in qs:
            for x, y in ss:
                best = np.fmin(best, segment_segment_distance64(u, v - u, x, y - x))
        for p in (qa, qb, qc):
            best = np.fmin(best, point_triangle_distance64(p, a, b, c))
        for p in (a, b, c):
            best = np.fmin(best, point_triangle_distance64(p, qa, qb, qc))
        through = np.zeros(len(qa), dtype=bool)
        for u, v in qs:
            through |= segment_triangle_distance64(u, v - u, a, b, c) == 0
        for x, y in ss:
            through |= segment_triangle_distance64(x, y - x, qa, qb, qc) == 0
    return np.where(through, 0.0, best)


def test_the_float64_distance_knows_its_own_answers():
    f = lambda *rows: [np.array([r], dtype=np.float64) for r in rows]
    t = f(*TRI)
    assert tri_tri_distance64(*f((1, 1, 0.75), (2, 1, 0.75), (1, 2, 0.75)), *t)[0] == 0.75
    assert tri_tri_distance64(*f((1, 1, -1), (1, 1, 3), (9, 9, 1)), *t)[0] == 0
    assert tri_tri_distance64(*f((7, 1, 0), (5, 0, 0), (7, -1, 0)), *t)[0] == 1
    assert tri_tri_distance64(*f((-10, -10, 1.5), (12, -10, 1.5), (-10, 12, 1.5)), *f((0, 0, 0), (0.5, 0.5, 1), (1, 0, 0)))[0] == 0.5
    assert tri_tri_distance64(*f((1, 1, 2), (1, 1, 2), (1, 1, 2)), *t)[0] == 2


def test_reference_agrees_with_an_independent_float64_evaluation():
    """Every record of the parity sets against float64 triangle-triangle geometry built from tests/test_shape_overlaps.py's helpers
    (nine segment_segment_distance64, six point_triangle_distance64, zero where a segment_triangle_distance64 is zero), with
    band = K_EPS * 2^-24 * extent, the extent that of what the arithmetic sees, the mesh AND the query.
      per pair    |sqrt(dist2) - dist64(query, winning triangle)| <= band
      the winner  on the first 64 active queries of each set: no triangle (but `skip`) is nearer in float64 than sqrt(dist2) - band,
                  and where the record is none, none is nearer than sqrt(R) - band"""
    eps = 2.0 ** -24
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        pts = np.concatenate([a, b, c]).astype(np.float64)
        verts = np.stack([q[k].astype(np.float64) for k in "abc"])
        reach = (np.maximum(pts.max(axis=0), verts.max(axis=0)) - np.minimum(pts.min(axis=0), verts.min(axis=0))).max(axis=1)
        assert (reach >= extent_of(a, b, c)).all() and np.median(reach) <= 1.3 * extent_of(a, b, c)
        band_of = K_EPS * eps * reach
        found = np.nonzero(ref.flags == 1)[0]
        tri = ref.records["tri"][found].astype(np.int64)
        dist = tri_tri_distance64(*(q[k][found].astype(np.float64) for k in "abc"), *(x[tri].astype(np.float64) for x in (a, b, c)))
        err = np.abs(np.sqrt(ref.records["dist2"][found].astype(np.float64)) - dist)
        print(f"{name}: {len(found)} records, {int((dist == 0).sum())} cross in float64, {int((ref.records['edge'][found] & 8 != 0).sum())} pierce "
              f"in fp32, distance error <= {(err / band_of[found]).max():.3f} band")
        assert (err <= band_of[found]).all(), (name, found[err > band_of[found]][:5], (err / band_of[found]).max())
        first = np.nonzero(T.active(q))[0][:64]
        rows, every = (v.reshape(-1) for v in np.meshgrid(first, np.arange(len(a)), indexing="ij"))
        d_all = tri_tri_distance64(*(q[k][rows].astype(np.float64) for k in "abc"),
                                   *(x[every].astype(np.float64) for x in (a, b, c))).reshape(len(first), len(a))
        skipped = np.nonzero(q["skip"][first] != T.NULL)[0]
        d_all[skipped, q["skip"][first][skipped].astype(np.int64)] = np.inf
        bound = np.where(ref.flags[first] == 1, np.sqrt(ref.records["dist2"][first].astype(np.float64)),
                         np.sqrt(T.radius2(q)[first].astype(np.float64)))
        assert (d_all.min(axis=1) >= bound - band_of[first]).all(), name


def tri_queries_of(q):
    return TQ.make_queries(q["a"], q["b"], q["c"], q["skip"])


def check_relation_b(records, offsets, tris):
    """(offsets, tris): lbvh_triangle_intersections of {a, b, c, skip} -> how many queries list anything"""
    listed = 0
    for k in range(len(records)):
        seg = tris[int(offsets[k]):int(offsets[k + 1])]
        if len(seg):
            listed += 1
            assert words(records["dist2"][k]) == 0 and records["edge"][k] & 8 and records["tri"][k] <= seg.min(), k
    return listed


def check_relation_c(q, records, edges, clean):
    """edges: the SEGMENT_CLOSEST records of the three query edges; clean: the queries for which no accept rule rejected anything
    -> how many records equal an edge's record word for word"""
    equal = 0
    plain = np.nonzero(clean & (q["skip"] == T.NULL))[0]
    for m in range(3):
        e = edges[m]
        assert (records["dist2"][plain] <= e["dist2"][plain]).all(), m
        same = plain[(records["edge"][plain] & 7 == m) & (records["tri"][plain] == e["tri"][plain]) & (records["dist2"][plain] != T.MAX_FLOAT)]
        assert (words(records["dist2"][same]) == words(e["dist2"][same])).all() and (words(records["s"][same]) == words(e["s"][same])).all()
        assert (words(records["delta"][same]) == words(e["delta"][same])).all(), m
        equal += len(same)
    return equal


def test_relation_b_in_the_reference():
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        hit = TQ.reference(tri_queries_of(q), a, b, c, lo, hi)
        listed = check_relation_b(ref.records, hit.offsets, hit.tris)
        print(f"{name}: {listed} queries intersect something")
        assert listed >= 100


def test_relation_c_in_the_reference():
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        edges = cpu_edges(name)
        assert ref.rejected == 0 and all(e.rejected == 0 for e in edges)       # (the accept rules rejected nothing on these sets)
        equal = check_relation_c(q, ref.records, [e.records for e in edges], np.ones(COUNT, dtype=bool))
        print(f"{name}: {equal} records are an edge's segment record word for word")
        assert equal >= 200


def workaround_dist2(edges):
    return np.minimum(np.minimum(edges[0]["dist2"], edges[1]["dist2"]), edges[2]["dist2"])


def test_the_parity_sets_are_not_vacuous():
    for name in PARITY:
        a, b, c, lo, hi, q, r, ref = cpu_case(name)
        found = ref.flags == 1
        rec = ref.records
        by_m = np.bincount((rec["edge"][found] & 7).astype(np.int64), minlength=6)
        pierced = int((rec["edge"][found] & 8 != 0).sum())
        larger = int((found & (workaround_dist2([e.records for e in cpu_edges(name)]) > rec["dist2"])).sum())
        degenerate = (q["a"] == q["b"]).all(axis=1) & (q["a"] == q["c"]).all(axis=1)
        print(f"{name}: {int(found.sum())} with a record, winning m {by_m.tolist()}, {pierced} pierced, {int((~found).sum())} none, "
              f"{larger} where the three-edge workaround is farther, {ref.rejected} rejected by the accept rule, {ref.tested} pairs tested")
        assert len(q) == COUNT and T.active(q).all()
        assert (by_m >= 20).all() and pierced >= 100 and (~found).sum() >= 100 and larger >= 100
        i = np.arange(COUNT - OWN)
        assert degenerate[:-OWN].sum() == (i % 16 == 5).sum() and found[degenerate].any()
        assert np.isinf(q["max_dist2"]).sum() > COUNT // 4 and (~np.isinf(q["max_dist2"])).sum() > COUNT // 4
        assert (q["skip"][-OWN:] != T.NULL).all() and (q["skip"][:-OWN] == T.NULL).all() and (rec["tri"][-OWN:][found[-OWN:]] != q["skip"][-OWN:][found[-OWN:]]).all()
        far = np.zeros(COUNT, dtype=bool)
        far[:-OWN] = i % 16 == 13
        assert (~found[far & ~np.isinf(q["max_dist2"])]).all() and found[far].any()
        # (d), reported, not a contract: the degenerate queries against the point query at a
        pq = P.reference(make_queries(q["a"][degenerate], q["max_dist2"][degenerate]), a, b, c, lo, hi)
        same = (words(pq.records["dist2"]) == words(rec["dist2"][degenerate])) & (pq.records["tri"] == rec["tri"][degenerate])
        print(f"{name}: {int(same.sum())} of {int(degenerate.sum())} degenerate queries have the point query's dist2 and tri")


def test_driver_generator_is_deterministic_and_inside_the_box():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    q, q2 = T.driver_triangles(lo, hi, 50, seed=5), T.driver_triangles(lo, hi, 50, seed=5)
    assert (words(q) == words(q2)).all() and (q["a"] >= lo).all() and (q["a"] <= hi).all()
    assert (np.abs(q["b"] - q["a"]) <= 3.001).all() and (np.abs(q["c"] - q["a"]) <= 3.001).all()
    assert (q["max_dist2"][0::2] == 4).all() and np.isinf(q["max_dist2"][1::2]).all() and T.active(q).all() and (q["skip"] == T.NULL).all()
    assert (words(q) != words(T.driver_triangles(lo, hi, 50, seed=6))).any()
    qa, qb, qc = TQ.driver_triangles(lo, hi, 50, seed=5)                  # the same draws as `lbvh_driver tris`
    assert (words(q["a"]) == words(qa)).all() and (words(q["c"]) == words(qc)).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Tris:
    """device buffers of one query set; closest() / within() = one call each on caller-owned buffers"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer, self.count = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, max(len(queries), 1), L().TRI_DISTANCE_QUERY)
        self.queries.local[:len(queries)] = queries
        self.queries.sync()
        self.out = H().DataBuffer(ctx, max(len(queries), 1), L().TRI_CLOSEST)
        self.flags = H().DataBuffer(ctx, max(len(queries), 1), np.uint32)

    def closest(self):
        self.out.fill_u32(0xDEADBEEF)
        self.drawer.triangle_closest_points(self.queries, self.out)
        return self.out.get_data()[:self.count].copy()

    def within(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.triangle_within_distance(self.queries, self.flags)
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
        _GPU["ref", name] = (q, r, T.reference(q, a, b, c, lo, hi))
    return (a, b, c, lo, hi) + _GPU["ref", name] + (d,)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, name)
    assert int(ref.flags.sum()) >= 1000
    q = Tris(ctx, d, queries)
    assert_equal(q.closest(), q.within(), ref)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t2_relations_a_b_and_c_on_the_device(ctx, name):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, name)
    q = Tris(ctx, d, queries)
    runs = [(words(q.closest()).copy(), q.within()) for _ in range(2)]
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all()       # two calls write the same bytes
    got, flags = q.closest(), q.within()
    assert ((got["dist2"] != T.MAX_FLOAT) == (flags == 1)).all() and set(flags.tolist()) == {0, 1}          # (a)
    q.dispose()
    # (b): lbvh_triangle_intersections of {a, b, c, skip} on the device
    tq = H().DataBuffer(ctx, COUNT, L().TRI_QUERY)
    tq.local[:] = tri_queries_of(queries)
    tq.sync()
    off, tris = d.intersections(tq)
    listed = check_relation_b(got, off, tris)
    tq.dispose()
    # (c): lbvh_segment_closest_point on the three edges of every query, on the device
    edges = []
    sq = H().DataBuffer(ctx, COUNT, L().SEGMENT_QUERY)
    so = H().DataBuffer(ctx, COUNT, L().SEGMENT_CLOSEST)
    for m in range(3):
        sq.local[:] = edge_segments(queries, m)
        sq.sync()
        d.segment_closest_points(sq, so)
        edges.append(so.get_data()[:COUNT].copy())
    sq.dispose()
    so.dispose()
    clean = np.ones(COUNT, dtype=bool)
    if ref.rejected or any(G.reference(edge_segments(queries, m), a, b, c, lo, hi).rejected for m in range(3)):
        pytest.fail("the accept rule rejected a pair on a parity set: relation (c) needs the per-query mask")
    equal = check_relation_c(queries, got, edges, clean)
    larger = int(((got["dist2"] != T.MAX_FLOAT) & (workaround_dist2(edges) > got["dist2"])).sum())
    print(f"{name}: {listed} queries intersect something, {equal} records equal an edge's segment record, the three-edge workaround is "
          f"farther on {larger}")
    assert listed >= 100 and equal >= 200 and larger >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_t3_query_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    first = int(np.nonzero(ref.flags)[0][0])                           # (the single query is one with a record)
    sub = queries[first:first + count]
    want = T.Result(ref.records[first:first + count], ref.flags[first:first + count], 0, 0)
    q = Tris(ctx, d, sub)
    assert_equal(q.closest(), q.within(), want, count)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t3_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 queries on 1, 2, 3 or 7 waves: runs of 1 500 .. 215, every lane refilled many times"""
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:1500].copy()
    sub["b"][100:235, 0] = np.nan                                       # a block of inactive queries inside a run
    want = T.Result(ref.records[:1500].copy(), ref.flags[:1500].copy(), 0, 0)
    want.records[100:235] = T.NONE
    want.flags[100:235] = 0
    q = Tris(ctx, d, sub)
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
    for j, p in enumerate(places[0:30]):
        sub["abc"[j % 3]][p, (j // 3) % 3] = (np.nan, np.inf, -np.inf)[j // 10]
    sub["max_dist2"][places[30:35]] = 0
    sub["max_dist2"][places[35:40]] = -0.0
    sub["max_dist2"][places[40:45]] = np.where(np.arange(5) % 2, -1.0, -np.inf).astype(F)
    sub["max_dist2"][places[45:50]] = np.nan
    return sub, places


@pytest.mark.gpu
def test_t4_inactive_queries_among_active_ones(ctx):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, "grid_80x80")
    sub, places = spoiled(queries[:700])
    act = T.active(sub)
    assert (~act).sum() == len(places) and not act[places].any()
    q = Tris(ctx, d, sub)
    got, flags = q.closest(), q.within()                                # (both buffers were filled with 0xDEADBEEF)
    assert (rw(got[~act]) == NONE_WORDS).all() and (flags[~act] == 0).all()
    # the neighbours are what they were in the full set: every output word is written, and none of another query
    assert (rw(got[act]) == rw(ref.records[:700][act])).all() and (flags[act] == ref.flags[:700][act]).all() and flags[act].sum() > 0
    assert (got["_zero"] == 0).all()
    q.dispose()
    # an inactive query is never walked: the set of only them fetches no node
    idle = Tris(ctx, d, sub[~act])
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


def small_case():
    """64 random triangles and 130 query triangles about them, with the brute force's records"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    rng = np.random.default_rng(5)
    centre = a[rng.integers(0, 64, 130)] + rng.normal(size=(130, 3)).astype(F) * F(3)
    arms = rng.normal(size=(3, 130, 3)).astype(F)
    return tris, a, b, c, centre, T.make_queries(centre + arms[0], centre + arms[1], centre + arms[2], F(1.0))


@pytest.mark.gpu
def test_t5_count_zero_rejections_a_stale_scene_and_the_live_path_list():
    """the rows tests/test_query_entry_contract.py has for the entry points it names, for these two: on a context of its own"""
    tris, a, b, c, centre, queries = small_case()
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        ref = T.reference(queries, a, b, c, lo, hi)
        assert (rw(ref.records) == rw(T.brute_force(queries, a, b, c, lo, hi))).all() and 0 < ref.flags.sum() < 130
        q = Tris(ctx, d, queries)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        one, any_ = lib.lbvh_triangle_closest_point, lib.lbvh_triangle_within_distance
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
        for fn, out, name in ((one, q.out, b"lbvh_triangle_closest_point"), (any_, q.flags, b"lbvh_triangle_within_distance")):
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
        for fn, out, name in ((one, do, b"lbvh_triangle_closest_point"), (any_, df, b"lbvh_triangle_within_distance")):
            assert fn(h, dq, 130, C.byref(s), out) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        assert (trace_rays() == expected_path).all()
        # aligned sub-ranges are fine
        assert one(h, at(q.queries, 48), 10, C.byref(s), at(q.out, 32)) == 0 and any_(h, at(q.queries, 48), 10, C.byref(s), at(q.flags, 4)) == 0
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
    q = Tris(ctx, d, queries)
    h, lib = ctx.handle, N().lib
    # a small LDS part exercises the device-memory part of the stack: the same answers
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        got, flags = q.closest(), q.within()
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert_equal(got, flags, ref, "stack split 1")
    q.dispose()
    # statistics, on the queries with a finite search radius and no `skip`: the closest form, the flag form, the three-edge workaround
    # (three lbvh_segment_closest_point calls) and lbvh_box_overlaps on the query's box padded by the search radius
    bounded = np.isfinite(r) & (queries["skip"] == T.NULL)
    n = int(bounded.sum())
    sub = Tris(ctx, d, queries[bounded])
    sq = [H().DataBuffer(ctx, n, L().SEGMENT_QUERY) for _ in range(3)]
    for m in range(3):
        sq[m].local[:] = edge_segments(queries[bounded], m)
        sq[m].sync()
    so = H().DataBuffer(ctx, n, L().SEGMENT_CLOSEST)
    boxes = H().DataBuffer(ctx, n, L().AABB)
    qlo, qhi = T.query_box(queries[bounded])
    boxes.local["min"], boxes.local["max"] = qlo - r[bounded][:, None], qhi + r[bounded][:, None]
    boxes.sync()
    offsets = H().DataBuffer(ctx, n + 1, np.uint64)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    want = T.Result(ref.records[bounded], ref.flags[bounded], 0, 0)
    seen = []
    try:
        for form in ("closest", "within", "edges", "boxes"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            if form == "closest":
                assert (rw(sub.closest()) == rw(want.records)).all()             # the counting instantiations write the same words
            elif form == "within":
                assert (sub.within() == want.flags).all()
            elif form == "edges":
                for m in range(3):
                    d.segment_closest_points(sq[m], so)
                so.get_data()
            else:
                d.box_overlaps(boxes, offsets)
                offsets.get_data()
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("queries, node fetches, triangle lines: closest %s, within %s, three edges %s, box_overlaps %s" % tuple(seen))
    assert seen[0][0] == seen[1][0] == n and seen[2][0] == 3 * n
    assert seen[1][1] <= seen[0][1] and seen[1][2] <= seen[0][2]            # the flag form: never more fetches or tests
    assert 0 < seen[0][2] < seen[2][2] and seen[0][1] < seen[2][1]           # one walk reads fewer lines than three
    for buf in sq + [so, boxes, offsets, stats]:
        buf.dispose()
    sub.dispose()


@pytest.mark.gpu
def test_t6_the_stack_limit_is_reported():
    """lbvh_debug_ray_stack_limit(1): a walk that needs more than one stack entry reports LBVH_FAULT_RAY_STACK (LBVH_ERR_HIP at the next
    sync), never a silently wrong record; with the limit lifted the records are the reference's again.  On a context of its own."""
    tris, a, b, c, centre, queries = small_case()
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        d.build_fast_scene()
        ref = T.reference(queries, a, b, c, *library_boxes(d))
        q = Tris(ctx, d, queries)
        h, lib = ctx.handle, N().lib
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        d.triangle_closest_points(q.queries, q.out)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_equal(q.closest(), q.within(), ref)
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t7_mesh_distance_of_a_tilted_fan_above_a_floor(ctx):
    """A floor z = 0 of two large triangles and a fan of four triangles about the apex (1, 2, 0.75) whose rim rises away from it: the
    apex is the nearest point of every fan triangle, so the distance is 0.75 exactly, the first fan triangle (the lower index on equal
    dist2) names it, and the witness points are the apex and its foot"""
    w = 20.0
    pos = np.array([((-w, -w, 0), (w, -w, 0), (w, w, 0)), ((-w, -w, 0), (w, w, 0), (-w, w, 0))], dtype=F)
    d = H().RaytracingMeshDrawer(ctx, pack(pos[:, 0], pos[:, 1], pos[:, 2])).awake()
    d.build_fast_scene()
    apex = np.array([1, 2, 0.75], dtype=F)
    rim = np.array([(3, 2, 1.75), (1, 4, 2.25), (-1, 2, 2.75), (1, 0, 1.25), (3, 2, 1.75)], dtype=F)
    fan = (rim[:4], np.tile(apex, (4, 1)), rim[1:])                        # (a, b, c): the apex is vertex b of every triangle
    dist, k, tri, p_query, p_scene = d.mesh_distance(fan)
    assert dist == 0.75 and k == 0 and tri in (0, 1)
    assert np.abs(p_query - apex).max() <= 1e-6 and np.abs(p_scene - (1, 2, 0)).max() <= 1e-5
    assert d.mesh_distance(fan, max_dist=0.75) == (float("inf"), -1, -1, None, None)          # the search radius is open
    assert d.mesh_distance(pack(*fan), max_dist=0.76)[:3] == (0.75, 0, tri)                     # layouts.TRIANGLE is taken the same way
    # the witness points of a whole set are sqrt(dist2) apart within the band
    q = H().tri_distance_queries_from_mesh(fan)
    buf = Tris(ctx, d, q)
    rec = buf.closest()
    on_q, on_s = H().tri_closest_witness(q, pack(pos[:, 0], pos[:, 1], pos[:, 2]), rec)
    band = K_EPS * 2.0 ** -24 * 2 * w
    assert (np.abs(np.linalg.norm(on_q - on_s, axis=1) - np.sqrt(rec["dist2"].astype(np.float64))) <= band).all()
    assert (rec["dist2"] == F(0.5625)).all() and (np.abs(on_q - apex).max(axis=1) <= band).all()
    buf.dispose()
    d.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t7_witness_points_are_the_distance_apart(ctx, name):
    a, b, c, lo, hi, queries, r, ref, d = gpu_case(ctx, name)
    q = Tris(ctx, d, queries)
    rec = q.closest()
    q.dispose()
    found = rec["dist2"] != T.MAX_FLOAT
    on_q, on_s = H().tri_closest_witness(queries, scene(name), rec)
    assert np.isnan(on_q[~found]).all() and np.isnan(on_s[~found]).all()
    pts = np.concatenate([a, b, c, queries["a"][found], queries["b"][found], queries["c"][found]]).astype(np.float64)
    band = K_EPS * 2.0 ** -24 * float((pts.max(axis=0) - pts.min(axis=0)).max())
    plain = found & (rec["edge"] & 8 == 0)
    gap = np.linalg.norm(on_q - on_s, axis=1)
    assert (np.abs(gap[plain] - np.sqrt(rec["dist2"][plain].astype(np.float64))) <= band).all()
    assert (gap[found & ~plain] == 0).all()                              # pierced: one point


@pytest.mark.gpu
def test_t7_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver triclosest 2000 21`: TriangleClosestPoints and TriangleWithinDistance of lbvh_host.hpp on the driver's own mesh and
    queries, against the reference on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "triclosest", str(count), "21"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    boxes = library_boxes(d)
    d.on_destroy()
    r = T.reference(T.driver_triangles(lo, hi, count, seed=21), a, b, c, *boxes)
    weigh = (rw(r.records).astype(np.uint64) * np.arange(1, 9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert 100 < int(r.flags.sum()) < count
    assert (res["triangles"], res["queries"], res["found"], res["within"]) == (4096, count, int(r.flags.sum()), int(r.flags.sum()))
    assert res["pierced"] == int((r.records["edge"] & 8 != 0).sum())
    assert res["word_sum"] == int((weigh * np.arange(1, count + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    first = np.nonzero(r.flags)[0][:3]
    assert res["closest"] == [[int(k)] + rw(r.records[k:k + 1])[0].tolist() for k in first]
