"""lbvh_triangle_intersection_segments: WHERE a triangle cuts each scene triangle it intersects — lbvh_triangle_intersections with a
32-byte record (the two ends, tri, edges) in place of an index.  The expectation is tests/triangle_segment_reference.py: the
header's record in numpy float32 on the candidate pairs of tests/triangle_query_reference.py, with the triangles' own boxes as the
library produced them — no tree.  The order inside a segment is not part of the contract, so every GPU comparison is word for word
after a host sort of each segment by tri.  The scenes and the parity_queries recipe are tests/test_triangle_queries.py's, restated,
with every 250th query laid through a scene vertex (the records with more than two bits).
  CPU  the surface in every host; hand-built pairs with known answers; the running-pair rule; the parity sets are not vacuous; the
       restatement against a float64 construction that shares no line with it
  T1   parity on grid_80x80 and cfg1_4096             T2  query counts around a wave; wave caps (the lane refill)
  T3   a mesh against itself                          T4  inactive queries
  T5   count-only, overflow, two calls                T6  count == 0, every rejection, a stale scene (the entry contract)
  T7   a small LDS stack; statistics                  T8  lbvh_driver trisegs: the C++ host end to end
  T9   non-empty exactly where lbvh_triangle_intersects_any says 1"""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import triangle_query_reference as T
import triangle_segment_reference as S
from query_support import driver_mesh, H, L, library_boxes, N, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NULL = T.NULL
COUNT = 2000
PARITY = ["grid_80x80", "cfg1_4096"]
# The margin of the float64 check in units of 2^-24 * extent: DESIGN §34's bound of a static test on these operations (four times
# the least K at which the box cast's restatement passes its float64 clip, §33).
K_EPS = 4 * 3.86


def scene(name):
    """the triangles of the two goldens, from the seeded generators that made them (tests/test_gpu_parity.py checks they still do)"""
    tris = scenes.grid_scene() if name == "grid_80x80" else scenes.random_triangles(4096, seed=1)
    assert len(tris) == (12800 if name == "grid_80x80" else 4096)
    return tris


def parity_queries(a, b, c, count=COUNT, seed=11):
    """The recipe of tests/test_triangle_queries.py: scene triangles turned about their centroid by a seeded angle about a seeded axis
    and scaled by 0.5 .. 4; two fifths of them then moved off by 2 .. 8 times their size in a random direction (the queries with no
    candidate); a quarter carry skip = the triangle they were made from."""
    rng = np.random.default_rng(seed + len(a))
    k = rng.integers(0, len(a), count)
    v = np.stack([a[k], b[k], c[k]], axis=1).astype(np.float64)
    centre = v.mean(axis=1, keepdims=True)
    axis = rng.normal(size=(count, 3))
    axis = (axis / np.linalg.norm(axis, axis=1, keepdims=True))[:, None, :]
    angle = rng.uniform(0.0, 2.0 * np.pi, count)
    co, si = np.cos(angle)[:, None, None], np.sin(angle)[:, None, None]
    r = v - centre
    turned = r * co + np.cross(axis, r) * si + axis * (axis * r).sum(axis=2, keepdims=True) * (1.0 - co)
    out = centre + turned * rng.uniform(0.5, 4.0, count)[:, None, None]
    size = np.linalg.norm(r, axis=2).max(axis=1)
    away = rng.random(count) < 0.4
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out[away] += (d[away] * (size[away] * rng.uniform(2.0, 8.0, away.sum()))[:, None])[:, None, :]
    skip = np.where(rng.random(count) < 0.25, k, NULL).astype(np.uint32)
    out = out.astype(F)
    # added to that recipe, for records with more than two bits: every 250th query has its edge a-b through a scene vertex p (the
    # middle of the edge, at steps of 1 / 64, so that p - d and p + d are exact where p is), where several scene triangles meet and
    # several tests sit at their bounds; no skip
    through = np.arange(count) % 250 == 7
    p = np.stack([a, b, c], axis=1)[k[through], rng.integers(0, 3, through.sum())]
    d, e = (np.round(rng.uniform(-1.0, 1.0, (through.sum(), 3)) * size[through, None] * 64.0) / 64.0 for _ in range(2))
    out[through] = np.stack([p - d, p + d, p + e], axis=1).astype(F)
    skip[through] = NULL
    return T.make_queries(out[:, 0], out[:, 1], out[:, 2], skip)


_CPU = {}


def cpu_case(name):
    """(a, b, c, queries, reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        q = parity_queries(a, b, c)
        _CPU[name] = (a, b, c, q, S.reference(q, a, b, c, *padded_boxes(a, b, c)))
    return _CPU[name]


def extent_of(a, b, c):
    pts = np.concatenate([a, b, c]).astype(np.float64)
    return float((pts.max(axis=0) - pts.min(axis=0)).max())


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_struct_and_the_call():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_tri_segment \{\s*float p0\[3\]; uint32_t tri;[^\n]*\n\s*float p1\[3\]; uint32_t edges;[^\n]*\n"
                     r"\} lbvh_tri_segment;", h)
    assert re.search(r"lbvh_status lbvh_triangle_intersection_segments\(lbvh_context\* ctx, const lbvh_tri_query\* d_queries, size_t count,\s+"
                     r"const lbvh_scene\* h_scene, uint64_t\* d_offsets,\s+lbvh_tri_segment\* d_segments, uint64_t capacity\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_triangle_intersection_segments" in bounce
    text = h[h.index("Triangle intersection segments: WHERE"):h.index("lbvh_status lbvh_triangle_intersection_segments(")]
    for must in ("No test ends the sequence", "X_j = P_j + D_j * t_j", "d0 > d01 && d0 >= d1", "else if (d1 > d01)", "bits 8 .. 10",
                 "bits 12 .. 14", "p0 == p1", "NOT PART OF THE CONTRACT", "d_offsets[0] included", "function of (query, triangle) only",
                 "16-byte aligned"):
        assert must in text, must


def test_native_prototype_layout_and_the_other_hosts():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_triangle_intersection_segments"]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    assert hasattr(nat.lib, "lbvh_triangle_intersection_segments")
    lay = L()
    assert lay.TRI_SEGMENT.itemsize == 32
    assert [lay.TRI_SEGMENT.fields[f][1] for f in ("p0", "tri", "p1", "edges")] == [0, 12, 16, 28]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_triangle_intersection_segments\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, "
                     r"IntPtr \w+,\s+IntPtr \w+,\s+ulong capacity\);", cs)
    ts = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "TriangleSegments.cs")).read())
    assert "lbvh_triangle_intersection_segments" in ts and "unsafe" not in ts
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void TriangleIntersectionSegments(" in hpp
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"trisegs", trisegs_main}' in drv
    host = H()
    assert all(hasattr(host.RaytracingMeshDrawer, m) for m in ("triangle_intersection_segments", "intersection_segments"))
    assert callable(host.tri_queries_from_mesh) and callable(host.segment_edges)


def test_host_helpers():
    host = H()
    tris = scenes.random_triangles(n=10, seed=3)
    q = host.tri_queries_from_mesh(tris, skip_self=True)
    assert q.dtype == L().TRI_QUERY and (q["skip"] == np.arange(10)).all() and (q["b"] == tris["b"][:, :3]).all()
    q = host.tri_queries_from_mesh(positions(tris))
    assert (q["skip"] == NULL).all() and (q["c"] == tris["c"][:, :3]).all()
    rec = np.zeros(2, dtype=L().TRI_SEGMENT)
    rec["edges"] = [0x5031, 0x0001]
    passed, j0, j1 = host.segment_edges(rec)
    assert passed.tolist() == [[True, False, False, False, True, True], [True, False, False, False, False, False]]
    assert j0.tolist() == [0, 0] and j1.tolist() == [5, 0]


# ---- CPU: the restatement on pairs with known answers ------------------------------------------------------------------------
# Every coordinate is a dyadic number and every determinant a power of two, so each operation of the definition is exact and
# the expected points are exact too.

LARGE = [(-8, -8, 0), (24, -8, 0), (-8, 24, 0)]                # in the plane z = 0
SMALL = [(0, 0, -1), (0.5, 0, 1), (-0.5, 0.25, 1)]             # its edges a-b and c-a pass through the face of LARGE
FLAT = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]                       # in the plane z = 0
LINKED = [(1, 1, -1), (1, 1, 1), (9, 1, 1)]                    # in the plane y = 1: a-b through FLAT, FLAT's edge v1-v2 through it
THROUGH_EDGE = [(0, 1, -1), (0, 1, 1), (8, 1, 1)]              # its edge a-b passes through FLAT's edge v0-v2 at (0, 1, 0)
TINY = [(0, 0, 0), (2.0 ** -6, 0, 0), (0, 2.0 ** -6, 0)]
# a touches the face of TINY at t = 0 of a-b; c-a is all but parallel to the face (|det| = 2^-28 < 1e-8: rejected), b-c ends above it,
# and the plane y = 2^-8 of the query holds TINY's edge v0-v1 (det = 0) and is met by the two others outside the query
TOUCHING = [(2.0 ** -8, 2.0 ** -8, 0), (2.0 ** -8, 2.0 ** -8, 2.0 ** -8), (2.0 ** -7, 2.0 ** -8, 2.0 ** -16)]


def one_record(query, tri):
    q, t = np.array(query, dtype=F), np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    r = S.reference(T.make_queries(q[None, 0], q[None, 1], q[None, 2]), a, b, c, *padded_boxes(a, b, c))
    assert r.offsets.tolist() == [0, 1] and r.records["tri"][0] == 0
    return r.records[0]["p0"].tolist(), r.records[0]["p1"].tolist(), int(r.records[0]["edges"])


def test_reference_two_query_edges_through_a_face():
    assert one_record(SMALL, LARGE) == ([0.25, 0.0, 0.0], [-0.25, 0.125, 0.0], 0b000101 | (0 << 8) | (2 << 12))
    # the converse: the same two points from the scene triangle's edges v0-v1 (j = 3) and v0-v2 (j = 4)
    assert one_record(LARGE, SMALL) == ([0.25, 0.0, 0.0], [-0.25, 0.125, 0.0], 0b011000 | (3 << 8) | (4 << 12))


def test_reference_one_edge_of_each_through_the_other():
    assert one_record(LINKED, FLAT) == ([1.0, 1.0, 0.0], [3.0, 1.0, 0.0], 0b100001 | (0 << 8) | (5 << 12))


def test_reference_an_edge_through_an_edge_keeps_the_extremes():
    # j = 0 and j = 4 both give (0, 1, 0), j = 5 gives (3, 1, 0): three bits; the third point replaces p1, which came from j = 4
    p0, p1, edges = one_record(THROUGH_EDGE, FLAT)
    assert (p0, p1) == ([0.0, 1.0, 0.0], [3.0, 1.0, 0.0])
    assert edges == 0b110001 | (0 << 8) | (5 << 12) and bin(edges & 0x3F).count("1") >= 3


def test_reference_a_single_touching_test_has_equal_ends():
    p0, p1, edges = one_record(TOUCHING, TINY)
    assert p0 == p1 == [2.0 ** -8, 2.0 ** -8, 0.0] and edges == 0b000001


def test_running_pair_keeps_the_extremes_in_every_order():
    """six collinear points (dyadic steps along a dyadic direction: every distance is exact) in all 720 orders, and every subset of
    the tests passing in one order: the pair is the two extreme points of those that pass"""
    steps = np.array([0.0, 1.0, 2.0, 3.0, 5.0, 8.0])
    pts = (np.array([1.0, 2.0, 3.0]) + steps[:, None] * np.array([0.5, 0.25, -1.0])).astype(F)
    orders = np.array(list(itertools.permutations(range(6))))
    p0, p1, j0, j1 = S.running_pair(np.ones((720, 6), dtype=bool), pts[orders])
    k0, k1 = orders[np.arange(720), j0], orders[np.arange(720), j1]
    assert (p0 == pts[k0]).all() and (p1 == pts[k1]).all()
    assert (np.sort(np.stack([k0, k1], axis=1), axis=1) == [0, 5]).all()
    masks = np.array([[(m >> j) & 1 for j in range(6)] for m in range(1, 64)], dtype=bool)
    order = np.array([3, 0, 5, 1, 4, 2])
    p0, p1, j0, j1 = S.running_pair(masks, np.broadcast_to(pts[order], (63, 6, 3)))
    for m, mask in enumerate(masks):
        on = order[mask]
        assert sorted((order[j0[m]], order[j1[m]])) == [on.min(), on.max()] and mask[j0[m]] and mask[j1[m]]
        assert (p0[m] == pts[order[j0[m]]]).all() and (p1[m] == pts[order[j1[m]]]).all()
        if mask.sum() == 1:
            assert j0[m] == j1[m]
        elif mask.sum() == 2:
            assert (j0[m], j1[m]) == tuple(np.nonzero(mask)[0])          # the two points in the order of j


def test_the_parity_sets_are_not_vacuous():
    """Conditions on the REFERENCE alone: per set several hundred records with exactly two bits, some with more than two, some
    segments with more than one record, and both groups of tests among the ends."""
    for name in PARITY:
        a, b, c, q, r = cpu_case(name)
        bits = np.array([bin(int(e) & 0x3F).count("1") for e in r.records["edges"]])
        n = np.diff(r.offsets).astype(np.int64)
        passed, j0, j1 = H().segment_edges(r.records)
        print(f"{name}: {len(bits)} records, {int((bits == 1).sum())} / {int((bits == 2).sum())} / {int((bits > 2).sum())} with one / two / "
              f"more bits, {int((n > 1).sum())} segments with more than one record, longest {int(n.max())}")
        assert len(q) == COUNT and T.active(q).all()
        assert (bits >= 1).all() and (passed.sum(axis=1) == bits).all()
        assert (bits == 2).sum() >= 300 and (bits > 2).sum() > 0 and (n > 1).sum() > 0
        assert passed[np.arange(len(bits)), j0].all() and passed[np.arange(len(bits)), j1].all() and (j0 <= 5).all() and (j1 <= 5).all()
        assert (r.records["edges"] & ~np.uint32(0x773F) == 0).all()
        two = bits == 2
        assert (j0[two] < j1[two]).all() and (j1[two] < 3).any() and (j0[two] >= 3).any() and ((j0[two] < 3) & (j1[two] >= 3)).any()


# ---- CPU: the restatement against float64 geometry that shares no line with it ---------------------------------------------------

def plane_cut64(query, tri):
    """Moeller's interval construction in float64 for pairs given row by row ([n, 3, 3] vertices each): the line in which the two
    planes meet, each triangle's interval on it from the two edges that cross the other's plane, the overlap of the two intervals.
    -> (proper, lo point, hi point, lo j, hi j, cos lo, cos hi): proper = both triangles have vertices strictly on both sides of the
    other's plane and the overlap has positive length; j = the edge, in the header's numbering, that gave the end; cos = the cosine
    between that edge and the other triangle's normal."""
    q, t = np.asarray(query, dtype=np.float64), np.asarray(tri, dtype=np.float64)
    n = len(q)
    nq = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    nt = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    line = np.cross(nq, nt)
    hq = ((q - t[:, :1]) * nt[:, None]).sum(axis=2)              # heights of the query's vertices over the scene triangle's plane
    ht = ((t - q[:, :1]) * nq[:, None]).sum(axis=2)              # and the converse
    # the header's edges: j = 0, 1, 2 = a-b, b-c, c-a of the query; j = 3, 4, 5 = v0-v1, v0-v2, v1-v2 of the scene triangle
    ends = [(q, hq, nt, 0, 1), (q, hq, nt, 1, 2), (q, hq, nt, 2, 0), (t, ht, nq, 0, 1), (t, ht, nq, 0, 2), (t, ht, nq, 1, 2)]
    pts, par, cross, cos = [np.zeros((n, 6) + s) for s in ((3,), (), (), ())]
    with np.errstate(all="ignore"):
        for j, (v, h, normal, i, k) in enumerate(ends):
            w = h[:, i] / (h[:, i] - h[:, k])
            pts[:, j] = v[:, i] + (v[:, k] - v[:, i]) * w[:, None]
            par[:, j] = (pts[:, j] * line).sum(axis=1)
            cross[:, j] = h[:, i] * h[:, k] < 0
            edge = v[:, k] - v[:, i]
            cos[:, j] = np.abs((edge * normal).sum(axis=1)) / (np.linalg.norm(edge, axis=1) * np.linalg.norm(normal, axis=1))
    cross = cross.astype(bool)
    proper = (cross[:, :3].sum(axis=1) == 2) & (cross[:, 3:].sum(axis=1) == 2) & (hq != 0).all(axis=1) & (ht != 0).all(axis=1)
    big = np.where(cross, par, np.inf)
    small = np.where(cross, par, -np.inf)
    lo_q, lo_t = big[:, :3].argmin(axis=1), big[:, 3:].argmin(axis=1) + 3          # where each interval starts
    hi_q, hi_t = small[:, :3].argmax(axis=1), small[:, 3:].argmax(axis=1) + 3      # and ends
    rows = np.arange(n)
    lo_j = np.where(par[rows, lo_q] >= par[rows, lo_t], lo_q, lo_t)                # the overlap starts at the later start
    hi_j = np.where(par[rows, hi_q] <= par[rows, hi_t], hi_q, hi_t)                # and ends at the earlier end
    proper &= par[rows, hi_j] > par[rows, lo_j]
    return proper, pts[rows, lo_j], pts[rows, hi_j], lo_j, hi_j, cos[rows, lo_j], cos[rows, hi_j]


@pytest.mark.parametrize("name", PARITY)
def test_reference_against_float64_geometry(name):
    """Every record of the parity set against plane_cut64 (DESIGN section 38 has the derivation).  An end is P + D * t of an edge
    test; t is the height of P over the other triangle's plane divided by the edge's descent, so an error e in that height — at
    most section 34's band = K_EPS * 2^-24 * extent, the bound of a static test on these operations — moves the point along the
    edge by e / cos, cos the cosine between the edge and the other triangle's normal: the point error grows as the edge nears the
    plane.  The unordered pair {p0, p1} is compared with the float64 ends, each within band / cos of its edge.
    Left out, and counted, at most 1 % of the records: pairs for which float64 finds no proper segment (a triangle not strictly
    on both sides of the other's plane, an overlap of no length) and pairs whose passing tests are not exactly the two edges that
    give the float64 ends (the two disagree at a bound: an end within roundings of a vertex or of an edge of the other triangle).
    Measured, seed 11: grid_80x80 5 529 records, 48 left out (0.868 %), worst error 0.025 of its bound; cfg1_4096 899 records, 8 left out (0.890 %), worst error 0.025 of its bound."""
    a, b, c, q, r = cpu_case(name)
    band = K_EPS * 2.0 ** -24 * extent_of(a, b, c)
    rec, tri = r.records, r.records["tri"].astype(np.int64)
    query = np.stack([q["a"][r.rows], q["b"][r.rows], q["c"][r.rows]], axis=1)
    proper, lo, hi, lo_j, hi_j, cos_lo, cos_hi = plane_cut64(query, np.stack([a[tri], b[tri], c[tri]], axis=1))
    predicted = (np.uint32(1) << lo_j.astype(np.uint32)) | (np.uint32(1) << hi_j.astype(np.uint32))
    same_tests = (rec["edges"] & np.uint32(0x3F)) == predicted
    keep = proper & same_tests
    left_out = 1.0 - keep.mean()
    p0, p1 = rec["p0"].astype(np.float64), rec["p1"].astype(np.float64)
    dist = lambda x, y: np.linalg.norm(x - y, axis=1)
    with np.errstate(all="ignore"):
        straight = np.maximum(dist(p0, lo) * cos_lo, dist(p1, hi) * cos_hi)
        swapped = np.maximum(dist(p0, hi) * cos_hi, dist(p1, lo) * cos_lo)
    err = np.minimum(straight, swapped)                              # the worse end of the better matching, in units of its 1 / cos
    print(f"{name}: {len(rec)} records, {int((~keep).sum())} left out ({100.0 * left_out:.3f} %): {int((~proper).sum())} without a proper "
          f"float64 segment, {int((proper & ~same_tests).sum())} with other tests passing; worst error {err[keep].max() / band:.3f} of its bound")
    assert left_out <= 0.01
    assert (err[keep] <= band).all(), (np.nonzero(keep & (err > band))[0][:5], err[keep].max() / band)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def rec_words(records):
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 8)


class Queries:
    """device buffers of one query set; run() = one lbvh_triangle_intersection_segments call on caller-owned buffers"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer, self.count = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, max(len(queries), 1), L().TRI_QUERY)
        self.queries.local[:len(queries)] = queries
        self.queries.sync()
        self.offsets = H().DataBuffer(ctx, len(queries) + 1, np.uint64)
        self.flags = H().DataBuffer(ctx, max(len(queries), 1), np.uint32)

    def run(self, segments=None, capacity=None):
        """offsets (host copy) after one call; segments: a TRI_SEGMENT DataBuffer or None, capacity defaults to its size"""
        self.offsets.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        cap = 0 if segments is None else (segments.size if capacity is None else capacity)
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersection_segments(
            self.ctx.handle, self.queries.device, self.count, C.byref(s), self.offsets.device,
            segments.device if segments is not None else None, cap))
        return self.offsets.get_data().copy()

    def index_offsets(self):
        """the offsets lbvh_triangle_intersections writes for the same queries (count-only)"""
        self.offsets.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersections(self.ctx.handle, self.queries.device, self.count, C.byref(s),
                                                                       self.offsets.device, None, 0))
        return self.offsets.get_data().copy()

    def lists(self):
        """(offsets, records sorted by tri inside every segment) through count -> allocate -> fill"""
        off = self.run(None)
        total = int(off[self.count])
        buf = H().DataBuffer(self.ctx, max(total, 1), L().TRI_SEGMENT)
        try:
            off2 = self.run(buf)
            assert (off2 == off).all()
            return off[:self.count + 1], S.sort_segments(off[:self.count + 1], buf.get_data()[:total].copy())
        finally:
            buf.dispose()

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersects_any(self.ctx.handle, self.queries.device, self.count, C.byref(s), self.flags.device))
        return self.flags.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.queries, self.offsets, self.flags):
            b.dispose()


def assert_equal_records(got, ref, what=""):
    (go, gr), ro, rr = got, ref.offsets, ref.records
    assert (go[:len(ro)] == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gr) == len(rr) == int(ro[-1]), what
    bad = np.nonzero((rec_words(gr) != rec_words(rr)).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:10], gr[bad[:3]], rr[bad[:3]])


_GPU = {}


def gpu_case(ctx, name):
    """(a, b, c, lo, hi, queries, reference with the library's boxes, drawer): the reference once per scene; a context keeps one
    derived traversal scene, so it is derived again for the test that asks"""
    if name not in _GPU:
        tris = scene(name)
        a, b, c = positions(tris)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        q = parity_queries(a, b, c)
        _GPU[name] = (a, b, c, lo, hi, q, S.reference(q, a, b, c, lo, hi), d)
    _GPU[name][-1].build_fast_scene()
    return _GPU[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, name)
    q = Queries(ctx, d, queries)
    got = q.lists()
    assert (got[0] == q.index_offsets()[:COUNT + 1]).all()               # lbvh_triangle_intersections' offsets, word for word
    assert_equal_records(got, ref, name)
    # the public convenience of the drawer gives the same records
    off, rec = d.intersection_segments(q.queries, sort=True)
    assert_equal_records((off, rec), ref, "intersection_segments()")
    off, rec = d.intersection_segments(q.queries)
    assert_equal_records((off, S.sort_segments(off, rec)), ref, "intersection_segments(), host sort")
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129, 1500])
def test_t2_query_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[200:200 + count]
    r = S.reference(sub, a, b, c, lo, hi)
    assert count == 1 or int(r.offsets[-1]) > 0
    q = Queries(ctx, d, sub)
    assert_equal_records(q.lists(), r, count)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t2_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 queries on 1, 2, 3 or 7 waves: every lane refilled many times"""
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:1500].copy()
    sub["a"][100:235, 0] = np.nan                                    # a block of inactive queries inside a run
    r = S.reference(sub, a, b, c, lo, hi)
    q = Queries(ctx, d, sub)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        got = q.lists()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal_records(got, r, waves)
    q.dispose()


@pytest.mark.gpu
def test_t3_a_mesh_against_itself(ctx):
    a, b, c, lo, hi, _, _, d = gpu_case(ctx, "cfg1_4096")
    queries = H().tri_queries_from_mesh((a, b, c), skip_self=True)
    r = S.reference(queries, a, b, c, lo, hi)
    assert int(r.offsets[-1]) > 0
    q = Queries(ctx, d, queries)
    off, rec = q.lists()
    assert_equal_records((off, rec), r)
    own = np.repeat(np.arange(len(a), dtype=np.uint32), np.diff(off).astype(np.int64))
    assert (rec["tri"] != own).all()                                    # no record carries tri == skip
    q.dispose()


@pytest.mark.gpu
def test_t4_inactive_queries_among_active_ones(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:540].copy()
    bad = (F(np.nan), F(np.inf), F(-np.inf))
    for j, (vertex, axis) in enumerate((v, x) for v in "abc" for x in range(3)):
        for m, value in enumerate(bad):
            sub[vertex][5 + 20 * (3 * j + m), axis] = value             # 27 inactive queries, each between active neighbours
    sub["_pad0"], sub["_pad1"] = 0x7FC00000, 0xFFFFFFFF                  # not read
    act = T.active(sub)
    assert (~act).sum() == 27
    r = S.reference(sub, a, b, c, lo, hi)
    q = Queries(ctx, d, sub)
    off, rec = q.lists()
    assert_equal_records((off, rec), r)
    assert (np.diff(off)[~act] == 0).all()
    # the neighbours are what they were in the full set
    full = np.diff(ref.offsets)[:540]
    assert (np.diff(off)[act] == full[act]).all() and np.diff(off)[act].sum() > 0
    q.dispose()


@pytest.mark.gpu
def test_t5_count_only_overflow_and_two_calls(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    total = int(ref.offsets[-1])
    q = Queries(ctx, d, queries)
    assert (q.run(None) == ref.offsets).all()                            # capacity == 0, d_segments == NULL
    # one record short: the capacity cuts through the last non-empty segment
    cap, guard = total - 1, 512
    last_seg = int(np.nonzero(np.diff(ref.offsets))[0][-1])
    assert int(ref.offsets[last_seg]) <= cap < int(ref.offsets[last_seg + 1]) == total
    buf = H().DataBuffer(ctx, total + guard, L().TRI_SEGMENT)
    buf.fill_u32(0xABABABAB)
    off = q.run(buf, capacity=cap)
    got = buf.get_data().copy()
    assert (off == ref.offsets).all() and int(off[-1]) == total
    assert (rec_words(got[cap:]) == 0xABABABAB).all()                    # no word at the capacity or beyond
    fits = int(ref.offsets[last_seg])                                    # every segment before the last non-empty one fits
    assert fits > 0
    assert (rec_words(S.sort_segments(ref.offsets[:last_seg + 1], got[:fits])) == rec_words(ref.records[:fits])).all()
    # the retry with what the offsets asked for, twice: the same bytes
    buf.fill_u32(0xABABABAB)
    off = q.run(buf, capacity=total)
    first = buf.get_data().copy()
    assert (rec_words(first[total:]) == 0xABABABAB).all()
    assert_equal_records((off, S.sort_segments(off, first[:total])), ref)
    buf.fill_u32(0xCDCDCDCD)
    q.run(buf, capacity=total)
    assert (rec_words(buf.get_data()[:total]) == rec_words(first[:total])).all()
    buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t6_count_zero_rejections_and_a_stale_scene():
    """the rows test_query_entry_contract.py has for the other entry points, for this one: on a context of its own"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        k = rng.integers(0, 64, 130)
        shift = rng.normal(size=(130, 1, 3)).astype(F)
        pts = np.stack([a[k], b[k], c[k]], axis=1) + shift
        queries = T.make_queries(pts[:, 0], pts[:, 1], pts[:, 2])
        ref = S.reference(queries, a, b, c, lo, hi)
        assert 0 < int((np.diff(ref.offsets) > 0).sum()) < 130
        q = Queries(ctx, d, queries)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, L().TRI_SEGMENT)
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        call = lib.lbvh_triangle_intersection_segments
        dq, do, dl = q.queries.device, q.offsets.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, lst)

        def poison():
            for buf in bufs:
                buf.fill_u32(0x7FC0DEAD)

        def untouched():
            return all((words(buf.get_data()) == 0x7FC0DEAD).all() for buf in bufs)

        poison()
        assert call(h, dq, 0, C.byref(s), do, dl, 64) == 0                                             # count == 0: a no-op
        for args in ((None, 10, C.byref(s), do, None, 0), (dq, 10, None, do, None, 0), (dq, 10, C.byref(s), None, None, 0),
                     (dq, 10, C.byref(s), do, None, 5), (at(q.queries, 4), 10, C.byref(s), do, None, 0),
                     (dq, 10, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, C.byref(s), do, at(lst, 4), 8),
                     (dq, 10, C.byref(s), do, at(lst, 8), 8), (dq, 1 << 32, C.byref(s), do, None, 0)):
            assert call(h, *args) == -1, args
            assert lib.lbvh_last_error(h)
        assert call(None, dq, 10, C.byref(s), do, None, 0) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        assert call(h, dq, 130, C.byref(s), do, None, 0) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_triangle_intersection_segments: ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        # aligned sub-ranges are fine; the plain and the counting instantiation write the same words, and the latter counts
        assert call(h, at(q.queries, 48), 10, C.byref(s), at(q.offsets, 8), at(lst, 32), 8) == 0
        stats.fill_u32(0x7FC0DEAD)
        plain = q.lists()
        assert (words(stats.get_data()) == 0x7FC0DEAD).all()
        assert_equal_records(plain, ref)
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            counted = q.lists()
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        st = stats.get_data()[0]
        assert_equal_records(counted, ref)
        assert st["rays"] > 0 and st["node_fetches"] > 0 and st["triangle_tests"] > 0, st
        for buf in (lst, stats):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t7_a_small_lds_stack_and_the_statistics(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    q = Queries(ctx, d, queries)
    h, lib = ctx.handle, N().lib
    # a small LDS part exercises the device-memory part of the stack: the same records
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        got = q.lists()
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert_equal_records(got, ref, "stack split 1")
    # statistics: the fill walk reads the triangle lines the count walk reads
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    big = H().DataBuffer(ctx, max(int(ref.offsets[-1]), 1), L().TRI_SEGMENT)
    seen = []
    try:
        for form in ("count", "full"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            q.run(big if form == "full" else None)
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("rays, node fetches, triangle tests: count-only %s, full %s" % tuple(seen))
    assert seen[0][2] > 0 and seen[1] == tuple(2 * x for x in seen[0])
    for buf in (stats, big):
        buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t8_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver trisegs 2000 5`: TriangleIntersectionSegments of lbvh_host.hpp on the driver's own mesh and queries, against the
    reference on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "trisegs", str(count), "5"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    r = S.reference(T.make_queries(*T.driver_triangles(lo, hi, count, seed=5)), a, b, c, *library_boxes(d))
    d.on_destroy()
    n = np.diff(r.offsets).astype(np.int64)
    offset_sum, record_sum = S.checksums(r.offsets, r.records)
    two_ends = int((((r.records["edges"] >> 8) & 7) != ((r.records["edges"] >> 12) & 7)).sum())
    assert int(r.offsets[-1]) > 0
    assert (res["triangles"], res["queries"], res["total"], res["non_empty"], res["two_ends"], res["offset_sum"], res["record_sum"]) == \
        (4096, count, int(r.offsets[-1]), int((n > 0).sum()), two_ends, offset_sum, record_sum)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t9_non_empty_exactly_where_any_says_so(ctx, name):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, name)
    q = Queries(ctx, d, queries)
    off = q.run(None)
    flags = q.any()
    assert ((np.diff(off[:COUNT + 1]) > 0) == (flags == 1)).all() and set(np.unique(flags)) <= {0, 1} and flags.sum() > 0
    q.dispose()
