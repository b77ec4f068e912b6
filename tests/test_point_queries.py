"""lbvh_closest_point_query / lbvh_within_distance: the nearest triangle of a point and "anything within r", over the four-wide
derived traversal scene.  The expectation is tests/point_reference.py: the header's definition in numpy float32, brute force over
every (query, triangle) pair with the triangles' own boxes as the library produced them — no tree.  Every GPU comparison is word
for word:
  P1  lbvh_closest_point_query == reference records
  P2  lbvh_within_distance == (the reference has a candidate)
and on the P1 / P2 sets the reference's box rule rejects nothing (asserted), so the rule does not carry those tests; a separate
case constructs rejections by shrinking a few triangles' boxes."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import point_reference as R
from query_support import (driver_mesh, driver_points, golden, H, L, library_boxes, make_queries, _mixed_points, mixed_queries,
                           N, padded_boxes, positions, words)
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def _header():
    return open(os.path.join(ROOT, "include", "lbvh.h")).read()


def test_header_declares_both_records_and_both_queries():
    h = _header()
    m = re.search(r"typedef struct lbvh_point_query \{(.*?)\} lbvh_point_query;", h, re.S)
    assert m and re.findall(r"float\s+(\w+)", m.group(1)) == ["p", "max_dist2"]
    m = re.search(r"typedef struct lbvh_closest_point \{(.*?)\} lbvh_closest_point;", h, re.S)
    assert m and re.findall(r"\b(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)) == ["dist2", "tri", "u", "v"]
    for fn, out in (("lbvh_closest_point_query", r"lbvh_closest_point\* d_out"), ("lbvh_within_distance", r"uint32_t\* d_flags")):
        assert re.search(r"lbvh_status " + fn + r"\(lbvh_context\* ctx, const lbvh_point_query\* d_queries, size_t count, "
                         r"const lbvh_scene\* h_scene,\s+" + out + r"\);", h), fn


def test_layouts():
    lay = L()
    assert lay.POINT_QUERY.itemsize == 16 and lay.CLOSEST_POINT.itemsize == 16
    assert [lay.POINT_QUERY.fields[k][1] for k in ("p", "max_dist2")] == [0, 12]
    assert [lay.CLOSEST_POINT.fields[k][1] for k in ("dist2", "tri", "u", "v")] == [0, 4, 8, 12]
    assert lay.CLOSEST_POINT.fields["tri"][0] == np.dtype("<u4")
    assert lay.POINT_QUERY is R.POINT_QUERY and lay.CLOSEST_POINT is R.CLOSEST_POINT and R.MAX_FLOAT == lay.MAX_FLOAT


def test_native_prototypes():
    nat = N()
    for fn in ("lbvh_closest_point_query", "lbvh_within_distance"):
        res, args = nat.SIGNATURES[fn]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
        assert getattr(nat.lib, fn).argtypes is not None


def test_csharp_structs_have_the_c_field_order():
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public struct PointQuery \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["pX", "pY", "pZ", "maxDist2"]
    m = re.search(r"public struct ClosestPoint \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["dist2", "tri", "u", "v"]
    assert re.search(r"public uint tri;", m.group(1))
    for fn in ("lbvh_closest_point_query", "lbvh_within_distance"):
        assert re.search(r"public static extern int " + fn + r"\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+\);", cs)
    pq = open(os.path.join(ROOT, "bindings", "csharp", "PointQueries.cs")).read()
    assert "lbvh_closest_point_query" in pq and "lbvh_within_distance" in pq and "unsafe" not in pq
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void ClosestPoints(" in hpp and "void WithinDistance(" in hpp


# ---- CPU: the restatement against float64 and against cases with known answers ---------------------------------------------

@pytest.mark.parametrize("name", ["viking_room", "example_object3"])
def test_reference_agrees_with_its_float64_evaluation(name):
    """Nearest distance: |sqrt(d32) - sqrt(d64)| <= 64 * 2^-24 * extent, d64 the same definition in float64 on the same fp32
    inputs, extent the largest side of the scene's box.
    Why a bound of this form: every quantity of the definition is a sum of three products of coordinate differences, so the
    rounding error of dist2 is a few units of 2^-24 * extent^2 and a distance inherits a few units of 2^-24 * extent.
    Measured while the definition was written (1500 points per scene): viking_room (extent 1.5) worst 1.1e-6 = 12 * 2^-24 *
    extent; example_object3 (extent 8) 1.0e-7 = 0.2 units; 4096 random triangles (extent 204) 3.1e-5 = 2.6 units.  The bound
    leaves a factor 5 over the worst of them; the test prints what it measures."""
    a, b, c = positions(golden(name))
    rng = np.random.default_rng(11)
    pts = _mixed_points(a, b, c, 600, rng)
    d32 = R.nearest_dist2(pts, a, b, c, np.float32)
    d64 = R.nearest_dist2(pts, a, b, c, np.float64)
    lo, hi = padded_boxes(a, b, c)
    extent = float((hi.max(axis=0) - lo.min(axis=0)).max())
    err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64))
    print(f"{name}: extent {extent:.4g} worst |d32 - d64| {err.max():.3g} = {err.max() / (2.0 ** -24 * extent):.2f} * 2^-24 * extent")
    assert err.max() <= 64 * 2.0 ** -24 * extent
    # the brute force with rule and radius, unbounded: the same minimum, and nothing rejected
    ref = R.reference(make_queries(pts, INF), a, b, c, lo, hi)
    assert ref.rejected == 0 and ref.flags.all()
    assert (words(ref.records["dist2"]) == words(d32)).all()


def _one(tri_abc, p, r2=INF, boxes=None):
    a, b, c = (np.asarray(x, dtype=F).reshape(-1, 3) for x in tri_abc)
    lo, hi = boxes if boxes is not None else padded_boxes(a, b, c)
    q = make_queries(np.asarray(p, dtype=F).reshape(-1, 3), r2)
    return R.reference(q, a, b, c, lo, hi)


def test_known_answers_for_every_region():
    tri = ([[0, 0, 0]], [[4, 0, 0]], [[0, 4, 0]])            # a, b, c: right triangle in z = 0
    cases = [((1, 1, 3), 9.0, (0.25, 0.25)),                 # above the face interior
             ((2, -2, 0), 4.0, (0.5, 0.0)),                  # beyond edge ab
             ((-3, 1, 0), 9.0, (0.0, 0.25)),                 # beyond edge ac
             ((3, 3, 0), 2.0, (0.5, 0.5)),                   # beyond edge bc
             ((-1, -2, 2), 9.0, (0.0, 0.0)),                 # beyond vertex a
             ((7, -1, 0), 10.0, (1.0, 0.0)),                 # beyond vertex b
             ((-1, 6, 1), 6.0, (0.0, 1.0)),                  # beyond vertex c
             ((1, 2, 0), 0.0, (0.25, 0.5))]                  # on the face
    for p, d2, (u, v) in cases:
        r = _one(tri, [p])
        rec = r.records[0]
        assert r.flags[0] == 1 and r.rejected == 0
        assert (rec["dist2"], rec["tri"], rec["u"], rec["v"]) == (F(d2), 0, F(u), F(v)), p


def test_ties_go_to_the_lowest_index_and_the_radius_is_strict():
    # a fan of four triangles around the shared vertex (1, 1, 1), the query exactly on it: four distances of 0
    s = np.array([1, 1, 1], dtype=F)
    a = np.tile(s, (4, 1))
    b = s + np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], dtype=F)
    c = s + np.array([[0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, 0, 0]], dtype=F)
    r = _one((a, b, c), [s])
    assert r.records[0]["tri"] == 0 and r.records[0]["dist2"] == 0 and r.flags[0] == 1
    r = _one((a[::-1], b[::-1], c[::-1]), [s + np.array([0, 0, 2], dtype=F)])         # any order: still the lowest index
    assert r.records[0]["tri"] == 0 and r.records[0]["dist2"] == F(4.0)
    # strict radius: max_dist2 just below / equal to / just above the true dist2 = 4
    p = np.tile(s + np.array([0, 0, 2], dtype=F), (7, 1))
    r2 = np.array([np.nextafter(F(4), F(0)), 4.0, np.nextafter(F(4), INF), np.inf, R.MAX_FLOAT, 0.0, -1.0], dtype=F)
    r = _one((a, b, c), p, r2)
    assert r.flags.tolist() == [0, 0, 1, 1, 1, 0, 0]
    none = words(np.array([R.NONE]))
    assert (words(r.records[[0, 1, 5, 6]]).reshape(-1, 4) == none).all()
    assert (r.records["dist2"][[2, 3, 4]] == F(4.0)).all() and (r.records["tri"][[2, 3, 4]] == 0).all()
    # inactive: NaN radius; a NaN coordinate has no candidate either
    r = _one((a, b, c), [s, [np.nan, 0, 0]], np.array([np.nan, np.inf], dtype=F))
    assert r.flags.tolist() == [0, 0] and (words(r.records).reshape(-1, 4) == none).all()


def test_box_rule_rejects_a_distance_in_front_of_the_own_box():
    tri = ([[0, 0, 0], [0, 0, 5]], [[4, 0, 0], [4, 0, 5]], [[0, 4, 0], [0, 4, 5]])
    a, b, c = (np.asarray(x, dtype=F) for x in tri)
    lo, hi = padded_boxes(a, b, c)
    p = [[1, 1, 1]]
    assert _one(tri, p).records[0]["tri"] == 0
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[0], hi2[0] = [3.0, 3.0, -0.001], [3.5, 3.5, 0.001]            # triangle 0's box moved away from the query: box2 > dist2 = 1
    r = _one(tri, p, boxes=(lo2, hi2))
    assert r.rejected == 1 and r.records[0]["tri"] == 1 and r.records[0]["dist2"] == F(16.0)
    r = _one(tri, p, r2=F(10.0), boxes=(lo2, hi2))
    assert r.rejected == 1 and r.flags[0] == 0


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Points:
    """device buffers for one query set and the two calls"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer = ctx, drawer
        self.queries = H().DataBuffer(ctx, len(queries), L().POINT_QUERY)
        self.queries.local[:] = queries
        self.queries.sync()
        self.out = H().DataBuffer(ctx, len(queries), L().CLOSEST_POINT)
        self.flags = H().DataBuffer(ctx, len(queries), np.uint32)

    def closest(self):
        self.out.fill_u32(0x7FC00000)
        self.drawer.closest_points(self.queries, self.out)
        return self.out.get_data().copy()

    def within(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.within_distance(self.queries, self.flags)
        return self.flags.get_data().copy()

    def dispose(self):
        for b in (self.queries, self.out, self.flags):
            b.dispose()


def _scene(name):
    if name == "random":
        return scenes.random_triangles(4096)
    if name == "grid":
        return scenes.grid_scene()
    return golden(name)


_CASES = {}


def parity_case(ctx, name):
    """(triangles, queries, reference result, unbounded reference, drawer): the reference is computed once per scene; one context
    keeps one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _CASES:
        tris = _scene(name)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        a, b, c = positions(tris)
        lo, hi = library_boxes(d)
        queries, unb = mixed_queries(a, b, c, lo, hi, 1500, 5 + len(tris))
        _CASES[name] = (tris, queries, R.reference(queries, a, b, c, lo, hi), unb, d)
    _CASES[name][4].build_fast_scene()
    return _CASES[name]


SCENES = ["random", "grid", "example_object3", "viking_room"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_p1_closest_point_equals_the_brute_force_word_for_word(ctx, name):
    tris, queries, ref, unb, d = parity_case(ctx, name)
    assert len(queries) >= 1500
    assert ref.rejected == 0 and unb.rejected == 0                     # the box rule does not carry this test
    q = Points(ctx, d, queries)
    got = q.closest()
    bad = np.nonzero((words(got).reshape(-1, 4) != words(ref.records).reshape(-1, 4)).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], got[bad[:3]], ref.records[bad[:3]], queries[bad[:3]])
    q.dispose()
    # what the set exercised: the strict radius on both sides, inactive queries, both unbounded forms
    act = R.active(queries)
    du = unb.records["dist2"]
    at = act & (queries["max_dist2"] == du)
    above = act & (queries["max_dist2"] == np.nextafter(du, INF))
    print(f"{name}: {int(act.sum())} active, {int(at.sum())} with R == d, {int(above.sum())} with R one ulp above d, "
          f"{int((got['dist2'] < R.MAX_FLOAT).sum())} found")
    assert at.sum() > 20 and (got["dist2"][at] == R.MAX_FLOAT).all() and (got["tri"][at] == 0).all()
    assert above.sum() > 50 and (words(got[above]) == words(unb.records[above])).all()
    assert (~act).sum() > 300 and (words(got[~act]).reshape(-1, 4) == words(np.array([R.NONE]))).all()
    for r in (INF, R.MAX_FLOAT):
        sel = queries["max_dist2"] == r
        assert sel.sum() > 100 and (words(got[sel]) == words(unb.records[sel])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_p2_within_distance_equals_the_reference_having_a_candidate(ctx, name):
    tris, queries, ref, unb, d = parity_case(ctx, name)
    assert ref.rejected == 0
    q = Points(ctx, d, queries)
    flags = q.within()
    assert (flags == ref.flags).all(), np.nonzero(flags != ref.flags)[0][:10]
    assert 0 < flags.sum() < R.active(queries).sum()
    q.dispose()


@pytest.mark.gpu
def test_constructed_box_rule_rejections(ctx):
    """A few triangles' boxes shrunk about their centres after the Morton stage and the sort, the derived scene built from them:
    those triangles' own boxes no longer reach their corners, so for points near the corners dist2 < box2 and the triangle does
    not count.  GPU == reference fed the same boxes, the reference counts rejections, and answers differ from the untouched scene's."""
    tris = scenes.random_triangles(n=3000, seed=21, extent=30.0, edge=6.0)
    a, b, c = positions(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    n = len(tris)
    lo0, hi0 = library_boxes(d)
    rng = np.random.default_rng(3)
    picked = rng.choice(n, 60, replace=False)
    # queries: the corners and surface points of the picked triangles, and points all over the scene
    w = rng.dirichlet((1, 1, 1), 600)
    k = picked[rng.integers(0, len(picked), 600)]
    pts = np.concatenate([a[picked], b[picked], c[picked], a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:],
                          rng.uniform(lo0.min(axis=0), hi0.max(axis=0), (800, 3))]).astype(F)
    r2 = np.where(rng.random(len(pts)) < 0.5, INF, F(4.0)).astype(F)
    queries = make_queries(pts, r2)[rng.permutation(len(pts))]
    before = R.reference(queries, a, b, c, lo0, hi0)
    q = Points(ctx, d, queries)
    assert before.rejected == 0 and (words(q.closest()) == words(before.records)).all()
    box = d.container.triangle_aabb.local                              # the mirror get_data() filled, all `capacity` entries
    centre = (box["min"][picked] + box["max"][picked]) * F(0.5)
    half = (box["max"][picked] - box["min"][picked]) * F(0.05)
    box["min"][picked] = centre - half
    box["max"][picked] = centre + half
    d.container.triangle_aabb.sync()
    d.build_fast_scene()
    lo1, hi1 = box["min"][:n].copy(), box["max"][:n].copy()
    ref = R.reference(queries, a, b, c, lo1, hi1)
    got, flags = q.closest(), q.within()
    assert ref.rejected > 0
    assert (words(got) == words(ref.records)).all()
    assert (flags == ref.flags).all()
    changed = (words(ref.records).reshape(-1, 4) != words(before.records).reshape(-1, 4)).any(axis=1)
    print(f"box rule: {ref.rejected} pairs rejected, {int(changed.sum())} of {len(queries)} answers changed, "
          f"{int((ref.flags != before.flags).sum())} flags changed")
    assert changed.sum() > 0 and (ref.flags != before.flags).sum() > 0
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
def test_both_build_paths_animation_and_a_stale_scene(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres)
    d = pt.drawer
    a, b, c = positions(tris)
    rng = np.random.default_rng(8)
    pts = _mixed_points(a, b, c, 1200, rng)[rng.permutation(1200)]
    queries = make_queries(pts, np.where(rng.random(1200) < 0.5, INF, F(9.0)).astype(F))
    q = Points(ctx, d, queries)
    lo, hi = library_boxes(d)
    ref = R.reference(queries, a, b, c, lo, hi)
    for staged in (False, True):                                       # lbvh_build_scene(LBVH_BUILD_FAST_SCENE) / the staged calls
        d.rebuild(fast=True, staged=staged)
        assert (words(q.closest()) == words(ref.records)).all(), staged
        assert (q.within() == ref.flags).all(), staged
    pt.animate(0.4)                                                    # lbvh_animate_build_scene: moved geometry, new answers
    moved = d.container.triangle_data.get_data()[: len(tris)]
    a2, b2, c2 = positions(moved)
    lo2, hi2 = library_boxes(d)
    ref2 = R.reference(queries, a2, b2, c2, lo2, hi2)
    got = q.closest()
    assert (words(got) == words(ref2.records)).all() and (q.within() == ref2.flags).all()
    assert (words(ref2.records).reshape(-1, 4) != words(ref.records).reshape(-1, 4)).any(axis=1).sum() > 300
    assert ref.rejected == 0 and ref2.rejected == 0
    # a stale scene: triangles uploaded without a rebuild
    lib, h, s = N().lib, ctx.handle, d.container.scene()
    d.container.triangle_data.sync()
    for fn, out in ((lib.lbvh_closest_point_query, q.out), (lib.lbvh_within_distance, q.flags)):
        assert fn(h, q.queries.device, len(queries), C.byref(s), out.device) == -1
        assert b"stale" in lib.lbvh_last_error(h)
    d.rebuild(fast=True)
    assert (words(q.closest()) == words(ref2.records)).all()
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
def test_statistics_count_active_queries_and_within_never_walks_more(ctx):
    tris, queries, ref, unb, d = parity_case(ctx, "random")
    lay = L()
    for bounded in (False, True):
        qs = queries.copy()
        if not bounded:
            qs["max_dist2"] = np.where(R.active(qs), INF, qs["max_dist2"])
        q = Points(ctx, d, qs)
        stats = H().DataBuffer(ctx, 1, lay.RAY_STATS)
        per = {}
        try:
            for call in ("closest", "within"):
                stats.fill_u32(0)
                N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
                getattr(q, call)()
                N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
                per[call] = stats.get_data()[0].copy()
        finally:
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
        n_active = int(R.active(qs).sum())
        cl, wi = per["closest"], per["within"]
        print(f"bounded={bounded}: active {n_active}, closest {int(cl['node_fetches'])} lines {int(cl['triangle_tests'])} tests, "
              f"within {int(wi['node_fetches'])} lines {int(wi['triangle_tests'])} tests")
        assert int(cl["rays"]) == n_active and int(wi["rays"]) == n_active
        assert int(wi["node_fetches"]) <= int(cl["node_fetches"]) and int(wi["triangle_tests"]) <= int(cl["triangle_tests"])
        assert int(cl["node_fetches"]) >= n_active                     # every active query fetches the root line at least
        stats.dispose()
        q.dispose()


@pytest.mark.gpu
def test_errors_scratch_failure_and_the_stack_limit(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        rng = np.random.default_rng(2)
        queries = make_queries(_mixed_points(a, b, c, 3000, rng), INF)
        lo, hi = library_boxes(d)
        ref = R.reference(queries, a, b, c, lo, hi)
        q = Points(c2, d, queries)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(queries)
        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
        q.out.fill_u32(0x7FC00000)
        assert lib.lbvh_closest_point_query(h, q.queries.device, n, C.byref(s), q.out.device) == -2
        assert (words(q.out.get_data()) == 0x7FC00000).all()
        assert (words(q.closest()) == words(ref.records)).all()
        assert (q.within() == ref.flags).all()
        # argument checks
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        for fn, out, bad in ((lib.lbvh_closest_point_query, q.out, 8), (lib.lbvh_within_distance, q.flags, 2)):
            assert fn(h, None, n, C.byref(s), out.device) == -1
            assert fn(h, q.queries.device, n, None, out.device) == -1
            assert fn(h, q.queries.device, n, C.byref(s), None) == -1
            assert fn(h, p(q.queries, 16), 10, C.byref(s), out.device) == 0        # queries 1 .. 10: 16-byte aligned
            assert fn(h, p(q.queries, 4), 10, C.byref(s), out.device) == -1
            assert fn(h, q.queries.device, 10, C.byref(s), p(out, bad)) == -1
            assert fn(h, q.queries.device, 1 << 32, C.byref(s), out.device) == -1
            assert fn(None, q.queries.device, 10, C.byref(s), out.device) == -1
        # count == 0: a no-op, the outputs untouched
        q.out.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        assert lib.lbvh_closest_point_query(h, q.queries.device, 0, C.byref(s), q.out.device) == 0
        assert lib.lbvh_within_distance(h, q.queries.device, 0, C.byref(s), q.flags.device) == 0
        assert (words(q.out.get_data()) == 0x7FC00000).all() and (q.flags.get_data() == 0xDEADBEEF).all()
        # a small LDS part exercises the device-memory part of the stack: same records
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        assert (words(q.closest()) == words(ref.records)).all() and (q.within() == ref.flags).all()
        # the stack limit: a reported error (LBVH_ERR_HIP at the next sync), never a silently wrong record
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        q.drawer.closest_points(q.queries, q.out)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert (words(q.closest()) == words(ref.records)).all()
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_path_tracer_frame_undisturbed_by_point_queries_between_bounces(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    # the same frame with both queries issued between the bounces, 4x the frame's count: the ray scratch grows in mid-frame
    a, b, c = positions(tris)
    queries = make_queries(_mixed_points(a, b, c, 4 * 160 * 96, np.random.default_rng(12)), F(25.0))
    q = Points(ctx, pt.drawer, queries)
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def both():
        pt.drawer.closest_points(q.queries, q.out)
        pt.drawer.within_distance(q.queries, q.flags)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    both()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        both()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    both()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    assert 0 < q.flags.get_data().sum() < len(queries)
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
def test_scale_one_million_triangles_one_million_queries(ctx):
    """cfg2's mesh, 2^20 queries (half uniform in the grown box, half on surfaces; a quarter with a finite radius).  Every record:
    dist2, u, v equal the reference on the reported triangle alone, and no candidate among 64 random triangles per block of 4096
    queries is nearer.  128 fixed queries: the full brute force, word for word."""
    tris = scenes.tiled_torus()
    n = len(tris)
    a, b, c = positions(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    count = 1 << 20
    rng = np.random.default_rng(44)
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    ext = shi - slo
    pts = rng.uniform(slo - 0.25 * ext, shi + 0.25 * ext, (count, 3)).astype(F)
    k = rng.integers(0, n, count // 2)
    w = rng.dirichlet((1, 1, 1), count // 2).astype(F)
    pts[1::2] = a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
    r2 = np.where(rng.random(count) < 0.25, F(4.0), INF).astype(F)
    queries = make_queries(pts, r2)
    q = Points(ctx, d, queries)
    got, flags = q.closest(), q.within()
    q.dispose()
    d.on_destroy()
    found = got["dist2"] < R.MAX_FLOAT
    assert (flags == found).all() and found.sum() > count // 2
    assert (words(got[~found]).reshape(-1, 4) == words(np.array([R.NONE]))).all()
    # the record against the reference on the reported triangle alone
    t = got["tri"][found]
    dd, uu, vv = R.point_triangle(pts[found], a[t], (b - a)[t], (c - a)[t])
    assert (words(dd) == words(got["dist2"][found])).all() and (words(uu) == words(got["u"][found])).all() \
        and (words(vv) == words(got["v"][found])).all()
    assert (got["dist2"][found] < R.radius2(queries)[found]).all()
    assert not (dd < R.box_dist2(pts[found], lo[t], hi[t])).any()
    # nothing nearer among sampled triangles
    best = np.where(found, got["dist2"], R.radius2(queries))           # none found: no candidate below R
    for s in range(0, count, 4096):
        sample = rng.integers(0, n, 64)
        p = pts[s:s + 4096, None, :]
        ds, _, _ = R.point_triangle(p, a[sample][None], (b - a)[sample][None], (c - a)[sample][None])
        own = R.box_dist2(p, lo[sample][None], hi[sample][None])
        ds = np.where(ds < own, INF, ds)
        assert not (ds < best[s:s + 4096, None]).any(), s
    # 128 fixed queries: brute force over all the triangles
    sub = np.arange(128) * (count // 128) + np.arange(128) % 2         # both kinds of points
    ref = R.reference(queries[sub], a, b, c, lo, hi)
    assert ref.rejected == 0
    assert (words(got[sub]) == words(ref.records)).all() and (flags[sub] == ref.flags).all()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [None, 3.0])
def test_cpp_host_driver_points_matches_the_python_host(ctx, radius):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    n, count = 4096, 20000
    args = [exe, "points", str(n), str(count)] + ([str(radius)] if radius is not None else [])
    res = json.loads(subprocess.run(args, check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(n)                                   # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    pts = driver_points(lo, hi, count)                                 # and its points (seed 2)
    queries = make_queries(pts, INF if radius is None else F(radius) * F(radius))
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Points(ctx, d, queries)
    got, flags = q.closest(), q.within()
    assert res["triangles"] == n and res["points"] == count
    assert res["found"] == int((got["dist2"] < R.MAX_FLOAT).sum()) and res["within"] == int(flags.sum())
    assert res["word_sum"] == int(words(got).astype(np.uint64).sum())
    assert res["found"] == count if radius is None else 0 < res["found"] < count
    q.dispose()
    d.on_destroy()
