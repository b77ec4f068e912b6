"""lbvh_k_closest_points: the k nearest triangles of a point, over the four-wide derived traversal scene.  The expectation is
tests/k_closest_reference.py: point_reference's distances and candidate predicate, per query a stable sort on dist2 over the
triangles in index order, the first k, padded with none-records.  Every GPU comparison is word for word on uint32 views, no
tolerance, no case left out.  Scenes and query sets are those of tests/test_point_queries.py, built by the same code (copied
here, not imported from the test file)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import k_closest_reference as K
import point_reference as R
from query_support import (assert_rows, driver_mesh, driver_points, golden, H, L, library_boxes, make_queries, _mixed_points,
                           mixed_queries, N, pack, padded_boxes, positions, row_words, words)
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
KMAX = 32
KS = [1, 2, 5, 8, 32]


NONE_WORDS = words(np.array([R.NONE]))


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_the_macro_and_the_prototype():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"#define LBVH_K_CLOSEST_MAX 32\b", h)
    assert re.search(r"lbvh_status lbvh_k_closest_points\(lbvh_context\* ctx, const lbvh_point_query\* d_queries, size_t count, uint32_t k,\s+"
                     r"const lbvh_scene\* h_scene, lbvh_closest_point\* d_out, uint32_t\* d_found\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_k_closest_points" in bounce                               # listed among the calls that drop the live-path list


def test_native_signature_has_seven_arguments():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_k_closest_points"]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[3] is C.c_uint32
    assert nat.lib.lbvh_k_closest_points.argtypes is not None
    assert nat.K_CLOSEST_MAX == 32


def test_csharp_import_wrapper_and_cpp_host():
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public static extern int lbvh_k_closest_points\((.*?)\);", cs, re.S)
    assert m and len(m.group(1).split(",")) == 7
    assert re.match(r"IntPtr ctx, IntPtr \w+, UIntPtr count, uint k, ref Scene scene, IntPtr \w+,\s+IntPtr \w+$", m.group(1))
    kc = open(os.path.join(ROOT, "bindings", "csharp", "KClosestPoints.cs")).read()
    assert "lbvh_k_closest_points" in kc and "unsafe" not in kc
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void KClosestPoints(" in hpp and "lbvh_k_closest_points(" in hpp


# ---- CPU: known answers of the reference --------------------------------------------------------------------------------

def test_reference_known_answers_duplicated_triangle():
    a = np.tile(np.array([[0, 0, 0]], dtype=F), (5, 1))
    b = np.tile(np.array([[4, 0, 0]], dtype=F), (5, 1))
    c = np.tile(np.array([[0, 4, 0]], dtype=F), (5, 1))
    lo, hi = padded_boxes(a, b, c)
    q = make_queries(np.array([[1, 1, 3]], dtype=F), INF)
    r = K.reference(q, a, b, c, lo, hi, 3)
    assert r.records.shape == (1, 3) and r.found.tolist() == [3] and r.rejected == 0 and r.candidates.tolist() == [5]
    assert r.records["tri"][0].tolist() == [0, 1, 2] and (r.records["dist2"][0] == F(9.0)).all()
    assert (r.records["u"][0] == F(0.25)).all() and (r.records["v"][0] == F(0.25)).all()
    r = K.reference(q, a, b, c, lo, hi, 8)
    assert r.found.tolist() == [5] and r.records["tri"][0].tolist() == [0, 1, 2, 3, 4, 0, 0, 0]
    assert (row_words(r.records)[0].reshape(8, 4)[5:] == NONE_WORDS).all()
    assert (row_words(K.truncate(r, 3).records) == row_words(K.reference(q, a, b, c, lo, hi, 3).records)).all()
    # inactive and NaN points: rows of none-records, nothing found
    q = make_queries(np.array([[1, 1, 3], [np.nan, 0, 0], [1, 1, 3]], dtype=F), np.array([0.0, np.inf, np.nan], dtype=F))
    r = K.reference(q, a, b, c, lo, hi, 4)
    assert r.found.tolist() == [0, 0, 0] and (row_words(r.records).reshape(-1, 4) == NONE_WORDS).all()
    # the radius is strict: dist2 == 9 is not below R == 9
    r = K.reference(make_queries(np.array([[1, 1, 3]] * 2, dtype=F), np.array([9.0, np.nextafter(F(9), INF)], dtype=F)), a, b, c, lo, hi, 2)
    assert r.found.tolist() == [0, 2]


def test_reference_k1_is_the_closest_point_reference():
    a, b, c = positions(golden("viking_room"))
    lo, hi = padded_boxes(a, b, c)
    rng = np.random.default_rng(11)
    pts = _mixed_points(a, b, c, 600, rng)
    q = make_queries(pts, np.where(rng.random(600) < 0.5, INF, F(0.01)).astype(F))
    one = R.reference(q, a, b, c, lo, hi)
    r = K.reference(q, a, b, c, lo, hi, 1)
    assert (row_words(r.records) == words(one.records).reshape(-1, 4)).all()
    assert (r.found == one.flags).all() and r.rejected == one.rejected
    assert 0 < r.found.sum() < 600


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class KPoints:
    """device buffers for one query set: rows of up to KMAX records, the found counts, and the two single-answer calls"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer, self.n = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, self.n, L().POINT_QUERY)
        self.queries.local[:] = queries
        self.queries.sync()
        self.rows = H().DataBuffer(ctx, self.n * KMAX, L().CLOSEST_POINT)
        self.found = H().DataBuffer(ctx, self.n, np.uint32)
        self.out = H().DataBuffer(ctx, self.n, L().CLOSEST_POINT)
        self.flags = H().DataBuffer(ctx, self.n, np.uint32)

    def knn(self, k, with_found=True):
        """(rows (n, k), found (n)); the words beyond n * k must stay as they were filled"""
        self.rows.fill_u32(0x7FC00000)
        self.found.fill_u32(0xDEADBEEF)
        self.drawer.k_closest_points(self.queries, k, self.rows, self.found if with_found else None)
        got = self.rows.get_data().copy()
        assert (words(got[self.n * k:]) == 0x7FC00000).all()
        return got[: self.n * k].reshape(self.n, k), self.found.get_data().copy()

    def closest(self):
        self.out.fill_u32(0x7FC00000)
        self.drawer.closest_points(self.queries, self.out)
        return self.out.get_data().copy()

    def within(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.within_distance(self.queries, self.flags)
        return self.flags.get_data().copy()

    def dispose(self):
        for b in (self.queries, self.rows, self.found, self.out, self.flags):
            b.dispose()


def _scene(name):
    if name == "random":
        return scenes.random_triangles(4096)
    if name == "grid":
        return scenes.grid_scene()
    return golden(name)


_CASES = {}


def parity_case(ctx, name):
    """(triangles, queries, the reference for k = KMAX, drawer): the reference is computed once per scene and truncated for the
    smaller k; one context keeps one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _CASES:
        tris = _scene(name)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        a, b, c = positions(tris)
        lo, hi = library_boxes(d)
        queries, _ = mixed_queries(a, b, c, lo, hi, 1500, 5 + len(tris))
        _CASES[name] = (tris, queries, K.reference(queries, a, b, c, lo, hi, KMAX), d)
    _CASES[name][3].build_fast_scene()
    return _CASES[name]


SCENES = ["random", "grid", "example_object3", "viking_room"]

# what the k = 8 rows of each scene's set must exercise: more than this many full rows, partial rows (0 < found < 8), inactive
# queries, and rows with two consecutive records of equal dist2 (several triangles share a vertex at dist2 == 0).  `random` cannot
# meet the last one: its 4096 scattered triangles share no vertex, a vertex point has ONE triangle at dist2 == 0, and the reference
# alone counts 0 rows with a tie on its set (checked on the CPU with the Morton stage's boxes; 310 full, 273 partial, 633
# inactive).  Its threshold is lowered to what the reference gives — the count must EQUAL the reference's, as on every scene —;
# the tie rule is carried by the three mesh scenes (grid / example_object3 456 rows, viking_room 379) and by test 3.
EXERCISED = {"random": (50, 50, 300, None), "grid": (50, 50, 300, 20), "example_object3": (50, 50, 300, 20), "viking_room": (50, 50, 300, 20)}


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", SCENES)
def test_1_rows_equal_the_brute_force_word_for_word(ctx, name, k):
    tris, queries, ref32, d = parity_case(ctx, name)
    assert len(queries) == 1500 and ref32.rejected == 0                # the box rule does not carry this test
    ref = K.truncate(ref32, k)
    q = KPoints(ctx, d, queries)
    got, found = q.knn(k)
    q.dispose()
    assert_rows(got, found, ref, (name, k))
    if k == 8:
        act = R.active(queries)
        full = int((found == k).sum())
        partial = int(((found > 0) & (found < k)).sum())

        def tie_rows(rec, cnt):
            dd = rec["dist2"]
            return int(((dd[:, 1:] == dd[:, :-1]) & (np.arange(1, k)[None, :] < cnt[:, None])).any(axis=1).sum())

        ties = tie_rows(got, found)
        print(f"{name}: {int(act.sum())} active, {full} full rows, {partial} partial, {int((~act).sum())} inactive, {ties} rows with a tie")
        m_full, m_partial, m_inactive, m_ties = EXERCISED[name]
        assert full > m_full and partial > m_partial and (~act).sum() > m_inactive
        assert ties == tie_rows(ref.records, ref.found) and (ties > m_ties if m_ties is not None else ties == 0)
        assert (row_words(got[~act]).reshape(-1, 4) == NONE_WORDS).all() and (found[~act] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_2_k1_is_the_closest_point_query_and_record_0_is_it_for_k8(ctx, name):
    tris, queries, ref32, d = parity_case(ctx, name)
    q = KPoints(ctx, d, queries)
    one, flags = q.closest(), q.within()
    got1, found1 = q.knn(1)
    assert (row_words(got1) == words(one).reshape(-1, 4)).all()
    assert (found1 == flags).all()
    got8, found8 = q.knn(8)
    assert (row_words(got8[:, :1]) == words(one).reshape(-1, 4)).all()
    assert ((found8 >= 1) == (flags == 1)).all()
    got8n, _ = q.knn(8, with_found=False)                              # d_found == NULL: the same rows, the counts untouched
    assert (row_words(got8n) == row_words(got8)).all() and (q.found.get_data() == 0xDEADBEEF).all()
    q.dispose()


_TIES = {}


def ties_case():
    """2048 triangles: 128 distinct random ones, each present 16 times at scattered indices; points on and near them"""
    if not _TIES:
        base = scenes.random_triangles(n=128, seed=9, extent=20.0, edge=4.0)
        rng = np.random.default_rng(17)
        tris = np.repeat(base, 16)[rng.permutation(2048)]
        a, b, c = positions(tris)
        k = rng.integers(0, 2048, 600)
        w = rng.dirichlet((1, 1, 1), 600)
        on = a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
        pts = np.concatenate([on[:300], on[300:] + rng.normal(0.0, 1.5, (300, 3)), a[k[:60]]]).astype(F)
        r2 = np.where(rng.random(len(pts)) < 0.7, INF, F(6.0)).astype(F)
        _TIES["case"] = (tris, make_queries(pts, r2)[rng.permutation(len(pts))])
    return _TIES["case"]


@pytest.mark.gpu
def test_3_ties_across_the_kth_place_go_to_the_lowest_indices(ctx):
    tris, queries = ties_case()
    a, b, c = positions(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    ref32 = K.reference(queries, a, b, c, lo, hi, KMAX)
    assert ref32.rejected == 0
    # every distance class has 16 equal members (or a multiple): the candidate counts say so, and the cut at 4 and 20 falls inside one
    act = R.active(queries)
    unbounded = act & (queries["max_dist2"] == INF)
    assert (ref32.candidates[unbounded] == 2048).all()
    dd = ref32.records["dist2"][unbounded]
    assert (dd[:, 0] == dd[:, 15]).all() and (dd[:, 16] == dd[:, 31]).all()
    q = KPoints(ctx, d, queries)
    for k in (4, 16, 20):
        ref = K.truncate(ref32, k)
        got, found = q.knn(k)
        assert_rows(got, found, ref, k)
        full = found == k
        assert full.sum() > 300 and (np.diff(got["tri"][full][:, :min(k, 16)].astype(np.int64), axis=1) > 0).all()
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_4_fewer_triangles_than_k(ctx, n):
    centre = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], dtype=F)[:n]
    a = centre
    b = centre + np.array([1, 0, 0], dtype=F)
    c = centre + np.array([0, 1, 0], dtype=F)
    tris = pack(a, b, c)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    rng = np.random.default_rng(n)
    pts = np.concatenate([[[0.25, 0.25, 0.5]], rng.uniform(-3, 13, (6, 3))]).astype(F)           # 7 queries: less than a wave
    for r2, want in ((INF, n), (F(1.0), None)):
        queries = make_queries(pts, r2)
        ref = K.reference(queries, a, b, c, lo, hi, KMAX)
        q = KPoints(ctx, d, queries)
        got, found = q.knn(KMAX)
        q.dispose()
        assert_rows(got, found, ref, (n, float(r2)))
        if want is not None:
            assert (found == n).all()
            assert (row_words(got[:, n:]).reshape(-1, 4) == NONE_WORDS).all()
            assert (np.sort(got["tri"][:, :n], axis=1) == np.arange(n)).all()
        else:                                                          # the radius admits exactly one triangle for the first point
            assert found[0] == 1 and got["tri"][0, 0] == 0 and got["dist2"][0, 0] == F(0.25)
            assert (row_words(got[:1, 1:]).reshape(-1, 4) == NONE_WORDS).all()
    d.on_destroy()


@pytest.mark.gpu
def test_5_rows_are_the_heads_of_the_sorted_gather_segments(ctx):
    tris, queries, ref32, d = parity_case(ctx, "random")
    a, b, c = positions(tris)
    finite = queries.copy()
    act = R.active(finite)
    rng = np.random.default_rng(4)
    finite["max_dist2"] = np.where(act, (F(400.0) * rng.uniform(0.2, 3.0, len(finite))).astype(F), finite["max_dist2"])
    q = KPoints(ctx, d, finite)
    offsets, seg_tris = d.overlaps(q.queries)
    k = 8
    got, found = q.knn(k)
    q.dispose()
    lens = np.diff(offsets.astype(np.int64))
    assert (found == np.minimum(lens, k)).all()
    assert (lens > k).sum() > 50 and ((lens > 0) & (lens < k)).sum() > 50
    for i in np.nonzero(lens > 0)[0]:
        t = seg_tris[offsets[i]:offsets[i + 1]].astype(np.int64)
        dist, _, _ = R.point_triangle(finite["p"][i][None, :], a[t], (b - a)[t], (c - a)[t])
        order = np.lexsort((t, dist))[:k]                              # (dist2, tri)
        m = len(order)
        assert (got["tri"][i, :m] == t[order]).all(), i
        assert (words(got["dist2"][i, :m]) == words(dist[order])).all(), i


@pytest.mark.gpu
def test_6_constructed_box_rule_rejections(ctx):
    """A few triangles' boxes shrunk about their centres after the Morton stage and the sort, the derived scene built from them:
    GPU == reference fed the same boxes, the reference counts rejections, and rows differ from the untouched scene's."""
    tris = scenes.random_triangles(n=3000, seed=21, extent=30.0, edge=6.0)
    a, b, c = positions(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    n = len(tris)
    lo0, hi0 = library_boxes(d)
    rng = np.random.default_rng(3)
    picked = rng.choice(n, 60, replace=False)
    w = rng.dirichlet((1, 1, 1), 600)
    k = picked[rng.integers(0, len(picked), 600)]
    pts = np.concatenate([a[picked], b[picked], c[picked], a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:],
                          rng.uniform(lo0.min(axis=0), hi0.max(axis=0), (800, 3))]).astype(F)
    r2 = np.where(rng.random(len(pts)) < 0.5, INF, F(40.0)).astype(F)
    queries = make_queries(pts, r2)[rng.permutation(len(pts))]
    kk = 8
    before = K.reference(queries, a, b, c, lo0, hi0, kk)
    q = KPoints(ctx, d, queries)
    got, found = q.knn(kk)
    assert before.rejected == 0
    assert_rows(got, found, before, "before")
    box = d.container.triangle_aabb.local                              # the mirror get_data() filled, all `capacity` entries
    centre = (box["min"][picked] + box["max"][picked]) * F(0.5)
    half = (box["max"][picked] - box["min"][picked]) * F(0.05)
    box["min"][picked] = centre - half
    box["max"][picked] = centre + half
    d.container.triangle_aabb.sync()
    d.build_fast_scene()
    lo1, hi1 = box["min"][:n].copy(), box["max"][:n].copy()
    ref = K.reference(queries, a, b, c, lo1, hi1, kk)
    got, found = q.knn(kk)
    assert ref.rejected > 0
    assert_rows(got, found, ref, "after")
    changed = (row_words(ref.records) != row_words(before.records)).any(axis=1)
    print(f"box rule: {ref.rejected} pairs rejected, {int(changed.sum())} of {len(queries)} rows changed")
    assert changed.sum() > 0
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
def test_7_statistics(ctx):
    tris, queries, ref32, d = parity_case(ctx, "random")
    lay = L()
    q = KPoints(ctx, d, queries)
    stats = H().DataBuffer(ctx, 1, lay.RAY_STATS)
    per = {}
    try:
        for name, call in (("closest", q.closest), (1, lambda: q.knn(1)), (8, lambda: q.knn(8)), (32, lambda: q.knn(32))):
            stats.fill_u32(0)
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
            call()
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
            s = stats.get_data()[0]
            per[name] = (int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"]))
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    print("rays, node lines, triangle tests:", per)
    n_active = int(R.active(queries).sum())
    assert all(v[0] == n_active for v in per.values())
    assert per[1] == per["closest"]                                    # k = 1: the walk makes the same decisions
    assert per[1][1] <= per[8][1] <= per[32][1] and per[1][2] <= per[8][2] <= per[32][2]
    assert per[1][1] >= n_active
    stats.dispose()
    q.dispose()


@pytest.mark.gpu
def test_8_errors_scratch_failure_and_the_stack_limit(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        rng = np.random.default_rng(2)
        queries = make_queries(_mixed_points(a, b, c, 3000, rng), INF)
        lo, hi = library_boxes(d)
        kk = 5
        ref = K.reference(queries, a, b, c, lo, hi, kk)
        q = KPoints(c2, d, queries)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(queries)
        fn = lib.lbvh_k_closest_points

        def untouched():
            return (words(q.rows.get_data()) == 0x7FC00000).all() and (q.found.get_data() == 0xDEADBEEF).all()

        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
        q.rows.fill_u32(0x7FC00000)
        q.found.fill_u32(0xDEADBEEF)
        assert fn(h, q.queries.device, n, kk, C.byref(s), q.rows.device, q.found.device) == -2
        assert untouched()
        got, found = q.knn(kk)
        assert_rows(got, found, ref, "after the failed reservation")
        # argument checks: LBVH_ERR_INVALID_ARG, nothing enqueued
        q.rows.fill_u32(0x7FC00000)
        q.found.fill_u32(0xDEADBEEF)
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        assert fn(h, None, n, kk, C.byref(s), q.rows.device, q.found.device) == -1
        assert fn(h, q.queries.device, n, kk, None, q.rows.device, q.found.device) == -1
        assert fn(h, q.queries.device, n, kk, C.byref(s), None, q.found.device) == -1
        assert fn(h, q.queries.device, n, 0, C.byref(s), q.rows.device, q.found.device) == -1
        assert fn(h, q.queries.device, n, 33, C.byref(s), q.rows.device, q.found.device) == -1
        assert fn(h, p(q.queries, 4), 10, kk, C.byref(s), q.rows.device, q.found.device) == -1
        assert fn(h, q.queries.device, 10, kk, C.byref(s), p(q.rows, 8), q.found.device) == -1
        assert fn(h, q.queries.device, 10, kk, C.byref(s), q.rows.device, p(q.found, 2)) == -1
        assert fn(h, q.queries.device, 1 << 32, kk, C.byref(s), q.rows.device, q.found.device) == -1
        assert fn(None, q.queries.device, 10, kk, C.byref(s), q.rows.device, q.found.device) == -1
        # count == 0: a no-op
        assert fn(h, q.queries.device, 0, kk, C.byref(s), q.rows.device, q.found.device) == 0
        assert untouched()
        # aligned sub-ranges are accepted: queries 1 .. 10 into rows from record 1, counts from word 1
        assert fn(h, p(q.queries, 16), 10, kk, C.byref(s), p(q.rows, 16), p(q.found, 4)) == 0
        sub = q.rows.get_data()[1:1 + 10 * kk].reshape(10, kk)
        assert (row_words(sub) == row_words(ref.records[1:11])).all() and (q.found.get_data()[1:11] == ref.found[1:11]).all()
        # a stale scene: triangles uploaded without a rebuild
        d.container.triangle_data.sync()
        q.rows.fill_u32(0x7FC00000)
        q.found.fill_u32(0xDEADBEEF)
        assert fn(h, q.queries.device, n, kk, C.byref(s), q.rows.device, q.found.device) == -1
        assert b"stale" in lib.lbvh_last_error(h)
        assert untouched()
        d.rebuild(fast=True)
        s = d.container.scene()
        # a small LDS part exercises the device-memory part of the stack: same rows
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        got, found = q.knn(kk)
        assert_rows(got, found, ref, "stack split 1")
        # the stack limit: a reported error (LBVH_ERR_HIP at the next sync), never a silently wrong row
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        q.drawer.k_closest_points(q.queries, kk, q.rows, q.found)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        got, found = q.knn(kk)
        assert_rows(got, found, ref, "after the stack limit")
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_9_path_tracer_frame_undisturbed_by_a_k_nearest_call_between_bounces(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    # the same frame with the query issued between the bounces, 4x the frame's count: the ray scratch grows in mid-frame
    a, b, c = positions(tris)
    queries = make_queries(_mixed_points(a, b, c, 4 * 160 * 96, np.random.default_rng(12)), F(25.0))
    q = KPoints(ctx, pt.drawer, queries)
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def knn():
        pt.drawer.k_closest_points(q.queries, 4, q.rows, q.found)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    knn()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        knn()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    knn()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    f = q.found.get_data()
    assert 0 < (f > 0).sum() < len(queries) and f.max() == 4
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [None, 12.0])
def test_10_cpp_host_driver_knn_matches_the_python_host(ctx, radius):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    n, count, k = 4096, 20000, 8
    args = [exe, "knn", str(k), str(n), str(count)] + ([str(radius)] if radius is not None else [])
    res = json.loads(subprocess.run(args, check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(n)                                 # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    pts = driver_points(lo, hi, count)                                 # and its points (seed 2)
    queries = make_queries(pts, INF if radius is None else F(radius) * F(radius))
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    rows = H().DataBuffer(ctx, count * k, L().CLOSEST_POINT)
    found = H().DataBuffer(ctx, count, np.uint32)
    qb = H().DataBuffer(ctx, count, L().POINT_QUERY)
    qb.local[:] = queries
    qb.sync()
    d.k_closest_points(qb, k, rows, found)
    got, f = rows.get_data(), found.get_data()
    assert res["triangles"] == n and res["points"] == count and res["k"] == k
    assert res["found_sum"] == int(f.sum()) and res["full_rows"] == int((f == k).sum())
    assert res["word_sum"] == int(words(got).astype(np.uint64).sum())
    assert [[t for _, t in row] for row in res["rows"]] == [got["tri"][i * k: i * k + f[i]].tolist() for i in range(3)]
    assert res["full_rows"] == count if radius is None else 0 < res["full_rows"] < count
    for buf in (rows, found, qb):
        buf.dispose()
    d.on_destroy()
