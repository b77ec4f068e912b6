"""lbvh_triangle_intersections / lbvh_triangle_intersects_any: which scene triangles a triangle intersects, as a CSR list and as a
flag, over the four-wide derived traversal scene.  The expectation is tests/triangle_query_reference.py: the header's definition in
numpy float32 (box comparisons over every pair, the six edge tests on the pairs that pass them), with the triangles' own boxes as
the library produced them — no tree.  The order inside a segment is not part of the contract, so every GPU comparison is word for
word AFTER lbvh_sort_index_segments (T1) or a host sort of each segment.
  CPU  the surface in every host; the restatement on hand-built pairs; the parity sets are not vacuous
  T1   parity on grid_80x80 and cfg1_4096             T2  query counts around a wave; wave caps (the lane refill)
  T3   skip: a mesh against itself                    T4  inactive queries
  T5   count-only and overflow                        T6  count == 0, every rejection, a stale scene (the entry contract)
  T7   subset of lbvh_box_overlaps; a small LDS stack; statistics      T8  lbvh_driver tris: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_reference as V
import triangle_query_reference as T
from query_support import driver_mesh, H, L, library_boxes, N, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NULL = T.NULL
COUNT = 2000
PARITY = ["grid_80x80", "cfg1_4096"]


def scene(name):
    """the triangles of the two goldens, from the seeded generators that made them (tests/test_gpu_parity.py checks they still do)"""
    tris = scenes.grid_scene() if name == "grid_80x80" else scenes.random_triangles(4096, seed=1)
    assert len(tris) == (12800 if name == "grid_80x80" else 4096)
    return tris


def parity_queries(a, b, c, count=COUNT, seed=11):
    """Scene triangles turned about their centroid by a seeded angle about a seeded axis and scaled by 0.5 .. 4; two fifths of them
    then moved off by 2 .. 8 times their size in a random direction (the queries with no candidate); a quarter carry skip = the
    triangle they were made from."""
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
    return T.make_queries(out[:, 0].astype(F), out[:, 1].astype(F), out[:, 2].astype(F), skip)


_CPU = {}


def cpu_case(name):
    """(a, b, c, queries, reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        q = parity_queries(a, b, c)
        _CPU[name] = (a, b, c, q, T.reference(q, a, b, c, *padded_boxes(a, b, c)))
    return _CPU[name]


def sorted_lists(offsets, tris):
    return V.sort_segments(offsets, tris)


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_struct_and_both_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_tri_query \{\s*float a\[3\]; uint32_t skip;[^\n]*\n\s*float b\[3\]; uint32_t _pad0;[^\n]*\n"
                     r"\s*float c\[3\]; uint32_t _pad1;[^\n]*\n\} lbvh_tri_query;", h)
    assert re.search(r"lbvh_status lbvh_triangle_intersections\(lbvh_context\* ctx, const lbvh_tri_query\* d_queries, size_t count, "
                     r"const lbvh_scene\* h_scene,\s+uint64_t\* d_offsets, uint32_t\* d_tris, uint64_t capacity\);", h)
    assert re.search(r"lbvh_status lbvh_triangle_intersects_any\(lbvh_context\* ctx, const lbvh_tri_query\* d_queries, size_t count, "
                     r"const lbvh_scene\* h_scene,\s+uint32_t\* d_flags\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_triangle_intersections" in bounce and "lbvh_triangle_intersects_any" in bounce
    text = h[h.index("Triangle queries: WHICH"):h.index("lbvh_status lbvh_triangle_intersections(")]
    for must in ("Coplanar overlapping triangles are generally NOT reported", "only touch", "fp32 noise", "NOT PART OF THE CONTRACT",
                 "d_offsets[0] included"):
        assert must in text, must


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_triangle_intersections"]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
    res, args = nat.SIGNATURES["lbvh_triangle_intersects_any"]
    assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.TRI_QUERY.itemsize == 48
    assert [lay.TRI_QUERY.fields[f][1] for f in ("a", "skip", "b", "_pad0", "c", "_pad1")] == [0, 12, 16, 28, 32, 44]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_triangle_intersections\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+,"
                     r"\s+IntPtr \w+,\s+ulong capacity\);", cs)
    assert re.search(r"public static extern int lbvh_triangle_intersects_any\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    tq = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "TriangleQueries.cs")).read())
    assert "lbvh_triangle_intersections" in tq and "lbvh_triangle_intersects_any" in tq and "unsafe" not in tq
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void TriangleIntersections(" in hpp and "void TriangleIntersectsAny(" in hpp
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("triangle_intersections", "triangle_intersects_any", "intersections"))


# ---- CPU: the restatement on pairs with known answers ------------------------------------------------------------------------

def one_pair(query, tri, skip=NULL):
    """-> (candidate?, a query edge passed, a scene edge passed, the boxes overlap) for one query and one scene triangle"""
    q = np.array(query, dtype=F)
    t = np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    lo, hi = padded_boxes(a, b, c)
    queries = T.make_queries(q[None, 0], q[None, 1], q[None, 2], skip)
    r = T.reference(queries, a, b, c, lo, hi)
    boxes = (q.min(axis=0) <= hi[0]).all() and (lo[0] <= q.max(axis=0)).all()
    assert r.flags[0] == (int(r.offsets[1]) > 0) and int(r.offsets[1]) in (0, 1)
    found = int(r.offsets[1]) == 1
    return found, bool(r.query_edge[0]) if found else False, bool(r.scene_edge[0]) if found else False, bool(boxes)


TILTED = [(-2, -1, -2), (2, 1, -2), (0, 0, 2)]                 # the plane x - 2 y = 0
CROSSING = [(0, -1, 0), (0, 1, 0), (0, 0, 3)]                  # in the plane x = 0; its edge a-b passes through (0, 0, 0)
LARGE = [(-10, -10, 0), (10, -10, 0), (0, 10, 0)]
SMALL = [(0, 0, -1), (0.5, 0, 1), (-0.5, 0.3, 1)]              # two of its edges pass through the face of LARGE


def test_reference_two_triangles_crossing_and_moved_apart():
    found, _, _, boxes = one_pair(CROSSING, TILTED)
    assert found and boxes
    # the same pair, the query moved by (0.5, -1, 0) — along the normal (1, -2, 0) / sqrt 5 of TILTED: the plane x = 0.5 meets TILTED
    # at y = 0.25, the moved query has y <= 0; the boxes still overlap
    moved = [(x + 0.5, y - 1.0, z) for x, y, z in CROSSING]
    found, _, _, boxes = one_pair(moved, TILTED)
    assert not found and boxes
    assert one_pair(CROSSING, TILTED, skip=0)[0] is False        # the only scene triangle skipped


def test_reference_which_edges_fire():
    assert one_pair(SMALL, LARGE) == (True, True, False, True)   # the small triangle through the face of the large one: query edges only
    assert one_pair(LARGE, SMALL) == (True, False, True, True)   # the converse: scene edges only


def test_reference_coplanar_overlap_is_not_reported_and_a_shared_vertex_is():
    # both in the plane z = 0, overlapping: every edge is parallel to the other triangle's plane, det == 0 exactly
    found, _, _, boxes = one_pair([(0.5, 0.5, 0), (2.5, 0.5, 0), (0.5, 2.5, 0)], [(0, 0, 0), (2, 0, 0), (0, 2, 0)])
    assert not found and boxes
    # one shared vertex, at the scene triangle's first vertex: s = 0, so u = v = t = 0 with a non-zero det — the arithmetic passes it
    found, qe, se, boxes = one_pair([(0, 0, 0), (0, -1, 1), (-1, 0, 1)], [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    assert found and qe and boxes


def test_reference_inactive_queries_have_nothing():
    a, b, c = (np.array([x], dtype=F) for x in TILTED)
    lo, hi = padded_boxes(a, b, c)
    q = np.repeat(T.make_queries(*(np.array([x], dtype=F) for x in CROSSING)), 28)
    for k, (vertex, axis) in enumerate((v, x) for v in "abc" for x in range(3)):
        q[vertex][1 + 3 * k, axis] = np.nan
        q[vertex][2 + 3 * k, axis] = np.inf
        q[vertex][3 + 3 * k, axis] = -np.inf
    r = T.reference(q, a, b, c, lo, hi)
    assert T.active(q).tolist() == [True] + [False] * 27 and r.flags.tolist() == [1] + [0] * 27


def test_the_parity_sets_are_not_vacuous():
    """Conditions on the REFERENCE alone (tuned on the CPU, not measured on the GPU): per set at least a quarter of the active queries
    have a candidate and at least a quarter have none, and both a candidate found by the query's edges only and one found by the
    scene triangle's edges only occur.  A query with 8 or more candidates exists in the sets taken together: cfg1_4096 is a soup of
    4 096 two-unit triangles in a 200-unit cube, where a query of at most four times that size meets two triangles at the most;
    the long lists come from the grid."""
    longest = 0
    for name in PARITY:
        a, b, c, q, r = cpu_case(name)
        n = np.diff(r.offsets).astype(np.int64)
        act = T.active(q)
        qe_only, se_only = int((r.query_edge & ~r.scene_edge).sum()), int((r.scene_edge & ~r.query_edge).sum())
        print(f"{name}: {100.0 * (n[act] > 0).mean():.1f} % with a candidate, longest {int(n.max())}, total {int(n.sum())}, "
              f"query-edge-only {qe_only}, scene-edge-only {se_only}")
        assert act.all() and len(q) == COUNT
        assert (n[act] > 0).mean() >= 0.25 and (n[act] == 0).mean() >= 0.25
        assert qe_only > 0 and se_only > 0
        assert (q["skip"] != NULL).sum() > COUNT // 8
        longest = max(longest, int(n.max()))
    assert longest >= 8


def test_driver_generator_is_deterministic_and_inside_the_box():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    a, b, c = T.driver_triangles(lo, hi, 50, seed=5)
    a2, _, _ = T.driver_triangles(lo, hi, 50, seed=5)
    assert (a == a2).all() and (a >= lo).all() and (a <= hi).all()
    assert (np.abs(b - a) <= 3).all() and (np.abs(c - a) <= 3).all() and (a != T.driver_triangles(lo, hi, 50, seed=6)[0]).any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Queries:
    """device buffers of one query set; run() = one lbvh_triangle_intersections call on caller-owned buffers"""

    def __init__(self, ctx, drawer, queries):
        self.ctx, self.drawer, self.count = ctx, drawer, len(queries)
        self.queries = H().DataBuffer(ctx, max(len(queries), 1), L().TRI_QUERY)
        self.queries.local[:len(queries)] = queries
        self.queries.sync()
        self.offsets = H().DataBuffer(ctx, len(queries) + 1, np.uint64)
        self.flags = H().DataBuffer(ctx, max(len(queries), 1), np.uint32)

    def run(self, tris=None, capacity=None):
        """offsets (host copy) after one call; tris: a uint32 DataBuffer or None, capacity defaults to its size"""
        self.offsets.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        cap = 0 if tris is None else (tris.size if capacity is None else capacity)
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersections(self.ctx.handle, self.queries.device, self.count, C.byref(s),
                                                                       self.offsets.device, tris.device if tris is not None else None, cap))
        return self.offsets.get_data().copy()

    def lists(self, device_sort=True):
        """(offsets, tris) through the count -> allocate -> fill convenience, every segment ascending"""
        off, tris = self.drawer._csr_lists(self._call, self.queries, 1, device_sort)
        return (off, tris) if device_sort else (off, sorted_lists(off, tris))

    def _call(self, queries, offsets, tris=None):
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersections(self.ctx.handle, queries.device, self.count, C.byref(s), offsets.device,
                                                                       tris.device if tris is not None else None, tris.size if tris is not None else 0))

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, N().lib.lbvh_triangle_intersects_any(self.ctx.handle, self.queries.device, self.count, C.byref(s), self.flags.device))
        return self.flags.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.queries, self.offsets, self.flags):
            b.dispose()


def assert_equal_lists(got, ref, what=""):
    (go, gt), ro, rt = got, ref.offsets, ref.tris
    assert (go[:len(ro)] == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gt) == len(rt) == int(ro[-1]), what
    bad = np.nonzero(gt != rt)[0]
    assert len(bad) == 0, (what, bad[:10], gt[bad[:10]], rt[bad[:10]])


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
        _GPU[name] = (a, b, c, lo, hi, q, T.reference(q, a, b, c, lo, hi), d)
    _GPU[name][-1].build_fast_scene()
    return _GPU[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, name)
    n = np.diff(ref.offsets).astype(np.int64)
    print(f"{name}: {100.0 * (n > 0).mean():.1f} % non-empty, longest {int(n.max())}, total {int(n.sum())}")
    assert 0.25 <= (n > 0).mean() <= 0.75
    q = Queries(ctx, d, queries)
    assert_equal_lists(q.lists(device_sort=True), ref, "device sort")
    assert (q.any() == ref.flags).all()
    # the public convenience of the drawer gives the same lists
    off, tris = d.intersections(q.queries, device_sort=True)
    assert_equal_lists((off, tris), ref, "intersections()")
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_t2_query_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[200:200 + count]
    r = T.reference(sub, a, b, c, lo, hi)
    assert count == 1 or int(r.offsets[-1]) > 0
    q = Queries(ctx, d, sub)
    assert_equal_lists(q.lists(), r, count)
    assert (q.any() == r.flags).all()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 3])
def test_t2_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 queries on 1 or 3 waves: runs of 1 500 / 500, every lane refilled many times"""
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    sub = queries[:1500].copy()
    sub["a"][100:235, 0] = np.nan                                    # a block of inactive queries inside a run
    r = T.reference(sub, a, b, c, lo, hi)
    q = Queries(ctx, d, sub)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        got, flags = q.lists(), q.any()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal_lists(got, r, waves)
    assert (flags == r.flags).all()
    q.dispose()


@pytest.mark.gpu
def test_t3_skip_removes_the_own_triangle(ctx):
    a, b, c, lo, hi, _, _, d = gpu_case(ctx, "cfg1_4096")
    n = len(a)
    own = np.arange(n, dtype=np.uint32)
    for skip in (own, np.full(n, NULL, dtype=np.uint32)):
        queries = T.make_queries(a, b, c, skip)
        r = T.reference(queries, a, b, c, lo, hi)
        q = Queries(ctx, d, queries)
        off, tris = q.lists()
        assert_equal_lists((off, tris), r)
        seg = np.repeat(own, np.diff(off).astype(np.int64))
        has_own = np.bincount(seg[tris == seg], minlength=n)
        ref_seg = np.repeat(own, np.diff(r.offsets).astype(np.int64))
        ref_own = np.bincount(ref_seg[r.tris == ref_seg], minlength=n)
        assert (has_own == ref_own).all()
        if skip[0] != NULL:
            assert not has_own.any()
        else:
            # (a triangle's edges lie in its own plane: det ~ 0, so whether it finds itself is rounding — the reference decides)
            print(f"skip = LBVH_NULL: {int(ref_own.sum())} of {n} triangles find themselves")
        assert (q.any() == r.flags).all()
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
    r = T.reference(sub, a, b, c, lo, hi)
    q = Queries(ctx, d, sub)
    off, tris = q.lists()
    assert_equal_lists((off, tris), r)
    flags = q.any()
    assert (np.diff(off)[~act] == 0).all() and (flags[~act] == 0).all() and (flags == r.flags).all()
    # the neighbours are what they were in the full set
    full = np.diff(ref.offsets)[:540]
    assert (np.diff(off)[act] == full[act]).all() and np.diff(off)[act].sum() > 0
    q.dispose()


@pytest.mark.gpu
def test_t5_count_only_and_overflow(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    total = int(ref.offsets[-1])
    cap, guard = total // 2, 4096
    q = Queries(ctx, d, queries)
    assert (q.run(None) == ref.offsets).all()                            # capacity == 0, d_tris == NULL
    buf = H().DataBuffer(ctx, total + guard, np.uint32)
    buf.fill_u32(0xABABABAB)
    off = q.run(buf, capacity=cap)
    got = buf.get_data().copy()
    assert (off == ref.offsets).all() and int(off[-1]) == total
    assert (got[cap:] == 0xABABABAB).all()                               # nothing at the capacity or beyond
    fits = np.nonzero(ref.offsets[1:] <= cap)[0]
    assert 0 < len(fits) < COUNT
    last = int(ref.offsets[fits[-1] + 1])
    assert (sorted_lists(ref.offsets[:fits[-1] + 2], got[:last]) == ref.tris[:last]).all()
    buf.fill_u32(0xABABABAB)                                             # the retry with what the offsets asked for
    off = q.run(buf, capacity=total)
    got = buf.get_data().copy()
    assert (got[total:] == 0xABABABAB).all()
    assert_equal_lists((off, sorted_lists(off, got[:total])), ref)
    buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t6_count_zero_rejections_and_a_stale_scene():
    """the rows test_query_entry_contract.py has for the other entry points, for these two: on a context of its own"""
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
        ref = T.reference(queries, a, b, c, lo, hi)
        assert 0 < ref.flags.sum() < 130
        q = Queries(ctx, d, queries)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, np.uint32)
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        both, flag = lib.lbvh_triangle_intersections, lib.lbvh_triangle_intersects_any
        dq, do, df, dl = q.queries.device, q.offsets.device, q.flags.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, q.flags, lst)

        def poison():
            for buf in bufs:
                buf.fill_u32(0x7FC0DEAD)

        def untouched():
            return all((words(buf.get_data()) == 0x7FC0DEAD).all() for buf in bufs)

        poison()
        assert both(h, dq, 0, C.byref(s), do, dl, 64) == 0 and flag(h, dq, 0, C.byref(s), df) == 0     # count == 0: a no-op
        for args in ((None, 10, C.byref(s), do, None, 0), (dq, 10, None, do, None, 0), (dq, 10, C.byref(s), None, None, 0),
                     (dq, 10, C.byref(s), do, None, 5), (at(q.queries, 4), 10, C.byref(s), do, None, 0),
                     (dq, 10, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, C.byref(s), do, at(lst, 2), 8),
                     (dq, 1 << 32, C.byref(s), do, None, 0)):
            assert both(h, *args) == -1, args
            assert lib.lbvh_last_error(h)
        for args in ((None, 10, C.byref(s), df), (dq, 10, None, df), (dq, 10, C.byref(s), None), (at(q.queries, 8), 10, C.byref(s), df),
                     (dq, 10, C.byref(s), at(q.flags, 2)), (dq, 1 << 32, C.byref(s), df)):
            assert flag(h, *args) == -1, args
        assert both(None, dq, 10, C.byref(s), do, None, 0) == -1 and flag(None, dq, 10, C.byref(s), df) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        for fn, args, name in ((both, (do, None, 0), b"lbvh_triangle_intersections"), (flag, (df,), b"lbvh_triangle_intersects_any")):
            assert fn(h, dq, 130, C.byref(s), *args) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        # aligned sub-ranges are fine; the plain and the counting instantiation write the same words, and the latter counts
        assert both(h, at(q.queries, 48), 10, C.byref(s), at(q.offsets, 8), at(lst, 4), 8) == 0
        stats.fill_u32(0x7FC0DEAD)
        plain = (q.lists(), q.any())
        assert (words(stats.get_data()) == 0x7FC0DEAD).all()
        assert_equal_lists(plain[0], ref)
        assert (plain[1] == ref.flags).all()
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            counted = (q.lists(), q.any())
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        st = stats.get_data()[0]
        assert (counted[0][0] == plain[0][0]).all() and (counted[0][1] == plain[0][1]).all() and (counted[1] == plain[1]).all()
        assert st["rays"] > 0 and st["node_fetches"] > 0 and st["triangle_tests"] > 0, st
        for buf in (lst, stats):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t7_subset_of_the_broad_phase_a_small_lds_stack_and_the_statistics(ctx):
    a, b, c, lo, hi, queries, ref, d = gpu_case(ctx, "grid_80x80")
    q = Queries(ctx, d, queries)
    h, lib = ctx.handle, N().lib
    # every segment is a subset of lbvh_box_overlaps' segment for the query's box
    pts = np.stack([queries["a"], queries["b"], queries["c"]], axis=1)
    boxes = H().DataBuffer(ctx, COUNT, L().AABB)
    boxes.local[:] = V.make_boxes(pts.min(axis=1), pts.max(axis=1))
    boxes.sync()
    boff, btris = d.overlaps(boxes, device_sort=True)
    off, tris = q.lists()
    seg = np.repeat(np.arange(COUNT, dtype=np.int64), np.diff(off).astype(np.int64))
    bseg = np.repeat(np.arange(COUNT, dtype=np.int64), np.diff(boff).astype(np.int64))
    n = len(a)
    assert np.isin(seg * n + tris, bseg * n + btris).all() and len(tris) < len(btris)
    boxes.dispose()
    # a small LDS part exercises the device-memory part of the stack: the same lists and flags
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        got, flags = q.lists(), q.any()
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert_equal_lists(got, ref, "stack split 1")
    assert (flags == ref.flags).all()
    # statistics: the fill walk takes the count walk's decisions; the any form never tests more than the count walk
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    big = H().DataBuffer(ctx, max(int(ref.offsets[-1]), 1), np.uint32)
    seen = []
    try:
        for form in ("count", "full", "any"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            q.any() if form == "any" else q.run(big if form == "full" else None)
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("node fetches, triangle tests: count-only %s, full %s, any %s" % tuple(seen))
    assert seen[1] == (2 * seen[0][0], 2 * seen[0][1]) and 0 < seen[2][0] <= seen[0][0] and 0 < seen[2][1] <= seen[0][1]
    for buf in (stats, big):
        buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t8_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver tris 2000 5`: TriangleIntersections, SortIndexSegments and TriangleIntersectsAny of lbvh_host.hpp on the driver's own
    mesh and queries, against the brute force on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "tris", str(count), "5"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    r = T.reference(T.make_queries(*T.driver_triangles(lo, hi, count, seed=5)), a, b, c, *library_boxes(d))
    d.on_destroy()
    n = np.diff(r.offsets).astype(np.int64)
    weighted = int(((np.arange(len(r.tris), dtype=np.uint64) + np.uint64(1)) * r.tris.astype(np.uint64)).sum())
    assert int(r.offsets[-1]) > 0
    assert (res["triangles"], res["queries"], res["total"], res["non_empty"], res["flagged"], res["weighted_index_sum"]) == \
        (4096, count, int(r.offsets[-1]), int((n > 0).sum()), int(r.flags.sum()), weighted)
    first = np.nonzero(n)[0][:3]
    assert res["segments"] == [[int(k)] + r.tris[int(r.offsets[k]):int(r.offsets[k + 1])].tolist() for k in first]
