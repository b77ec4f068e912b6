"""lbvh_gather_hits: every hit along a ray as an unordered CSR list, over the four-wide derived traversal scene.  The expectation
is tests/gather_hits_reference.py: ray_reference's slab test, Moeller-Trumbore and candidate mask, per ray all candidates in
(t, tri) order.  The library promises no order inside a segment, so both sides are put into the canonical order first (sorted by
(t as an fp32 value, tri): two candidates of a ray never share a triangle index); after that every GPU comparison is word for word
on uint32 views, no tolerance, no case left out.  The scenes and ray sets are those of tests/test_trace_k_closest.py, rebuilt here
from the same recipes, plus one stack of 300 coincident triangles."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gather_hits_reference as G
import k_hits_reference as K
import ray_reference as R
from query_support import (driver_mesh, driver_rays, H, L, library_boxes, make_rays, mixed_rays_of, N, pack, padded_boxes,
                           positions, scene_rays, stacked_sheets, words)
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
KMAX = 32
NAN_WORD = 0x7FC00000


def rec_words(a):
    """records -> (len, 4) words"""
    return words(a).reshape(-1, 4)


MISS_WORDS = words(np.array([R.MISS]))


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_the_prototype_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"lbvh_status lbvh_gather_hits\(lbvh_context\* ctx, const lbvh_ray\* d_rays, size_t count, const lbvh_scene\* h_scene,\s+"
                     r"uint64_t\* d_offsets, lbvh_hit\* d_hits, uint64_t capacity\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_gather_hits" in bounce                                    # listed among the calls that drop the live-path list
    doc = h[h.index("EVERY hit along"):h.index("lbvh_status lbvh_gather_hits(")]
    assert "NOT PART OF THE CONTRACT" in doc                               # the plain statement that segments are unordered


def test_native_signature_has_seven_arguments():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_gather_hits"]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
    assert nat.lib.lbvh_gather_hits.argtypes is not None
    assert nat.ABI_VERSION == 11


def test_csharp_import_wrapper_cpp_host_and_python_host():
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public static extern int lbvh_gather_hits\((.*?)\);", cs, re.S)
    assert m and len(m.group(1).split(",")) == 7
    assert re.match(r"IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+, IntPtr \w+,\s+ulong capacity$", m.group(1))
    rg = open(os.path.join(ROOT, "bindings", "csharp", "RayGather.cs")).read()
    assert "lbvh_gather_hits" in rg and "unsafe" not in rg
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void GatherHits(" in hpp and "lbvh_gather_hits(" in hpp
    drawer = H().RaytracingMeshDrawer
    assert hasattr(drawer, "gather_hits") and hasattr(drawer, "all_hits")
    assert "host" in drawer.all_hits.__doc__.lower()                       # sort=True is documented as a host sort


# ---- CPU: known answers of the reference --------------------------------------------------------------------------------

def five_coincident():
    a = np.tile(np.array([[0, 0, 0]], dtype=F), (5, 1))
    b = np.tile(np.array([[4, 0, 0]], dtype=F), (5, 1))
    c = np.tile(np.array([[0, 4, 0]], dtype=F), (5, 1))
    return (a, b, c) + padded_boxes(a, b, c)


def test_reference_known_answers_coincident_triangles():
    a, b, c, lo, hi = five_coincident()
    ray = make_rays(np.array([[1, 1, 3]], dtype=F), np.array([[0, 0, -1]], dtype=F), F(0), INF)
    r = G.reference(ray, a, b, c, lo, hi)
    assert r.offsets.dtype == np.uint64 and r.offsets.tolist() == [0, 5] and r.records.dtype == R.HIT
    assert r.records["tri"].tolist() == [0, 1, 2, 3, 4] and (r.records["t"] == F(3.0)).all()
    assert (r.records["u"] == F(0.25)).all() and (r.records["v"] == F(0.25)).all()
    # canonical() undoes any order inside a segment
    shuffled = r.records[[3, 0, 4, 2, 1]]
    assert (rec_words(G.canonical(r.offsets, shuffled)) == rec_words(r.records)).all()


def test_reference_bounds_are_strict_on_both_sides():
    a, b, c, lo, hi = five_coincident()
    three = F(3)
    below, above = np.nextafter(three, -INF), np.nextafter(three, INF)
    o, d = np.array([[1, 1, 3]] * 3, dtype=F), np.array([[0, 0, -1]] * 3, dtype=F)
    # t_max one float below t, == t, one float above: only the last admits the five
    r = G.reference(make_rays(o, d, F(0), np.array([below, three, above], dtype=F)), a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 0, 0, 5]
    # t_min one float below t, == t, one float above: only the first admits them
    r = G.reference(make_rays(o, d, np.array([below, three, above], dtype=F), INF), a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 5, 5, 5]


def test_reference_inactive_rays_have_empty_segments():
    a, b, c, lo, hi = five_coincident()
    # the four inactive kinds: empty range, reversed range, NaN t_min, NaN t_max; then one active ray
    rays = make_rays(np.array([[1, 1, 3]] * 5, dtype=F), np.array([[0, 0, -1]] * 5, dtype=F),
                     np.array([5.0, 5.0, np.nan, 0.0, 0.0], dtype=F), np.array([5.0, 1.0, np.inf, np.nan, np.inf], dtype=F))
    assert R.active(rays).tolist() == [False] * 4 + [True]
    r = G.reference(rays, a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 0, 0, 0, 0, 5] and len(r.records) == 5


def test_reference_orders_by_t_then_index():
    """three parallel sheets in the order 2, 0, 1 along the ray, the middle one present twice"""
    z = np.array([5.0, 9.0, 1.0, 5.0], dtype=F)
    a = np.stack([np.zeros(4), np.zeros(4), z], axis=1).astype(F)
    b = a + np.array([4, 0, 0], dtype=F)
    c = a + np.array([0, 4, 0], dtype=F)
    lo, hi = padded_boxes(a, b, c)
    ray = make_rays(np.array([[1, 1, 0]], dtype=F), np.array([[0, 0, 2]], dtype=F), F(0), INF)
    r = G.reference(ray, a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 4] and r.records["tri"].tolist() == [2, 0, 3, 1]
    assert r.records["t"].tolist() == [0.5, 2.5, 2.5, 4.5]


# ---- scenes and ray sets: the recipes of tests/test_trace_k_closest.py ---------------------------------------------------------

def scene_positions(name):
    if name == "sheets":
        return stacked_sheets()
    if name == "torus":
        return tuple(positions(scenes.tiled_torus(nu=24, nv=16, grid=2)))
    return tuple(positions(scenes.random_triangles(4096)))


STACK = 300


def coincident_stack():
    """512 triangles: 300 copies of one triangle and 212 others far to the side, the order permuted so that the copies sit at
    scattered indices.  Eight rays: six through the stack (open; t_max == t, one float below and one above; t_min == t; a
    scaled direction), one that misses it and one inactive.  -> (a, b, c, rays, the indices of the copies)"""
    rng = np.random.default_rng(300)
    other = scenes.random_triangles(n=512 - STACK, seed=3, extent=10.0, edge=2.0)
    oa, ob, oc = positions(other)
    shift = np.array([60.0, 0.0, 0.0], dtype=F)
    a = np.concatenate([np.tile(np.array([[0, 0, 0]], dtype=F), (STACK, 1)), oa + shift])
    b = np.concatenate([np.tile(np.array([[4, 0, 0]], dtype=F), (STACK, 1)), ob + shift])
    c = np.concatenate([np.tile(np.array([[0, 4, 0]], dtype=F), (STACK, 1)), oc + shift])
    order = rng.permutation(512)
    a, b, c = a[order], b[order], c[order]
    copies = np.nonzero(order < STACK)[0]
    three = F(3)
    origin = np.array([[1, 1, 3]] * 6 + [[-9, -9, 3]] + [[1, 1, 3]], dtype=F)
    direction = np.array([[0, 0, -1]] * 5 + [[0, 0, -2]] + [[0, 0, -1]] * 2, dtype=F)
    t_min = np.array([0, 0, 0, 0, 3, 0, 0, 5], dtype=F)
    t_max = np.array([np.inf, three, np.nextafter(three, -INF), np.nextafter(three, INF), np.inf, np.inf, np.inf, 1], dtype=F)
    return a, b, c, make_rays(origin, direction, t_min, t_max), copies


def exercised(rays, ref):
    """(segments of at least 32 records, empty segments of active rays, inactive rays) of a ray set's reference"""
    m = np.diff(ref.offsets.astype(np.int64))
    act = R.active(rays)
    return int((m >= 32).sum()), int((act & (m == 0)).sum()), int((~act).sum())


_CPU = {}


def cpu_case(name):
    """(positions, Morton-stage boxes, rays, the gather reference, the k = KMAX reference), computed once per scene"""
    if name not in _CPU:
        a, b, c = scene_positions(name)
        lo, hi = padded_boxes(a, b, c)
        rays = mixed_rays_of(name, a, b, c, lo, hi)
        _CPU[name] = ((a, b, c), (lo, hi), rays, G.reference(rays, a, b, c, lo, hi), K.reference(rays, a, b, c, lo, hi, KMAX))
    return _CPU[name]


SCENES = ["sheets", "torus", "random"]


def heads(offsets, canon, k):
    """(rows (n, k) of the first min(k, m) records of every canonical segment padded with miss records, found)"""
    off = offsets.astype(np.int64)
    n = len(off) - 1
    m = np.diff(off)
    rows = np.empty((n, k), dtype=R.HIT)
    rows[:] = R.MISS
    j = np.arange(k)[None, :]
    has = j < m[:, None]
    rows[has] = canon[(off[:-1, None] + j)[has]]
    return rows, np.minimum(m, k).astype(np.uint32)


@pytest.mark.parametrize("name", SCENES)
def test_reference_identities_with_the_k_hits_reference(name):
    (a, b, c), _, rays, ref, ref32 = cpu_case(name)
    assert len(rays) == 1500 and len(ref.offsets) == 1501
    m = np.diff(ref.offsets.astype(np.int64))
    assert (m == ref32.candidates).all()                                   # segment length == the candidate count
    assert (rec_words(G.canonical(ref.offsets, ref.records)) == rec_words(ref.records)).all()     # already canonical
    rows, found = heads(ref.offsets, ref.records, KMAX)
    assert (found == ref32.found).all()
    assert (words(rows).reshape(1500, -1) == words(ref32.records).reshape(1500, -1)).all()        # the sorted head == the k = 32 rows
    assert (m[~R.active(rays)] == 0).all() and m.sum() > 0


def test_the_sheets_set_exercises_long_empty_and_inactive_segments():
    """what the reference alone must meet on the stacked sheets (the Morton stage's boxes): more than 50 segments of at least 32
    records, more than 100 empty segments of active rays, more than 100 inactive rays.  The k-hits test documents 165, 113 and
    240 for this recipe; test 1 asserts the same thresholds with the library's boxes."""
    (a, _, _), _, rays, ref, _ = cpu_case("sheets")
    assert len(a) == 5120
    long_, empty, inactive = exercised(rays, ref)
    print(f"sheets: {long_} segments of >= 32 records, {empty} empty segments of active rays, {inactive} inactive rays, "
          f"longest {int(np.diff(ref.offsets.astype(np.int64)).max())}, M {int(ref.offsets[-1])}")
    assert long_ > 50 and empty > 100 and inactive > 100


def test_the_coincident_stack_is_one_long_segment_of_ties():
    a, b, c, rays, copies = coincident_stack()
    assert len(copies) == STACK and len(a) == 512 and not (np.diff(copies) == 1).all()
    lo, hi = padded_boxes(a, b, c)
    ref = G.reference(rays, a, b, c, lo, hi)
    assert np.diff(ref.offsets.astype(np.int64)).tolist() == [STACK, 0, 0, STACK, 0, STACK, 0, 0]
    first = ref.records[:STACK]
    assert (first["t"] == F(3.0)).all() and (first["tri"] == copies).all()
    assert (ref.records[2 * STACK:]["t"] == F(1.5)).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class GRays:
    """device buffers for one ray set: the offsets, and the four single-answer calls"""

    def __init__(self, ctx, drawer, rays):
        self.ctx, self.drawer, self.n = ctx, drawer, len(rays)
        self.rays = H().DataBuffer(ctx, self.n, L().RAY)
        self.rays.local[:] = rays
        self.rays.sync()
        self.offsets = H().DataBuffer(ctx, self.n + 1, np.uint64)
        self.hits = H().DataBuffer(ctx, self.n, L().HIT)
        self.flags = H().DataBuffer(ctx, self.n, np.uint32)
        self.rows = H().DataBuffer(ctx, self.n * KMAX, L().HIT)

    def count_only(self):
        self.offsets.fill_u32(0xDEADBEEF)
        self.drawer.gather_hits(self.rays, self.offsets)
        return self.offsets.get_data().copy()

    def gather(self):
        """count only -> a hits buffer of exactly M records -> the full form: (offsets, the M records as the walk left them)"""
        first = self.count_only()
        total = int(first[-1])
        assert total > 0
        out = H().DataBuffer(self.ctx, total, L().HIT)
        out.fill_u32(NAN_WORD)
        self.offsets.fill_u32(0xDEADBEEF)
        self.drawer.gather_hits(self.rays, self.offsets, out)
        off, rec = self.offsets.get_data().copy(), out.get_data().copy()
        out.dispose()
        assert (off == first).all()
        return off, rec

    def closest(self):
        self.hits.fill_u32(NAN_WORD)
        self.drawer.trace_closest(self.rays, self.hits)
        return self.hits.get_data().copy()

    def occluded(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.trace_occluded(self.rays, self.flags)
        return self.flags.get_data().copy()

    def counts(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.count_hits(self.rays, self.flags)
        return self.flags.get_data().copy()

    def khits(self, k):
        found = H().DataBuffer(self.ctx, self.n, np.uint32)
        self.rows.fill_u32(NAN_WORD)
        self.drawer.trace_k_closest(self.rays, k, self.rows, found)
        got, f = self.rows.get_data()[: self.n * k].reshape(self.n, k).copy(), found.get_data().copy()
        found.dispose()
        return got, f

    def dispose(self):
        for b in (self.rays, self.offsets, self.hits, self.flags, self.rows):
            b.dispose()


def assert_equal(off, rec, ref, what=""):
    """offsets equal; the canonical segments equal word for word"""
    assert off.dtype == np.uint64 and (off == ref.offsets).all(), (what, np.nonzero(off != ref.offsets)[0][:10])
    assert len(rec) == int(ref.offsets[-1])
    got = G.canonical(off, rec)
    bad = np.nonzero((rec_words(got) != rec_words(ref.records)).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:10], got[bad[:3]], ref.records[bad[:3]])


_CASES = {}


def parity_case(ctx, name):
    """(positions, rays, the reference from the library's boxes, drawer): the reference is computed once per scene; one context
    keeps one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _CASES:
        if name == "stack":
            a, b, c, rays, _ = coincident_stack()
        else:
            a, b, c = scene_positions(name)
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        lo, hi = library_boxes(d)
        if name != "stack":
            rays = mixed_rays_of(name, a, b, c, lo, hi)
        _CASES[name] = ((a, b, c), rays, G.reference(rays, a, b, c, lo, hi), d)
    _CASES[name][3].build_fast_scene()
    return _CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES + ["stack"])
def test_1_segments_equal_the_brute_force_word_for_word(ctx, name):
    _, rays, ref, d = parity_case(ctx, name)
    q = GRays(ctx, d, rays)
    off, rec = q.gather()                                              # the hits buffer is exactly M records long
    q.dispose()
    assert_equal(off, rec, ref, name)
    m = np.diff(off.astype(np.int64))
    long_, empty, inactive = exercised(rays, ref)
    print(f"{name}: M {int(off[-1])}, longest segment {int(m.max())}, {long_} of >= 32, {empty} empty of active rays, {inactive} inactive")
    if name == "sheets":
        assert len(rays) == 1500 and long_ > 50 and empty > 100 and inactive > 100      # see the CPU test above
    elif name == "stack":
        assert m.tolist() == [STACK, 0, 0, STACK, 0, STACK, 0, 0]
        assert (rec["t"][:STACK] == F(3.0)).all() and len(np.unique(rec["tri"][:STACK])) == STACK
    else:
        assert len(rays) == 1500


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_2_identities_with_the_shipped_calls(ctx, name):
    _, rays, ref, d = parity_case(ctx, name)
    q = GRays(ctx, d, rays)
    off, rec = q.gather()
    canon = G.canonical(off, rec)
    m = np.diff(off.astype(np.int64))
    one, flags, counts = q.closest(), q.occluded(), q.counts()
    assert (m == counts).all()                                         # segment length == lbvh_count_hits
    assert ((m > 0) == (flags == 1)).all()                             # non-empty == lbvh_trace_occluded
    rows1, _ = heads(off, canon, 1)
    assert (rec_words(rows1) == rec_words(one)).all()                  # the least record == lbvh_trace_closest (miss when empty)
    rows32, found32 = heads(off, canon, KMAX)
    got32, f32 = q.khits(KMAX)
    assert (f32 == found32).all()
    assert (words(rows32).reshape(q.n, -1) == words(got32).reshape(q.n, -1)).all()     # the sorted head == lbvh_trace_k_closest
    q.dispose()


@pytest.mark.gpu
def test_3_capacity_is_never_overrun_and_fitting_segments_are_complete(ctx):
    _, rays, ref, d = parity_case(ctx, "sheets")
    q = GRays(ctx, d, rays)
    total = int(ref.offsets[-1])
    big = H().DataBuffer(ctx, total + 64, L().HIT)
    lib, h, s = N().lib, ctx.handle, d.container.scene()
    ref_off = ref.offsets.astype(np.int64)
    for capacity in (total, total - 1, total // 2, 1):
        big.fill_u32(NAN_WORD)
        q.offsets.fill_u32(0xDEADBEEF)
        N().check(h, lib.lbvh_gather_hits(h, q.rays.device, q.n, C.byref(s), q.offsets.device, big.device, capacity))
        off, rec = q.offsets.get_data().copy(), big.get_data().copy()
        assert (off == ref.offsets).all(), capacity                    # the offsets do not depend on the capacity
        assert (words(rec[capacity:]) == NAN_WORD).all(), capacity     # no word at or beyond the capacity changed
        fits = np.nonzero(ref_off[1:] <= capacity)[0]                  # offsets rise: the fitting segments are a prefix
        end = int(ref_off[fits[-1] + 1]) if len(fits) else 0
        assert len(fits) == 0 or (fits == np.arange(len(fits))).all()
        got = G.canonical(off[: len(fits) + 1], rec[:end])
        assert (rec_words(got) == rec_words(ref.records[:end])).all(), capacity
        print(f"capacity {capacity}: {len(fits)} of {q.n} segments fit, {end} records checked")
        if capacity == total:
            assert len(fits) == q.n and end == total
    # capacity == 0 with d_hits == NULL: the same offsets, nothing else touched
    big.fill_u32(NAN_WORD)
    off = q.count_only()
    assert (off == ref.offsets).all()
    assert (words(big.get_data()) == NAN_WORD).all()
    big.dispose()
    q.dispose()


@pytest.mark.gpu
def test_4_lane_refill_reloads_the_write_position(ctx):
    _, rays, ref, d = parity_case(ctx, "sheets")
    q = GRays(ctx, d, rays)
    lib, h = N().lib, ctx.handle
    try:
        for cap in (1, 2, 3, 7):                                       # 1 500 rays on one wave: about 23 refills per lane
            N().check(h, lib.lbvh_debug_ray_waves(h, cap))
            off, rec = q.gather()
            assert_equal(off, rec, ref, f"waves <= {cap}")
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    off, rec = q.gather()
    assert_equal(off, rec, ref, "cap restored")
    q.dispose()


@pytest.mark.gpu
def test_5_output_does_not_depend_on_the_stack_split(ctx):
    _, rays, ref, d = parity_case(ctx, "sheets")
    q = GRays(ctx, d, rays)
    lib, h = N().lib, ctx.handle
    canon = []
    try:
        for split in (1, 16):                                          # 1: nearly every waiting sibling in the device-memory part
            N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
            off, rec = q.gather()
            assert_equal(off, rec, ref, f"split {split}")
            canon.append((off, G.canonical(off, rec)))
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert (canon[0][0] == canon[1][0]).all() and (rec_words(canon[0][1]) == rec_words(canon[1][1])).all()
    q.dispose()


@pytest.mark.gpu
def test_6_edge_rays(ctx):
    (a, b, c), rays, ref, d = parity_case(ctx, "sheets")
    lo, hi = library_boxes(d)
    act = np.nonzero(np.diff(ref.offsets.astype(np.int64)) > 0)[0]
    dead = make_rays(np.zeros((1, 3), dtype=F), np.array([[0, 0, 1]], dtype=F), F(1), F(0))[0]

    def check(set_, what, lists=True):
        r = G.reference(set_, a, b, c, lo, hi)
        q = GRays(ctx, d, set_)
        if lists:
            off, rec = q.gather()
            assert_equal(off, rec, r, what)
        else:                                                          # M == 0: no record may be written
            out = H().DataBuffer(ctx, 8, L().HIT)
            out.fill_u32(NAN_WORD)
            q.offsets.fill_u32(0xDEADBEEF)
            d.gather_hits(q.rays, q.offsets, out)
            assert (q.offsets.get_data() == 0).all() and (words(out.get_data()) == NAN_WORD).all()
            assert int(r.offsets[-1]) == 0
            out.dispose()
        q.dispose()

    edge = rays[act[:200]].copy()                                      # the first and the last ray inactive
    edge[0], edge[-1] = dead, dead
    check(edge, "first and last inactive")
    none = rays[:130].copy()                                           # all rays inactive: all-zero offsets, no hit written
    none["t_min"], none["t_max"] = F(2), F(1)
    check(none, "all inactive", lists=False)
    check(rays[act[:1]].copy(), "a count of 1")
    check(rays[act[np.arange(1025) % len(act)]].copy(), "1 025 rays: the offsets cross a scan tile")


@pytest.mark.gpu
def test_7_errors_scratch_failure_and_the_stack_limit(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        rng = np.random.default_rng(2)
        origin, direction = scene_rays(a, b, c, 3000, rng)
        rays = make_rays(origin, direction, F(1e-3), INF)
        lo, hi = library_boxes(d)
        ref = G.reference(rays, a, b, c, lo, hi)
        total = int(ref.offsets[-1])
        assert total > 1000
        q = GRays(c2, d, rays)
        out = H().DataBuffer(c2, total + 16, L().HIT)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(rays)
        fn = lib.lbvh_gather_hits

        def poison():
            out.fill_u32(NAN_WORD)
            q.offsets.fill_u32(0xDEADBEEF)

        def untouched():
            return (words(out.get_data()) == NAN_WORD).all() and (words(q.offsets.get_data()) == 0xDEADBEEF).all()

        def full():
            poison()
            assert fn(h, q.rays.device, n, C.byref(s), q.offsets.device, out.device, total) == 0
            return q.offsets.get_data().copy(), out.get_data()[:total].copy()

        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
        poison()
        assert fn(h, q.rays.device, n, C.byref(s), q.offsets.device, out.device, total) == -2
        assert untouched()
        assert_equal(*full(), ref, "after the failed reservation")
        # argument checks: LBVH_ERR_INVALID_ARG, nothing enqueued
        poison()
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        assert fn(None, q.rays.device, 10, C.byref(s), q.offsets.device, out.device, total) == -1
        assert fn(h, None, n, C.byref(s), q.offsets.device, out.device, total) == -1
        assert fn(h, q.rays.device, n, None, q.offsets.device, out.device, total) == -1
        assert fn(h, q.rays.device, n, C.byref(s), None, out.device, total) == -1
        assert fn(h, q.rays.device, n, C.byref(s), q.offsets.device, None, total) == -1       # NULL hits with a capacity
        assert fn(h, p(q.rays, 4), 10, C.byref(s), q.offsets.device, out.device, total) == -1
        assert fn(h, q.rays.device, 10, C.byref(s), q.offsets.device, p(out, 8), total) == -1
        assert fn(h, q.rays.device, 10, C.byref(s), p(q.offsets, 4), out.device, total) == -1
        assert fn(h, q.rays.device, 1 << 32, C.byref(s), q.offsets.device, out.device, total) == -1
        # count == 0: a no-op, d_offsets[0] included
        assert fn(h, q.rays.device, 0, C.byref(s), q.offsets.device, out.device, total) == 0
        assert untouched()
        # a stale scene: triangles uploaded without a rebuild
        d.container.triangle_data.sync()
        assert fn(h, q.rays.device, n, C.byref(s), q.offsets.device, out.device, total) == -1
        assert b"stale" in lib.lbvh_last_error(h)
        assert untouched()
        d.rebuild(fast=True)
        s = d.container.scene()
        # the stack limit: the library's own soft flag, reported at the next sync (LBVH_ERR_HIP), never a silently short segment
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        assert fn(h, q.rays.device, n, C.byref(s), q.offsets.device, out.device, total) == 0
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_equal(*full(), ref, "after the stack limit")
        out.dispose()
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_8_statistics_the_full_form_is_two_equal_walks(ctx):
    _, rays, ref, d = parity_case(ctx, "sheets")
    q = GRays(ctx, d, rays)
    out = H().DataBuffer(ctx, int(ref.offsets[-1]), L().HIT)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    per = []
    try:
        for hits in (None, out):
            stats.fill_u32(0)
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
            d.gather_hits(q.rays, q.offsets, hits)
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
            s = stats.get_data()[0]
            per.append((int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"])))
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    print("rays, node lines, triangle tests: count only", per[0], "full", per[1])
    assert per[0][0] == int(R.active(rays).sum()) and per[0][1] >= per[0][0] and per[0][2] >= int(ref.offsets[-1])
    assert per[1] == tuple(2 * v for v in per[0])
    for b in (stats, out):
        b.dispose()
    q.dispose()


@pytest.mark.gpu
def test_9_path_tracer_frame_undisturbed_by_a_call_between_bounces(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    # the same frame with the query issued between the bounces, 4x the frame's count: the ray scratch grows in mid-frame
    a, b, c = positions(tris)
    origin, direction = scene_rays(a, b, c, 4 * 160 * 96, np.random.default_rng(12))
    q = GRays(ctx, pt.drawer, make_rays(origin, direction, F(1e-3), F(25.0)))
    out = H().DataBuffer(ctx, 1 << 18, L().HIT)
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def gather():
        pt.drawer.gather_hits(q.rays, q.offsets, out)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    gather()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        gather()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    gather()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    m = np.diff(q.offsets.get_data().astype(np.int64))
    assert 0 < (m > 0).sum() < q.n and m.max() >= 2
    out.dispose()
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("t_max", [None, 1.0])
def test_10_cpp_host_driver_gather_matches_the_python_host(ctx, t_max):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    n, count = 4096, 20000
    args = [exe, "gather", str(count)] + ([str(t_max)] if t_max is not None else [])
    res = json.loads(subprocess.run(args, check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(n)                                 # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    origin, direction = driver_rays(lo, hi, count)                     # and its rays (seed 3): origin and target drawn axis by axis
    rays = make_rays(origin, direction, F(0.0), INF if t_max is None else F(t_max))
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    rb = H().DataBuffer(ctx, count, L().RAY)
    rb.local[:] = rays
    rb.sync()
    off, rec = d.all_hits(rb, sort=True)
    total = int(off[-1])
    m = np.diff(off.astype(np.int64))
    assert res["triangles"] == n and res["rays"] == count
    assert res["total"] == total == len(rec) and res["nonempty"] == int((m > 0).sum())
    assert res["word_sum"] == int(words(rec).astype(np.uint64).sum())
    weighted = sum((i + 1) * int(t) for i, t in enumerate(rec["tri"].tolist())) & ((1 << 64) - 1)
    assert res["weighted_sum"] == weighted
    assert [[t for _, t in row] for row in res["rows"]] == [rec["tri"][off[i]: off[i + 1]].tolist() for i in range(3)]
    assert 0 < res["nonempty"] < count and total > res["nonempty"]     # some rays cross more than one triangle
    # all_hits(sort=True): every segment in (t, tri) order, and equal to the reference
    la, lb = library_boxes(d)
    ref = G.reference(rays, pos[:, 0], pos[:, 1], pos[:, 2], la, lb)
    assert (off == ref.offsets).all() and (rec_words(rec) == rec_words(ref.records)).all()
    unsorted_off, unsorted = d.all_hits(rb)
    assert (unsorted_off == off).all() and (rec_words(G.canonical(unsorted_off, unsorted)) == rec_words(rec)).all()
    rb.dispose()
    d.on_destroy()
