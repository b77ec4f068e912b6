"""lbvh_triangle_cast_all: every triangle a moving triangle touches, as a CSR list, over the four-wide derived traversal scene.
The expectation is tests/triangle_cast_all_reference.py: the per-pair pieces of tests/triangle_cast_reference.py under the list rule
of tests/cast_all_reference.py, brute force over every (cast, triangle) pair with the boxes the library produced.  Every GPU
comparison is word for word on uint32 views, no tolerance.  Scenes and casts are those of tests/test_triangle_cast.py, imported."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hostile_scenes as HS
import triangle_cast_all_reference as TA
import triangle_cast_reference as TR
import triangle_query_reference as TQ
from query_support import driver_mesh, H, L, library_boxes, N, pack, padded_boxes, positions, words
from test_triangle_cast import _casts, BIG, inactive_forms, KNOWN, parity_casts, scene_positions, TILT
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
NAME = "lbvh_triangle_cast_all"
SETS = ("big", "soup64", "grid_80x80", "driver")
NAN_WORD = 0x7FC00000
START = 16                                  # LBVH_TRI_CAST_START
MISS = TR.MISS


def rec_words(r):
    return words(r).reshape(-1, 4)


# ---- CPU: the surface in every layer ------------------------------------------------------------------------------------

def test_surface_in_every_layer():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"lbvh_status lbvh_triangle_cast_all\(lbvh_context\* ctx, const lbvh_tri_ray\* d_casts, size_t count, "
                     r"const lbvh_scene\* h_scene,\s+uint64_t\* d_offsets, lbvh_tri_cast_hit\* d_hits, uint64_t capacity\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    assert h.index("lbvh_status lbvh_triangle_cast_any(") < h.index("lbvh_status lbvh_triangle_cast_all(")
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert NAME in bounce
    doc = h[h.index("Every triangle a moving triangle touches"):h.index("lbvh_status lbvh_triangle_cast_all(")]
    doc = re.sub(r"\s*\n \*\s+", " ", doc)                                 # (the comment's line breaks are not part of the wording)
    for must in ("NOT PART OF THE CONTRACT", "lbvh_sort_hit_segments applies unchanged", "d_offsets[0] included", "A NaN never counts",
                 "exactly when lbvh_triangle_cast_any gives 1", "word for word", "feature & LBVH_TRI_CAST_START", "now exists",
                 "LBVH_ERR_OUT_OF_MEMORY with nothing written", "lbvh_debug_ray_waves", "lbvh_debug_ray_stack_split",
                 "lbvh_debug_ray_stack_limit", "lbvh_ray_stats_target", "`skip` is not counted"):
        assert must in doc, must
    res, args = N().SIGNATURES[NAME]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64 and N().ABI_VERSION == 11
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    row = r"\(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,\s+ulong capacity\);"
    assert re.search(r"public static extern int lbvh_triangle_cast_all" + row, cs) and re.search(r"public static extern int lbvh_box_cast_all" + row, cs)
    cg = open(os.path.join(ROOT, "bindings", "csharp", "CastGather.cs")).read()
    assert "public void TriangleCastAll(" in cg and "lbvh_triangle_cast_all(" in cg and "unsafe" not in cg and "Check(casts, 64," in cg
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void TriangleCastAll(" in hpp and "DataBuffer<lbvh_tri_cast_hit>& hits, size_t count)" in hpp
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, k) for k in ("triangle_cast_all", "mesh_sweep_all", "cast_all"))
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert "castall triangle" in drv and '"triangle"' in drv
    assert "lbvh_triangle_cast_all" in open(os.path.join(ROOT, "README.md")).read()
    assert "lbvh_triangle_cast_all" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lbvh_triangle_cast_all" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_native_library_exports_the_entry_point():
    assert getattr(N().lib, NAME).argtypes is not None


# ---- CPU: known answers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", [BIG, TILT], ids=["big", "tilt"])
def test_known_answers_one_record_with_the_first_contact_words(scene):
    rows = [k for k in KNOWN if k[0] is scene]
    casts = _casts([k[1:7] for k in rows])
    a, b, c = scene
    lo, hi = padded_boxes(a, b, c)
    all_, first = TA.reference(casts, a, b, c, lo, hi), TR.reference(casts, a, b, c, lo, hi)
    m = np.diff(all_.offsets.astype(np.int64))
    assert m.tolist() == [0 if k[7] is None else 1 for k in rows] and m.sum() >= 1
    assert (rec_words(all_.records) == rec_words(first.records[m == 1])).all()
    for k, seg in zip(rows, np.split(all_.records, all_.offsets[1:-1].astype(np.int64))):
        if k[7] is not None:
            assert (float(seg["t"][0]), int(seg["feature"][0]), float(seg["w"][0])) == k[7] and seg["tri"][0] == 0
        if k[7] is not None and k[7][1] >= START:                          # starting in overlap: t = +0 and the start bit
            assert words(seg["t"])[0] == 0 and seg["feature"][0] & 16


def test_every_inactive_form_has_an_empty_segment():
    casts = inactive_forms()
    a, b, c = BIG
    r = TA.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert len(casts) == 42 and (r.offsets == 0).all() and len(r.records) == 0


# ---- the sets, their references computed once ------------------------------------------------------------------------------

_CPU = {}


def cpu_case(name):
    """(positions, casts, the list reference, the first-contact reference) with the CPU's padded boxes"""
    if name not in _CPU:
        a, b, c = scene_positions("grid_80x80" if name == "plough" else name)
        casts = plough_casts() if name == "plough" else parity_casts(name, a, b, c)
        lo, hi = padded_boxes(a, b, c)
        _CPU[name] = ((a, b, c), casts, TA.reference(casts, a, b, c, lo, hi), TR.reference(casts, a, b, c, lo, hi))
    return _CPU[name]


def plough_casts():
    """16 blades on grid_80x80 (z = 0, x and y in [-4, 4]): triangles with edges of about 30 % of the extent that stand across the
    sheet — one vertex below it, two above — and are swept through it along x, y or a diagonal over the whole grid (t_max = 1)"""
    rng = np.random.default_rng(4242)
    ext = 8.0
    rows = []
    for i in range(16):
        angle = (i % 8) * np.pi / 4 + rng.uniform(-0.1, 0.1)
        along = np.array([np.cos(angle), np.sin(angle), 0.0])
        across = np.array([-along[1], along[0], 0.0])
        start = -along * 0.55 * ext + across * rng.uniform(-0.3, 0.3) * ext
        half = 0.15 * ext * rng.uniform(0.9, 1.1)
        lean = along * rng.uniform(-0.2, 0.2)
        qa = start - across * half + np.array([0, 0, 0.4]) + lean
        qb = start + across * half + np.array([0, 0, 0.5]) - lean
        qc = start + across * rng.uniform(-0.2, 0.2) * half + np.array([0, 0, -0.3 * ext * rng.uniform(0.9, 1.1) + 0.45])
        move = along * 1.1 * ext + np.array([0, 0, rng.uniform(-0.05, 0.05)])
        rows.append((qa, qb, qc, move, 1.0, TR.NULL))
    return _casts(rows)


@pytest.mark.parametrize("name", SETS + ("plough",))
def test_reference_against_reference_the_least_record_is_the_first_contact(name):
    _, casts, ref, first = cpu_case(name)
    least = TA.least(ref.offsets, ref.records, MISS)
    assert (rec_words(least) == rec_words(first.records)).all()
    assert (first.flags == (np.diff(ref.offsets.astype(np.int64)) >= 1)).all()
    off = ref.offsets.astype(np.int64)
    for q in range(len(casts)):                                           # every segment is in (t, tri) order and holds a triangle once
        seg = ref.records[off[q]:off[q + 1]]
        assert (np.lexsort((seg["tri"], seg["t"])) == np.arange(len(seg))).all() and len(set(seg["tri"].tolist())) == len(seg)
        assert casts["skip"][q] not in seg["tri"]


@pytest.mark.parametrize("name", SETS)
def test_the_sets_are_not_vacuous(name):
    _, casts, ref, _ = cpu_case(name)
    act = TR.active(casts)
    m = np.diff(ref.offsets.astype(np.int64))
    f = ref.records["feature"]
    print(f"{name}: {len(casts)} casts, {int(act.sum())} active, {int(m.sum())} records, longest {int(m.max())}, {int((m >= 2).sum())} with two or more, "
          f"by feature {np.bincount(f, minlength=22).tolist()}")
    assert len(casts) == 130 and (~act).sum() > 0 and (casts["skip"][act] != TR.NULL).sum() > 0
    # `big` is one triangle and a far dummy: no cast aimed at the one can reach both, so its segments hold one record at the most
    assert (m >= 2).sum() >= 10 if name != "big" else ((m == 1).sum() >= 10 and m.max() == 1)
    assert (f <= 5).any() and ((f >= 6) & (f <= 14)).any() and ((f >= 16) & (f <= 21)).any()
    assert (((f <= 14) | ((f >= 16) & (f <= 21)))).all()


def test_the_plough_set_has_long_segments():
    _, casts, ref, _ = cpu_case("plough")
    m = np.diff(ref.offsets.astype(np.int64))
    print("plough: records per cast", m.tolist())
    assert len(casts) == 16 and TR.active(casts).all()
    assert (m > 256).sum() >= 1 and (m > 64).sum() >= 8                    # the segment sort's workgroup path meets these records


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Sweeps:
    """the casts on the device, offsets for count + 1 (+ 1 poisoned) entries, and the first-contact / any buffers"""

    def __init__(self, ctx, drawer, casts):
        self.ctx, self.drawer, self.n = ctx, drawer, len(casts)
        self.casts = H().DataBuffer(ctx, self.n, L().TRI_RAY)
        self.casts.local[:] = casts
        self.casts.sync()
        self.offsets = H().DataBuffer(ctx, self.n + 2, np.uint64)
        self.hits = H().DataBuffer(ctx, max(self.n, 1), L().TRI_CAST_HIT)
        self.flags = H().DataBuffer(ctx, max(self.n, 1), np.uint32)
        self.fn = getattr(N().lib, NAME)

    def count_only(self):
        self.offsets.fill_u32(0xDEADBEEF)
        self.drawer.triangle_cast_all(self.casts, self.offsets)
        got = self.offsets.get_data().copy()
        assert got[self.n + 1] == 0xDEADBEEFDEADBEEF
        return got[: self.n + 1]

    def gather(self, device_sort=False, tail=8):
        """count only -> a buffer of M + tail records -> the full form: (offsets, the M records); the tail keeps its poison"""
        first = self.count_only()
        total = int(first[-1])
        out = H().DataBuffer(self.ctx, total + tail, L().TRI_CAST_HIT)
        out.fill_u32(NAN_WORD)
        self.offsets.fill_u32(0xDEADBEEF)
        self.drawer.triangle_cast_all(self.casts, self.offsets, out)
        if device_sort:
            H().sort_hit_segments(self.ctx, self.offsets, out, self.n)
        off, rec = self.offsets.get_data()[: self.n + 1].copy(), out.get_data().copy()
        out.dispose()
        assert (off == first).all() and (words(rec[total:]) == NAN_WORD).all()
        return off, rec[:total]

    def first(self):
        self.hits.fill_u32(NAN_WORD)
        self.drawer.triangle_cast(self.casts, self.hits)
        return self.hits.get_data()[: self.n].copy()

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.triangle_cast_any(self.casts, self.flags)
        return self.flags.get_data()[: self.n].copy()

    def dispose(self):
        for b in (self.casts, self.offsets, self.hits, self.flags):
            b.dispose()


def assert_equal(off, rec, ref, what="", canonical=True):
    """offsets equal; the canonical segments equal word for word"""
    assert off.dtype == np.uint64 and (off == ref.offsets).all(), (what, np.nonzero(off != ref.offsets)[0][:10])
    assert len(rec) == int(ref.offsets[-1])
    got = TA.canonical(off, rec) if canonical else rec
    bad = np.nonzero((rec_words(got) != rec_words(ref.records)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], ref.records[bad[:3]])


_SCENES, _CASES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cached_scenes():
    """the parity scenes stay on the device for the tests of this file only"""
    yield
    for entry in _SCENES.values():
        entry[2].on_destroy()
    _SCENES.clear()
    _CASES.clear()


def gpu_case(ctx, name, scene=None, casts=None):
    """(positions, casts, the reference from the LIBRARY's boxes, drawer): one drawer per scene, one reference per set; one context
    keeps one derived traversal scene, so the scene is derived again for the test that asks"""
    scene = scene or ("grid_80x80" if name == "plough" else name)
    if scene not in _SCENES:
        a, b, c = scene_positions(scene)
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        _SCENES[scene] = ((a, b, c), library_boxes(d), d)
    (a, b, c), (lo, hi), d = _SCENES[scene]
    if name not in _CASES:
        if casts is None:
            casts = plough_casts() if name == "plough" else parity_casts(scene, a, b, c)
        _CASES[name] = (casts, TA.reference(casts, a, b, c, lo, hi))
    d.build_fast_scene()
    return (a, b, c), _CASES[name][0], _CASES[name][1], d


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS + ("plough",))
def test_g1_segments_equal_the_brute_force_word_for_word(ctx, name):
    _, casts, ref, d = gpu_case(ctx, name)
    q = Sweeps(ctx, d, casts)
    off, rec = q.gather()
    m = np.diff(ref.offsets.astype(np.int64))
    print(f"{name}: {len(casts)} casts, {int(m.sum())} records, longest {int(m.max())}, {int((m == 0).sum())} empty")
    assert_equal(off, rec, ref, name)
    for kw in ({"sort": True}, {"device_sort": True}):                     # the convenience call: ordered on the host and on the device
        off2, rec2 = d.cast_all(q.casts, **kw)
        assert rec2.dtype == L().TRI_CAST_HIT
        assert_equal(off2, rec2, ref, (name, kw), canonical=False)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS + ("plough",))
def test_g2_the_device_segment_sort_gives_the_reference_order(ctx, name):
    _, casts, ref, d = gpu_case(ctx, name)
    q = Sweeps(ctx, d, casts)
    off, rec = q.gather(device_sort=True)
    q.dispose()
    assert_equal(off, rec, ref, name, canonical=False)                     # no host sort: feature and w travelled with their record


@pytest.mark.gpu
def test_g3_identities_between_the_device_calls(ctx):
    """m >= 1 <=> _cast_any; the least record is lbvh_triangle_cast's; two calls write the same bytes; every triangle that
    lbvh_triangle_intersections lists for {a, b, c, skip} is in the segment at +0 with the start bit, except the pairs the
    references themselves exclude (the grown-box rule of the definition): those are counted and printed, and the device must
    agree with the references on them."""
    starts = 0
    for name in ("soup64", "grid_80x80"):
        (a, b, c), casts, ref, d = gpu_case(ctx, name)
        lo, hi = _SCENES[name][1]
        q = Sweeps(ctx, d, casts)
        off, rec = q.gather()
        off2, rec2 = q.gather()
        assert (off == off2).all() and (words(rec) == words(rec2)).all()
        first, flags = q.first(), q.any()
        m = np.diff(off.astype(np.int64))
        assert (flags == (m >= 1)).all()
        canon = TA.canonical(off, rec)
        assert (rec_words(TA.least(off, canon, MISS)) == rec_words(first)).all()
        tq = H().DataBuffer(ctx, len(casts), L().TRI_QUERY)
        tq.local[:] = TQ.make_queries(casts["a"], casts["b"], casts["c"], casts["skip"])
        tq.sync()
        t_off, tris = d.intersections(tq, device_sort=True)
        tq.dispose()
        q.dispose()
        pairs = {qi: (listed, admitted) for qi, listed, admitted in TA.start_pairs(casts, a, b, c, lo, hi)}
        listed_n = excepted = 0
        for qi in np.nonzero(TR.active(casts))[0]:
            listed = set(tris[int(t_off[qi]):int(t_off[qi + 1])].tolist())
            ref_listed, admitted = pairs.get(int(qi), (set(), set()))
            assert listed == ref_listed, (name, qi)
            seg = canon[int(off[qi]):int(off[qi + 1])]
            at_start = seg[(words(seg["t"]) == 0) & ((seg["feature"] & START) != 0)]
            assert set(at_start["tri"].tolist()) & listed == admitted, (name, qi)      # the device agrees with the references
            listed_n += len(listed)
            excepted += len(listed - admitted)
            starts += len(at_start)
        print(f"{name}: {listed_n} triangles listed at the start pose, {excepted} excluded by the grown-box rule of the definition")
    assert starts >= 20


@pytest.mark.gpu
def test_g4_capacity_is_never_overrun_and_fitting_segments_are_complete(ctx):
    _, casts, ref, d = gpu_case(ctx, "grid_80x80")
    q = Sweeps(ctx, d, casts)
    total = int(ref.offsets[-1])
    big = H().DataBuffer(ctx, total + 64, L().TRI_CAST_HIT)
    h, s = ctx.handle, d.container.scene()
    ref_off = ref.offsets.astype(np.int64)
    assert total > 200
    for capacity in (0, 1, total // 2, total - 1, total):
        big.fill_u32(NAN_WORD)
        q.offsets.fill_u32(0xDEADBEEF)
        N().check(h, q.fn(h, q.casts.device, q.n, C.byref(s), q.offsets.device, big.device, capacity))
        off, rec = q.offsets.get_data()[: q.n + 1].copy(), big.get_data().copy()
        assert (off == ref.offsets).all(), capacity                    # the offsets do not depend on the capacity
        assert (words(rec[capacity:]) == NAN_WORD).all(), capacity     # no word at or beyond the capacity changed
        fits = np.nonzero(ref_off[1:] <= capacity)[0]                  # offsets rise: the fitting segments are a prefix
        end = int(ref_off[fits[-1] + 1]) if len(fits) else 0
        assert len(fits) == 0 or (fits == np.arange(len(fits))).all()
        got = TA.canonical(off[: len(fits) + 1], rec[:end])
        assert (rec_words(got) == rec_words(ref.records[:end])).all(), capacity
        if capacity == total:
            assert len(fits) == q.n and end == total
        if capacity == total // 2:
            assert 0 < len(fits) < q.n
    big.fill_u32(NAN_WORD)                                             # capacity == 0 with d_hits == NULL: the same offsets
    assert (q.count_only() == ref.offsets).all()
    assert (words(big.get_data()) == NAN_WORD).all()
    big.dispose()
    q.dispose()


@pytest.mark.gpu
def test_g5_lane_refill_reloads_the_write_position(ctx):
    (a, b, c), casts, _, d = gpu_case(ctx, "soup64")
    casts = np.resize(casts, 1500)                                     # the set, repeated up to 1 500
    ref = TA.reference(casts, a, b, c, *_SCENES["soup64"][1])
    q = Sweeps(ctx, d, casts)
    h, lib = ctx.handle, N().lib
    seen = []
    try:
        for cap in (1, 2, 3, 7):                                       # 1 500 casts on one wave: about 23 refills per lane
            N().check(h, lib.lbvh_debug_ray_waves(h, cap))
            off, rec = q.gather()
            assert_equal(off, rec, ref, f"waves <= {cap}")
            seen.append(words(TA.canonical(off, rec)))
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert all((s == seen[0]).all() for s in seen)
    assert_equal(*q.gather(), ref, "cap restored")
    q.dispose()


@pytest.mark.gpu
def test_g6_output_does_not_depend_on_the_stack_split(ctx):
    _, casts, ref, d = gpu_case(ctx, "plough")
    q = Sweeps(ctx, d, casts)
    h, lib = ctx.handle, N().lib
    canon = []
    try:
        assert lib.lbvh_debug_ray_stack_split(h, 0) == -1              # the hook takes 1 .. the LDS depth: 0 is rejected, nothing changes
        for split in (1, 4, 16):                                       # 1: nearly every waiting sibling in the device-memory part
            N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
            off, rec = q.gather()
            assert_equal(off, rec, ref, f"split {split}")
            canon.append(words(TA.canonical(off, rec)))
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert (canon[0] == canon[1]).all() and (canon[1] == canon[2]).all()
    q.dispose()


@pytest.mark.gpu
def test_g7_edges(ctx):
    (a, b, c), casts, ref, d = gpu_case(ctx, "soup64")
    lo, hi = _SCENES["soup64"][1]
    m = np.diff(ref.offsets.astype(np.int64))
    live = np.nonzero(m > 0)[0]

    def check(set_, what):
        q = Sweeps(ctx, d, set_)
        r = TA.reference(set_, a, b, c, lo, hi)
        off, rec = q.gather()
        assert_equal(off, rec, r, what)
        q.dispose()
        return r

    for count in (1, 63, 64, 65):
        check(np.resize(casts[live], count), f"a count of {count}")
    # a tiny t_max: only the start records remain
    tiny = casts[live].copy()
    tiny["t_max"] = F(1e-30)
    r = check(tiny, "a tiny t_max")
    assert len(r.records) > 0 and (words(r.records["t"]) == 0).all() and (r.records["feature"] >= START).all()
    # skip removes exactly that triangle's record
    multi = casts[np.nonzero(m >= 2)[0]].copy()
    multi["skip"] = TR.NULL
    before = check(multi, "no skip")
    off = before.offsets.astype(np.int64)
    victim = before.records["tri"][off[:-1] + 1]                       # the second record of every segment
    multi["skip"] = victim
    after = check(multi, "skip = the second record's triangle")
    gone = np.ones(len(before.records), dtype=bool)
    gone[off[:-1] + 1] = False
    assert (rec_words(after.records) == rec_words(before.records[gone])).all()
    # count == 0 touches nothing, d_offsets[0] included
    q = Sweeps(ctx, d, casts)
    out = H().DataBuffer(ctx, 8, L().TRI_CAST_HIT)
    out.fill_u32(NAN_WORD)
    q.offsets.fill_u32(0xDEADBEEF)
    s = d.container.scene()
    assert q.fn(ctx.handle, q.casts.device, 0, C.byref(s), q.offsets.device, out.device, 8) == 0
    assert (words(q.offsets.get_data()) == 0xDEADBEEF).all() and (words(out.get_data()) == NAN_WORD).all()
    # all casts inactive: all-zero offsets, no record written; capacity == 0 with NULL hits is accepted
    dead = inactive_forms()
    qd = Sweeps(ctx, d, dead)
    qd.offsets.fill_u32(0xDEADBEEF)
    qd.drawer.triangle_cast_all(qd.casts, qd.offsets, out)
    assert (qd.offsets.get_data()[: qd.n + 1] == 0).all() and (words(out.get_data()) == NAN_WORD).all()
    assert q.fn(ctx.handle, qd.casts.device, qd.n, C.byref(s), qd.offsets.device, None, 0) == 0
    assert (qd.offsets.get_data()[: qd.n + 1] == 0).all()
    for x in (q, qd, out):
        x.dispose()


@pytest.mark.gpu
def test_g8_errors_scratch_failure_and_the_stack_limit(ctx):
    from test_triangle_cast import aimed_casts, extent_of, SIZES
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        ext = extent_of(a, b, c)
        casts = aimed_casts(a, b, c, 600, np.random.default_rng(2), [s * ext for s in SIZES])
        ref = TA.reference(casts, a, b, c, *library_boxes(d))
        total = int(ref.offsets[-1])
        assert total > 300
        q = Sweeps(c2, d, casts)
        out = H().DataBuffer(c2, total + 16, L().TRI_CAST_HIT)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n, fn, who = len(casts), q.fn, NAME.encode() + b": invalid argument: "

        def poison():
            out.fill_u32(NAN_WORD)
            q.offsets.fill_u32(0xDEADBEEF)

        def untouched():
            return (words(out.get_data()) == NAN_WORD).all() and (words(q.offsets.get_data()) == 0xDEADBEEF).all()

        def full():
            poison()
            assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, out.device, total) == 0
            return q.offsets.get_data()[: n + 1].copy(), out.get_data()[:total].copy()

        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
        poison()
        assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, out.device, total) == -2
        assert untouched()
        assert_equal(*full(), ref, "after the failed reservation")
        # argument checks: LBVH_ERR_INVALID_ARG with the entry point's name, nothing enqueued
        poison()
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        assert fn(None, q.casts.device, 10, C.byref(s), q.offsets.device, out.device, total) == -1
        null = who + b"d_casts != nullptr && h_scene != nullptr && d_offsets != nullptr"
        for args in ((None, n, C.byref(s), q.offsets.device, out.device, total), (q.casts.device, n, None, q.offsets.device, out.device, total),
                     (q.casts.device, n, C.byref(s), None, out.device, total)):
            assert fn(h, *args) == -1 and lib.lbvh_last_error(h) == null
        assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, None, total) == -1       # NULL hits with a capacity
        assert lib.lbvh_last_error(h) == who + b"d_hits != nullptr || capacity == 0"
        for args in ((p(q.casts, 4), 10, C.byref(s), q.offsets.device, out.device, total), (q.casts.device, 10, C.byref(s), q.offsets.device, p(out, 8), total),
                     (q.casts.device, 10, C.byref(s), p(q.offsets, 4), out.device, total)):
            assert fn(h, *args) == -1 and lib.lbvh_last_error(h).startswith(who + b"((uintptr_t)d_casts & 15) == 0")
        assert fn(h, q.casts.device, 1 << 32, C.byref(s), q.offsets.device, out.device, total) == -1
        assert lib.lbvh_last_error(h) == who + b"count <= 0xFFFFFFFFull"
        assert fn(h, q.casts.device, 0, C.byref(s), q.offsets.device, out.device, total) == 0      # count == 0: a no-op
        assert untouched()
        # a stale scene: triangles uploaded without a rebuild; the message names the entry point
        d.container.triangle_data.sync()
        assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, out.device, total) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(NAME.encode() + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        s = d.container.scene()
        # the stack limit: the library's own soft flag, reported at the next sync (LBVH_ERR_HIP), never a silently short segment
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, out.device, total) == 0
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
def test_g9_statistics_two_equal_walks_and_skip_is_not_counted(ctx):
    _, casts, ref, d = gpu_case(ctx, "grid_80x80")
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    h, lib = ctx.handle, N().lib
    total = int(ref.offsets[-1])
    out = H().DataBuffer(ctx, total, L().TRI_CAST_HIT)

    def counted(call):
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            call()
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        s = stats.get_data()[0]
        return int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"])

    q = Sweeps(ctx, d, casts)
    # the same casts with skip = a candidate of their own: the walk is the same (nothing shrinks), that one line is not counted
    m = np.diff(ref.offsets.astype(np.int64))
    free = casts.copy()
    free["skip"] = TR.NULL
    owned = free.copy()
    r_free = TA.reference(free, *_SCENES["grid_80x80"][0], *_SCENES["grid_80x80"][1])
    mf = np.diff(r_free.offsets.astype(np.int64))
    owned["skip"][mf > 0] = r_free.records["tri"][r_free.offsets.astype(np.int64)[:-1][mf > 0]]
    qf, qo = Sweeps(ctx, d, free), Sweeps(ctx, d, owned)
    try:
        one = counted(lambda: q.drawer.triangle_cast_all(q.casts, q.offsets))
        two = counted(lambda: q.drawer.triangle_cast_all(q.casts, q.offsets, out))
        assert_equal(q.offsets.get_data()[: q.n + 1].copy(), out.get_data().copy(), ref, "the counting kernels")
        without = counted(lambda: qf.drawer.triangle_cast_all(qf.casts, qf.offsets))
        with_skip = counted(lambda: qo.drawer.triangle_cast_all(qo.casts, qo.offsets))
    finally:
        for x in (stats, out, q, qf, qo):
            x.dispose()
    print(f"casts, node lines, triangle lines: count only {one}, full {two}; without skip {without}, with skip {with_skip}")
    assert one[0] == int(TR.active(casts).sum()) and one[1] >= one[0] and one[2] >= total and m.sum() == total
    assert two == tuple(2 * x for x in one)
    assert with_skip[:2] == without[:2] and without[2] - with_skip[2] == int((mf > 0).sum()) > 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_g10_hostile_scenes_word_for_word(ctx, name):
    """the scenes and the casts of test_t8 of the first-contact file"""
    a, b, c = scene_positions(name)
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    try:
        casts = parity_casts(name, a, b, c)
        ref = TA.reference(casts, a, b, c, *library_boxes(d))
        q = Sweeps(ctx, d, casts)
        off, rec = q.gather()
        q.dispose()
    finally:
        d.on_destroy()
    assert_equal(off, rec, ref, name)
    assert int(ref.offsets[-1]) > 10, name


@pytest.mark.gpu
def test_g11_mesh_sweep_all_is_the_join_of_the_per_triangle_casts(ctx):
    (a, b, c), _, _, d = gpu_case(ctx, "soup64")
    lo, hi = _SCENES["soup64"][1]
    other = tuple(x[:40] + np.array([0, 0, 40], dtype=F) for x in (a, b, c))     # a copy of 40 triangles, lifted
    for direction, t_max in (([0, 0, -1], 60.0), ([0.1, 0, -1], 25.0), ([0, 0, 1], 60.0)):
        ref = TA.reference(H().tri_casts_from_mesh(other, direction, t_max), a, b, c, lo, hi)
        moving = np.repeat(np.arange(40), np.diff(ref.offsets.astype(np.int64)))
        order = np.lexsort((ref.records["tri"], moving, ref.records["t"]))
        got = d.mesh_sweep_all(other, direction, t_max)
        assert len(got) == 5 and (got[0] == moving[order]).all()
        for col, key in zip(got[1:], ("tri", "t", "feature", "w")):
            assert (words(col) == words(ref.records[key][order])).all(), key
        loose = d.mesh_sweep_all(other, direction, t_max, sort=False)
        assert sorted(zip(loose[0].tolist(), loose[1].tolist())) == sorted(zip(moving.tolist(), ref.records["tri"].tolist()))
        record, index = d.mesh_sweep(other, direction, t_max)
        if len(moving):
            assert index == got[0][0] and record["tri"] == got[1][0] and words(record["t"]) == words(got[2][:1])
            assert record["feature"] == got[3][0] and words(record["w"]) == words(got[4][:1])
        else:
            assert index == -1
    assert len(d.mesh_sweep_all(other, [0, 0, -1], 60.0)[0]) > 40


@pytest.mark.gpu
def test_g12_cpp_host_driver_castall_triangle_matches_the_python_host(ctx):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "castall", "triangle", str(count)], check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(4096)
    casts = TR.driver_casts(lo, hi, count, 3, 2.0)                      # castall's defaults: seed 3, t_max 2
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Sweeps(ctx, d, casts)
    off, rec = q.gather(device_sort=True)
    flags = q.any()
    q.dispose()
    d.on_destroy()
    m = np.diff(off.astype(np.int64))
    total = int(off[-1])
    assert res["shape"] == "triangle" and res["triangles"] == len(tris) and res["casts"] == count and F(res["t_max"]) == F(2.0)
    assert res["total"] == total > 0 and res["nonempty"] == int((m > 0).sum()) == res["flagged"] == int(flags.sum())
    assert res["first_equal"] == count and res["longest"] == int(m.max()) and res["at_start"] == int((rec["t"] == 0).sum())
    assert res["word_sum"] == int(words(rec).astype(np.uint64).sum())
    weights = np.arange(1, total + 1, dtype=np.uint64)
    assert res["weighted_sum"] == int((weights * rec["tri"].astype(np.uint64)).sum(dtype=np.uint64))
    for row, k in zip(res["rows"], range(3)):
        seg = rec[int(off[k]):int(off[k + 1])]
        assert [r[1] for r in row] == seg["tri"].tolist()
        assert [words(np.array(r[0], dtype=F))[0] for r in row] == words(seg["t"]).tolist()
    assert 0 < res["nonempty"] < count
