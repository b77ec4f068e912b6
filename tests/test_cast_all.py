"""lbvh_sphere_cast_all / lbvh_capsule_cast_all / lbvh_box_cast_all: every triangle a swept sphere, capsule or box touches before
its t_max, as a CSR list, over the four-wide derived traversal scene.  The expectation is tests/cast_all_reference.py: the
per-pair pieces of the three first-contact references in numpy float32, brute force over every (cast, triangle) pair with the
boxes the library produced.  Every GPU comparison is word for word on uint32 views, no tolerance."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import box_cast_reference as BR
import capsule_reference as CR
import cast_all_reference as CA
import sweep_reference as SR
import test_box_cast as TB
import test_capsule_cast as TC
import test_sphere_cast as TS
from query_support import driver_mesh, driver_rays, H, L, library_boxes, N, pack, padded_boxes, positions, stacked_sheets, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
NAN_WORD = 0x7FC00000
SHAPES = ("sphere", "capsule", "box")
SCENES = ("cfg1_4096", "grid_80x80", "sheets")
COUNT = 600                                 # aimed casts per shape and scene; the grid gets the plough set on top
REF = {"sphere": SR, "capsule": CR, "box": BR}
GEN = {"sphere": TS, "capsule": TC, "box": TB}
ENTRY = {"sphere": "lbvh_sphere_cast_all", "capsule": "lbvh_capsule_cast_all", "box": "lbvh_box_cast_all"}


def rec_words(a):
    return words(a).reshape(-1, 4)


def ray_layout(shape):
    return {"sphere": L().SPHERE_RAY, "capsule": L().CAPSULE_RAY, "box": L().BOX_RAY}[shape]


def hit_layout(shape):
    return L().BOX_HIT if shape == "box" else L().HIT


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_the_three_prototypes_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    for fn, cast, hit in (("lbvh_sphere_cast_all", "lbvh_sphere_ray", "lbvh_hit"), ("lbvh_capsule_cast_all", "lbvh_capsule_ray", "lbvh_hit"),
                          ("lbvh_box_cast_all", "lbvh_box_ray", "lbvh_box_hit")):
        assert re.search(r"lbvh_status " + fn + r"\(lbvh_context\* ctx, const " + cast + r"\* d_casts, size_t count, const lbvh_scene\* h_scene,\s+"
                         r"uint64_t\* d_offsets, " + hit + r"\* d_hits, uint64_t capacity\);", h), fn
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert all(fn in bounce for fn in ENTRY.values())                      # listed among the calls that drop the live-path list
    doc = h[h.index("EVERY contact along"):h.index("lbvh_status lbvh_sphere_cast_all(")]
    assert "NOT PART OF THE CONTRACT" in doc and "lbvh_sort_hit_segments applies unchanged" in doc


def test_native_signatures_have_seven_arguments():
    nat = N()
    for fn in ENTRY.values():
        res, args = nat.SIGNATURES[fn]
        assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
        assert getattr(nat.lib, fn).argtypes is not None
    assert nat.ABI_VERSION == 11


def test_csharp_cpp_and_python_hosts():
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    for fn in ENTRY.values():
        m = re.search(r"public static extern int " + fn + r"\((.*?)\);", cs, re.S)
        assert m and len(m.group(1).split(",")) == 7
        assert re.match(r"IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+, IntPtr \w+,\s+ulong capacity$", m.group(1))
    cg = open(os.path.join(ROOT, "bindings", "csharp", "CastGather.cs")).read()
    assert all(fn + "(" in cg for fn in ENTRY.values()) and "unsafe" not in cg
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert all("void " + m + "(" in hpp for m in ("SphereCastAll", "CapsuleCastAll", "BoxCastAll"))
    assert "DataBuffer<lbvh_box_hit>& hits, size_t count" in hpp           # SortHitSegments takes box hits
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("sphere_cast_all", "capsule_cast_all", "box_cast_all", "cast_all"))
    assert "castall_main" in open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()


# ---- CPU: known answers of the reference --------------------------------------------------------------------------------

BIG = TB.BIG                                # one big triangle in z = 0 (vertices (0,0,0), (8,0,0), (0,8,0)) and a far dummy


def make(shape, origin, direction, t_max=INF, size=0.5):
    """one cast per row: a sphere of radius `size`, a capsule of that radius with the axis (0, 0, 2 * size), an AABB of that half extent"""
    o, d = np.atleast_2d(np.asarray(origin, dtype=F)), np.atleast_2d(np.asarray(direction, dtype=F))
    n = len(o)
    if shape == "sphere":
        c = np.zeros(n, dtype=SR.SPHERE_RAY)
        c["origin"], c["dir"], c["radius"], c["t_max"] = o, d, F(size), t_max
        return c
    if shape == "capsule":
        return CR.make_casts(o, d, F(size), np.tile(np.array([0, 0, 2 * size], dtype=F), (n, 1)), t_max)
    eye = np.eye(3, dtype=F) * F(size)
    return BR.make_casts(o, d, *(np.tile(eye[k], (n, 1)) for k in range(3)), t_max)


def inactive_forms(shape):
    o, d = [2, 2, 5], [0, 0, -1]
    nan, inf = np.nan, np.inf
    casts = np.concatenate([make(shape, o, d, t) for t in (0.0, -1.0, nan)] +
                           [make(shape, x, d) for x in ([nan, 2, 5], [2, nan, 5], [2, 2, nan])] +
                           [make(shape, o, x) for x in ([0, inf, -1], [nan, 0, -1], [0, 0, -inf], [0, 0, 0], [0, 0, -1e-30])])
    extra = []
    if shape != "box":
        for r in (0.0, -1.0, nan, inf):
            e = make(shape, o, d)
            e["radius"] = r
            extra.append(e)
    if shape == "capsule":
        e = make(shape, o, d)
        e["axis"][0, 1] = inf
        extra.append(e)
    if shape == "box":
        e = make(shape, o, d)
        e["az"] = e["ax"]                                                  # flat: det = 0
        extra.append(e)
        e = make(shape, o, d)
        e["ay"][0, 2] = nan
        extra.append(e)
    return np.concatenate([casts] + extra)


@pytest.mark.parametrize("shape", SHAPES)
def test_reference_known_answers(shape):
    a, b, c = BIG
    lo, hi = padded_boxes(a, b, c)
    # one triangle: dropped onto the face from z = 5 (the capsule's axis points up: its lower end touches); t = 4.5
    r = CA.reference(make(shape, [2, 2, 5], [0, 0, -1]), a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 1] and r.records["t"].tolist() == [4.5] and r.records["tri"].tolist() == [0]
    if shape == "box":
        assert r.records["axis"].tolist() == [0] and r.records["_zero"].tolist() == [0]
    else:
        assert r.records["u"].tolist() == [0.25] and r.records["v"].tolist() == [0.25]
    # t_max at the contact: no candidate (t < T is strict); just beyond: one
    assert CA.reference(make(shape, [2, 2, 5], [0, 0, -1], F(4.5)), a, b, c, lo, hi).offsets.tolist() == [0, 0]
    assert CA.reference(make(shape, [2, 2, 5], [0, 0, -1], np.nextafter(F(4.5), INF)), a, b, c, lo, hi).offsets.tolist() == [0, 1]
    # two coincident triangles: a tie, ordered by index
    a2, b2, c2 = (np.concatenate([x[:1], x[:1], x[1:]]) for x in (a, b, c))
    r = CA.reference(make(shape, [2, 2, 5], [0, 0, -1]), a2, b2, c2, *padded_boxes(a2, b2, c2))
    assert r.offsets.tolist() == [0, 2] and r.records["t"].tolist() == [4.5, 4.5] and r.records["tri"].tolist() == [0, 1]
    assert (rec_words(r.records)[0, [0, 2, 3]] == rec_words(r.records)[1, [0, 2, 3]]).all()
    # a start in overlap: +0 (the sign bit clear)
    r = CA.reference(make(shape, [2, 2, 0.25], [0, 0, -1]), a, b, c, lo, hi)
    assert r.offsets.tolist() == [0, 1] and words(r.records["t"]).tolist() == [0]
    if shape == "box":
        assert r.records["axis"].tolist() == [13]
    # every inactive form: an empty segment
    dead = inactive_forms(shape)
    assert not REF[shape].active(dead).any()
    r = CA.reference(dead, a, b, c, lo, hi)
    assert (r.offsets == 0).all() and len(r.records) == 0
    # a mix keeps the segments apart
    mix = np.concatenate([make(shape, [2, 2, 5], [0, 0, -1]), dead[:2], make(shape, [2, 2, 0.25], [0, 0, -1]), make(shape, [2, 2, 5], [0, 0, 1])])
    assert CA.reference(mix, a2, b2, c2, *padded_boxes(a2, b2, c2)).offsets.tolist() == [0, 2, 2, 2, 4, 4]


# ---- the parity sets -------------------------------------------------------------------------------------------------------

def scene_positions(name):
    return stacked_sheets() if name == "sheets" else TB.scene_positions(name)


def plough_casts(shape, count=48, seed=21):
    """Shapes sliding in the plane of grid_80x80 (z = 0, |x|, |y| <= 4, cells of 0.1): centres within the shape's radius or half
    height of the plane, directions in the plane, ways of 2 .. 7 units: a sweep touches every triangle of a band — hundreds.  A
    third have a t_max that ends the way early, a few start beyond the grid."""
    rng = np.random.default_rng(seed)
    size = rng.uniform(0.15, 0.4, count)
    start = np.stack([rng.uniform(-3.8, -3.0, count), rng.uniform(-3.5, 3.5, count), rng.uniform(-0.9, 0.9, count) * size], axis=1)
    angle = rng.uniform(-0.4, 0.4, count)
    d = np.stack([np.cos(angle), np.sin(angle), np.zeros(count)], axis=1) * rng.uniform(2.0, 7.0, count)[:, None]
    flip = rng.random(count) < 0.5
    start[flip, 0], d[flip, 0] = -start[flip, 0], -d[flip, 0]
    start[::11, 0] -= 20.0                                                 # beyond the grid: nothing in reach before t_max = 1
    t_max = np.where(np.arange(count) % 3 == 0, rng.uniform(0.2, 0.7, count), 1.0).astype(F)
    if shape == "sphere":
        c = np.zeros(count, dtype=SR.SPHERE_RAY)
        c["origin"], c["dir"], c["radius"], c["t_max"] = start, d, size, t_max
        return c
    if shape == "capsule":
        axis = rng.normal(size=(count, 3)) * size[:, None]
        return CR.make_casts(start.astype(F), d.astype(F), size.astype(F), axis.astype(F), t_max)
    ax, ay, az = TB.random_boxes(count, size, rng)
    return BR.make_casts(start.astype(F), d.astype(F), ax.astype(F), ay.astype(F), az.astype(F), t_max)


def parity_casts(shape, name, a, b, c):
    """the aimed casts of the shape's first-contact tests (their mix of sizes, ranges, starts in overlap and inactive forms) and, on
    the grid, the plough set in front"""
    casts = GEN[shape].aimed_casts(a, b, c, COUNT, np.random.default_rng(17 + len(a)))
    return np.concatenate([plough_casts(shape), casts]) if name == "grid_80x80" else casts


_CPU = {}


def cpu_case(shape, name):
    """(positions, boxes, casts, reference) with the Morton stage's boxes, once per shape and scene"""
    if (shape, name) not in _CPU:
        a, b, c = scene_positions(name)
        lo, hi = padded_boxes(a, b, c)
        casts = parity_casts(shape, name, a, b, c)
        _CPU[shape, name] = ((a, b, c), (lo, hi), casts, CA.reference(casts, a, b, c, lo, hi))
    return _CPU[shape, name]


def miss_of(shape):
    return REF[shape].MISS


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES)
def test_reference_least_of_every_segment_is_the_first_contact_reference(shape, name):
    (a, b, c), (lo, hi), casts, ref = cpu_case(shape, name)
    first = REF[shape].reference(casts, a, b, c, lo, hi)
    m = np.diff(ref.offsets.astype(np.int64))
    assert (first.flags == (m >= 1)).all()
    least = CA.least(ref.offsets, ref.records, miss_of(shape))
    bad = np.nonzero((rec_words(least) != rec_words(first.records)).any(axis=1))[0]
    assert len(bad) == 0, (shape, name, bad[:10], least[bad[:3]], first.records[bad[:3]])
    assert (m[~REF[shape].active(casts)] == 0).all()
    segment = np.repeat(np.arange(len(m)), m)                              # canonical() undoes any order inside the segments
    backwards = ref.records[np.lexsort((-np.arange(len(segment)), segment))]
    assert (rec_words(CA.canonical(ref.offsets, backwards)) == rec_words(ref.records)).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_parity_sets_exercise_what_they_must(shape):
    longest = empty = total = inactive = at_start = cut = 0
    for name in SCENES:
        (a, b, c), (lo, hi), casts, ref = cpu_case(shape, name)
        m = np.diff(ref.offsets.astype(np.int64))
        act = REF[shape].active(casts)
        longest = max(longest, int(m.max()))
        empty += int((m == 0).sum())
        total += len(m)
        inactive += int((~act).sum())
        at_start += int((words(ref.records["t"]) == 0).sum())
        # a finite t_max that cuts a segment: the same cast with an open range has more
        finite = np.nonzero(act & np.isfinite(casts["t_max"]) & (m > 0))[0][:60]
        opened = casts[finite].copy()
        opened["t_max"] = INF
        cut += int((np.diff(CA.reference(opened, a, b, c, lo, hi).offsets.astype(np.int64)) > m[finite]).sum())
        print(f"{shape} {name}: {len(m)} casts, {int(m.sum())} records, longest {int(m.max())}, empty {int((m == 0).sum())}, "
              f"inactive {int((~act).sum())}")
    assert longest >= 257, longest                                        # crosses the segment sort's one-wave limit
    assert empty >= 0.1 * total and inactive > 50 and at_start > 20 and cut > 10, (empty, total, inactive, at_start, cut)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_plough_set_has_long_segments(shape):
    (a, b, c), (lo, hi), casts, ref = cpu_case(shape, "grid_80x80")
    m = np.diff(ref.offsets.astype(np.int64))[:48]
    print(f"{shape}: plough segments {sorted(m.tolist())[-5:]} longest, {int((m == 0).sum())} empty")
    assert (m >= 257).sum() >= 5 and (m == 0).sum() >= 3


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Sweeps:
    """device buffers for one cast set: the list calls and the two single-answer calls"""

    def __init__(self, ctx, drawer, shape, casts):
        self.ctx, self.drawer, self.shape, self.n = ctx, drawer, shape, len(casts)
        self.casts = H().DataBuffer(ctx, max(self.n, 1), ray_layout(shape))
        self.casts.local[: self.n] = casts
        self.casts.sync()
        self.offsets = H().DataBuffer(ctx, self.n + 1, np.uint64)
        self.hits = H().DataBuffer(ctx, max(self.n, 1), hit_layout(shape))
        self.flags = H().DataBuffer(ctx, max(self.n, 1), np.uint32)
        self.all = getattr(drawer, shape + "_cast_all")
        self.fn = getattr(N().lib, ENTRY[shape])

    def count_only(self):
        self.offsets.fill_u32(0xDEADBEEF)
        self.all(self.casts, self.offsets)
        return self.offsets.get_data().copy()

    def gather(self, device_sort=False):
        """count only -> a buffer of exactly M records -> the full form: (offsets, the M records as the walk or the sort left them)"""
        first = self.count_only()
        total = int(first[-1])
        out = H().DataBuffer(self.ctx, max(total, 1), hit_layout(self.shape))
        out.fill_u32(NAN_WORD)
        self.offsets.fill_u32(0xDEADBEEF)
        self.all(self.casts, self.offsets, out)
        if device_sort:
            H().sort_hit_segments(self.ctx, self.offsets, out)
        off, rec = self.offsets.get_data().copy(), out.get_data()[:total].copy()
        out.dispose()
        assert (off == first).all()
        return off, rec

    def first(self):
        self.hits.fill_u32(NAN_WORD)
        getattr(self.drawer, self.shape + "_cast")(self.casts, self.hits)
        return self.hits.get_data()[: self.n].copy()

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        getattr(self.drawer, self.shape + "_cast_any")(self.casts, self.flags)
        return self.flags.get_data()[: self.n].copy()

    def dispose(self):
        for b in (self.casts, self.offsets, self.hits, self.flags):
            b.dispose()


def assert_equal(off, rec, ref, what="", canonical=True):
    """offsets equal; the canonical segments equal word for word"""
    assert off.dtype == np.uint64 and (off == ref.offsets).all(), (what, np.nonzero(off != ref.offsets)[0][:10])
    assert len(rec) == int(ref.offsets[-1])
    got = CA.canonical(off, rec) if canonical else rec
    bad = np.nonzero((rec_words(got) != rec_words(ref.records)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], ref.records[bad[:3]])


_SCENES, _CASES = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cached_scenes():
    """the parity scenes stay on the device for the tests of this file only (tests/test_box_cast.py says why)"""
    yield
    for entry in _SCENES.values():
        entry[2].on_destroy()
    _SCENES.clear()
    _CASES.clear()


def parity_case(ctx, shape, name):
    """(positions, casts, the reference from the library's boxes, drawer): one drawer per scene, one reference per shape and scene;
    one context keeps one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _SCENES:
        a, b, c = scene_positions(name)
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        _SCENES[name] = ((a, b, c), library_boxes(d), d)
    (a, b, c), (lo, hi), d = _SCENES[name]
    if (shape, name) not in _CASES:
        casts = parity_casts(shape, name, a, b, c)
        _CASES[shape, name] = (casts, CA.reference(casts, a, b, c, lo, hi))
    d.build_fast_scene()
    return (a, b, c), _CASES[shape, name][0], _CASES[shape, name][1], d


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES)
def test_1_segments_equal_the_brute_force_word_for_word(ctx, shape, name):
    _, casts, ref, d = parity_case(ctx, shape, name)
    q = Sweeps(ctx, d, shape, casts)
    off, rec = q.gather()
    q.dispose()
    m = np.diff(ref.offsets.astype(np.int64))
    print(f"{shape} {name}: {len(casts)} casts, {int(m.sum())} records, longest {int(m.max())}, {int((m == 0).sum())} empty")
    assert_equal(off, rec, ref, (shape, name))
    # the convenience call: the same list, ordered on the host and on the device
    buf = H().DataBuffer(ctx, len(casts), ray_layout(shape))
    buf.local[:] = casts
    buf.sync()
    for kw in ({"sort": True}, {"device_sort": True}):
        off2, rec2 = d.cast_all(buf, **kw)
        assert rec2.dtype == hit_layout(shape)
        assert_equal(off2, rec2, ref, (shape, name, kw), canonical=False)
    buf.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES)
def test_2_the_device_segment_sort_gives_the_canonical_order(ctx, shape, name):
    _, casts, ref, d = parity_case(ctx, shape, name)
    q = Sweeps(ctx, d, shape, casts)
    off, rec = q.gather(device_sort=True)
    q.dispose()
    assert_equal(off, rec, ref, (shape, name), canonical=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES)
def test_3_identities_with_the_shipped_calls(ctx, shape, name):
    _, casts, ref, d = parity_case(ctx, shape, name)
    q = Sweeps(ctx, d, shape, casts)
    off, rec = q.gather()
    first, flags = q.first(), q.any()
    q.dispose()
    m = np.diff(off.astype(np.int64))
    assert (flags == (m >= 1)).all()
    least = CA.least(off, CA.canonical(off, rec), miss_of(shape))
    bad = np.nonzero((rec_words(least) != rec_words(first)).any(axis=1))[0]
    assert len(bad) == 0, (shape, name, bad[:10], least[bad[:3]], first[bad[:3]])
    if shape == "sphere":
        return
    # every triangle the overlap query lists for the shape where it starts is in the segment with t = +0
    act = np.nonzero(REF[shape].active(casts))[0]
    if shape == "capsule":
        shapes = H().capsule_shapes(casts["origin"][act], casts["axis"][act], casts["radius"][act])
    else:
        shapes = np.zeros(len(act), dtype=L().OBB)
        for k in ("centre", "ax", "ay", "az"):
            shapes[k] = casts[k][act]
    buf = H().DataBuffer(ctx, len(shapes), shapes.dtype)
    buf.local[:] = shapes
    buf.sync()
    t_off, tris = d.touching(buf, device_sort=True)
    buf.dispose()
    canon = CA.canonical(off, rec)
    missing = extra = listed = 0
    for j, qi in enumerate(act):
        seg = canon[int(off[qi]):int(off[qi + 1])]
        zero = set(seg["tri"][words(seg["t"]) == 0].tolist())
        touched = set(tris[int(t_off[j]):int(t_off[j + 1])].tolist())
        listed += len(touched)
        missing += len(touched - zero)
        extra += len(zero - touched)
    print(f"{shape} {name}: {listed} triangles touched at the start; missing from the t = +0 records {missing}, t = +0 records not listed {extra}")
    assert listed > 50 and missing == 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_4_capacity_is_never_overrun_and_fitting_segments_are_complete(ctx, shape):
    _, casts, ref, d = parity_case(ctx, shape, "grid_80x80")
    q = Sweeps(ctx, d, shape, casts)
    total = int(ref.offsets[-1])
    big = H().DataBuffer(ctx, total + 64, hit_layout(shape))
    h, s = ctx.handle, d.container.scene()
    ref_off = ref.offsets.astype(np.int64)
    inside = int(ref_off[np.argmax(np.diff(ref_off))] + 100)                  # in the middle of the longest segment
    for capacity in (total, total - 1, inside, 1):
        big.fill_u32(NAN_WORD)
        q.offsets.fill_u32(0xDEADBEEF)
        N().check(h, q.fn(h, q.casts.device, q.n, C.byref(s), q.offsets.device, big.device, capacity))
        off, rec = q.offsets.get_data().copy(), big.get_data().copy()
        assert (off == ref.offsets).all(), capacity                    # the offsets do not depend on the capacity
        assert (words(rec[capacity:]) == NAN_WORD).all(), capacity     # no word at or beyond the capacity changed
        fits = np.nonzero(ref_off[1:] <= capacity)[0]                  # offsets rise: the fitting segments are a prefix
        end = int(ref_off[fits[-1] + 1]) if len(fits) else 0
        assert len(fits) == 0 or (fits == np.arange(len(fits))).all()
        got = CA.canonical(off[: len(fits) + 1], rec[:end])
        assert (rec_words(got) == rec_words(ref.records[:end])).all(), capacity
        if capacity == total:
            assert len(fits) == q.n and end == total
        if capacity == inside:
            assert 0 < len(fits) < q.n and end < capacity
    big.fill_u32(NAN_WORD)                                             # capacity == 0 with d_hits == NULL: the same offsets
    assert (q.count_only() == ref.offsets).all()
    assert (words(big.get_data()) == NAN_WORD).all()
    big.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_5_lane_refill_reloads_the_write_position(ctx, shape):
    _, casts, ref, d = parity_case(ctx, shape, "sheets")
    casts = np.resize(casts, 1500)                                     # the set, repeated up to 1 500
    ref = CA.reference(casts, *_SCENES["sheets"][0], *_SCENES["sheets"][1])
    q = Sweeps(ctx, d, shape, casts)
    h, lib = ctx.handle, N().lib
    try:
        for cap in (1, 2, 3, 7):                                       # 1 500 casts on one wave: about 23 refills per lane
            N().check(h, lib.lbvh_debug_ray_waves(h, cap))
            assert_equal(*q.gather(), ref, (shape, f"waves <= {cap}"))
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal(*q.gather(), ref, (shape, "cap restored"))
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_6_output_does_not_depend_on_the_stack_split(ctx, shape):
    _, casts, ref, d = parity_case(ctx, shape, "cfg1_4096")
    q = Sweeps(ctx, d, shape, casts)
    h, lib = ctx.handle, N().lib
    canon = []
    try:
        for split in (1, 16):                                          # 1: nearly every waiting sibling in the device-memory part
            N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
            off, rec = q.gather()
            assert_equal(off, rec, ref, (shape, f"split {split}"))
            canon.append((off, CA.canonical(off, rec)))
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert (canon[0][0] == canon[1][0]).all() and (rec_words(canon[0][1]) == rec_words(canon[1][1])).all()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_7_edges(ctx, shape):
    (a, b, c), casts, ref, d = parity_case(ctx, shape, "cfg1_4096")
    lo, hi = _SCENES["cfg1_4096"][1]
    live = np.nonzero(np.diff(ref.offsets.astype(np.int64)) > 0)[0]

    def check(set_, what):
        q = Sweeps(ctx, d, shape, set_)
        assert_equal(*q.gather(), CA.reference(set_, a, b, c, lo, hi), (shape, what))
        q.dispose()

    for count in (1, 63, 64, 65):
        check(casts[live[:count]].copy(), f"a count of {count}")
    opened = casts[live[:100]].copy()
    opened["t_max"] = INF
    check(opened, "t_max = +inf")
    # a shape far beyond the scene: it starts in overlap with every triangle
    ext = TB.extent_of(a, b, c)
    far = make(shape, np.tile(np.concatenate([a, b, c]).mean(axis=0), (3, 1)), np.eye(3), size=3.0 * ext)
    q = Sweeps(ctx, d, shape, far)
    off, rec = q.gather()
    assert int(off[-1]) > 2 * len(a) and (words(rec["t"]) == 0).all()
    assert_equal(off, rec, CA.reference(far, a, b, c, lo, hi), (shape, "beyond the scene"))
    # count == 0 touches nothing, d_offsets[0] included
    out = H().DataBuffer(ctx, 8, hit_layout(shape))
    out.fill_u32(NAN_WORD)
    q.offsets.fill_u32(0xDEADBEEF)
    s = d.container.scene()
    assert q.fn(ctx.handle, q.casts.device, 0, C.byref(s), q.offsets.device, out.device, 8) == 0
    assert (words(q.offsets.get_data()) == 0xDEADBEEF).all() and (words(out.get_data()) == NAN_WORD).all()
    # all casts inactive: all-zero offsets, no record written
    dead = inactive_forms(shape)
    qd = Sweeps(ctx, d, shape, dead)
    qd.offsets.fill_u32(0xDEADBEEF)
    qd.all(qd.casts, qd.offsets, out)
    assert (qd.offsets.get_data() == 0).all() and (words(out.get_data()) == NAN_WORD).all()
    for x in (q, qd, out):
        x.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_8_errors_scratch_failure_and_the_stack_limit(ctx, shape):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        casts = GEN[shape].aimed_casts(a, b, c, 600, np.random.default_rng(2))
        ref = CA.reference(casts, a, b, c, *library_boxes(d))
        total = int(ref.offsets[-1])
        assert total > 300
        q = Sweeps(c2, d, shape, casts)
        out = H().DataBuffer(c2, total + 16, hit_layout(shape))
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n, fn, who = len(casts), q.fn, ENTRY[shape].encode() + b": invalid argument: "

        def poison():
            out.fill_u32(NAN_WORD)
            q.offsets.fill_u32(0xDEADBEEF)

        def untouched():
            return (words(out.get_data()) == NAN_WORD).all() and (words(q.offsets.get_data()) == 0xDEADBEEF).all()

        def full():
            poison()
            assert fn(h, q.casts.device, n, C.byref(s), q.offsets.device, out.device, total) == 0
            return q.offsets.get_data().copy(), out.get_data()[:total].copy()

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
        assert msg.startswith(ENTRY[shape].encode() + b": ") and b"stale" in msg, msg
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
@pytest.mark.parametrize("shape", SHAPES)
def test_9_statistics_the_full_form_is_two_equal_walks(ctx, shape):
    _, casts, ref, d = parity_case(ctx, shape, "cfg1_4096")
    q = Sweeps(ctx, d, shape, casts)
    total = int(ref.offsets[-1])
    out = H().DataBuffer(ctx, total, hit_layout(shape))
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    h, lib = ctx.handle, N().lib

    def counted(call):
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            call()
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        s = stats.get_data()[0]
        return int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"])

    try:
        one = counted(lambda: q.all(q.casts, q.offsets))
        two = counted(lambda: q.all(q.casts, q.offsets, out))
        assert_equal(q.offsets.get_data().copy(), out.get_data().copy(), ref, (shape, "the counting kernels"))
    finally:
        stats.dispose()
        out.dispose()
        q.dispose()
    print(f"{shape}: casts, node lines, triangle lines: count only {one}, full {two}")
    assert one[0] == int(REF[shape].active(casts).sum()) and one[1] >= one[0] and one[2] >= total
    assert two == tuple(2 * x for x in one)


@pytest.mark.gpu
def test_10_path_tracer_frame_undisturbed_by_a_call_between_bounces(ctx):
    """the calls drop the live-path list: the next lbvh_path_bounce scans again and the frame is the one without them"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    count = 160 * 96
    st0 = pt.states.get_data()[:count].copy()
    a, b, c = positions(tris)
    sets = []
    for shape in SHAPES:                                                       # 4x the frame together: the scratch grows in mid-frame
        casts = GEN[shape].aimed_casts(a, b, c, 2 * count, np.random.default_rng(12))
        casts["t_max"] = np.minimum(casts["t_max"], F(0.6))
        sets.append(Sweeps(ctx, pt.drawer, shape, casts))
    cam = N().Camera.from_dict(cam_d)
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib
    turn = [0]

    def call():
        q = sets[turn[0] % 3]
        turn[0] += 1
        q.all(q.casts, q.offsets)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    call()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        call()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    call()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    for q in sets:
        assert 0 < int(q.offsets.get_data()[q.n])
        q.dispose()
    pt.drawer.on_destroy()


def driver_casts(shape, lo, hi, count, seed, t_max):
    if shape == "sphere":
        origin, direction = driver_rays(lo, hi, count, seed)
        c = np.zeros(count, dtype=SR.SPHERE_RAY)
        c["origin"], c["dir"], c["radius"], c["t_max"] = origin, direction, F(1.5), F(t_max)
        return c
    if shape == "capsule":
        c = CR.driver_casts(lo, hi, count, seed)
        c["t_max"] = F(t_max)
        return c
    return BR.driver_casts(lo, hi, count, seed, 1.5, t_max)


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), (7, 0.75)])
@pytest.mark.parametrize("shape", SHAPES)
def test_11_cpp_host_driver_castall_matches_the_python_host(ctx, shape, args):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 3000
    res = json.loads(subprocess.run([exe, "castall", shape, str(count)] + [str(x) for x in args], check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(4096)
    seed, t_max = args if args else (3, 2.0)
    casts = driver_casts(shape, lo, hi, count, seed, t_max)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Sweeps(ctx, d, shape, casts)
    off, rec = q.gather(device_sort=True)
    flags = q.any()
    q.dispose()
    d.on_destroy()
    m = np.diff(off.astype(np.int64))
    total = int(off[-1])
    assert res["shape"] == shape and res["triangles"] == len(tris) and res["casts"] == count and F(res["t_max"]) == F(t_max)
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
