"""lbvh_sort_record_segments: every segment of a CSR list of 32-byte records put into key order on the device, in place, in one of
three orders (ascending by (K(word 0), word 1), descending by (D(word 0), word 1), ascending by word 3).  The expectation is
tests/record_sort_reference.py: segsort_reference's K and fitting segments, D, and np.lexsort; everything outside the fitting
segments unchanged.  Every GPU comparison is word for word on uint32 views, no tolerance, no case left out.  The sort is not stable,
so the synthetic lists keep the keys inside a segment distinct (asserted on the CPU first).  Tier borders of the implementation: 256
records (wave tier / block tier) and 1 024 (one LDS chunk / merges on device memory); the first GPU test probes the neighbours of
every power of two up to 2^15 and two ragged lengths beyond two chunks.

The producers run on the 80 x 80 grid with these query counts (the generators of the producers' own tests, at a smaller count):
CAPSULES = BOXES = TRI_QUERIES = PROX_QUERIES = 300 shapes or triangles, PLANES = 160 random planes + 20 that miss + 20 across a
corner."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import box_contact_reference as BK
import contact_reference as CK
import plane_section_reference as PS
import record_sort_reference as R
import segsort_reference as S
import triangle_proximity_reference as X
import triangle_segment_reference as TS
from query_support import H, L, N, padded_boxes, positions, splitmix, words
from test_segment_sort import offsets_of, T_SET
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
POISON = 0x7FC00000
ORDERS = [R.ASCENDING, R.DESCENDING, R.BY_TRI]
CAPSULES = BOXES = TRI_QUERIES = PROX_QUERIES = 300
PLANES = (160, 20, 20)                       # random, missing the mesh, across a corner


def bits(*w):
    return np.array(w, dtype=np.uint32).view(F)


# ---- CPU: D ---------------------------------------------------------------------------------------------------------------------

def test_d_known_answers():
    d = lambda x: int(R.D(np.array([x], dtype=F))[0])
    inf = F(np.inf)
    denorm = bits(0x00000001)[0]
    assert d(F(-0.0)) == d(F(0.0)) == 0x7FFFFFFF
    chain = [inf, F(1), denorm, F(0), -denorm, F(-1), -inf]                 # greatest first
    keys = [d(x) for x in chain]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    nans = R.D(bits(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF))
    assert (nans == 0xFFFFFFFF).all()                                       # every NaN one class, still last
    assert d(inf) == 0x007FFFFF and d(-inf) == 0xFF800000 < 0xFFFFFFFF      # ~K <= 0xFF800000: below the NaNs


def test_d_reverses_k_on_random_pairs():
    rng = np.random.default_rng(12)
    w = rng.integers(0, 1 << 32, (10000, 2), dtype=np.uint64).astype(np.uint32)
    x, y = w[:, 0].view(F), w[:, 1].view(F)
    ok = ~(np.isnan(x) | np.isnan(y))
    assert ok.sum() > 9000
    kx, ky, dx, dy = S.K(x), S.K(y), R.D(x), R.D(y)
    assert ((kx < ky) == (dx > dy))[ok].all() and ((kx == ky) == (dx == dy))[ok].all()
    with np.errstate(invalid="ignore"):
        assert ((x > y) == (dx < dy))[ok].all()
    assert (dx[np.isnan(x)] == 0xFFFFFFFF).all() and (dx[~np.isnan(x)] <= 0xFF800000).all()
    assert (kx[~np.isnan(x)] != 0).all()


# ---- CPU: the surface in every host -------------------------------------------------------------------------------------------------

def test_header_declares_the_call_and_keeps_the_five_old_sentences():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"lbvh_status lbvh_sort_record_segments\(lbvh_context\* ctx, const uint64_t\* d_offsets, size_t count,\s*"
                     r"void\* d_records, uint64_t capacity, uint32_t order\);", h)
    for name, value in (("ASCENDING", 0), ("DESCENDING", 1), ("BY_TRI", 2)):
        assert re.search(r"#define LBVH_SORT_RECORDS_%s\s+%du\b" % (name, value), h)
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                   # purely additive
    doc = h[h.index("The same pass for the CSR lists of 32-byte records"):h.index("#define LBVH_SORT_RECORDS_ASCENDING")]
    for must in ("THE SORT IS NOT STABLE", "d_offsets is never written", "order > 2", "not 16-byte aligned", "NO context scratch",
                 "live-path list kept", "0xFFFFFFFF for a NaN", "NO DEPTH OF THE SEGMENT IS A NaN", "lbvh_triangle_closest_point's",
                 "strictly ascending"):
        assert must in " ".join(doc.replace("\n *", " ").split()), must
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_sort_record_segments" in bounce and "keep the live-path list" in bounce
    blocks = (("Capsule contacts: HOW DEEP", "lbvh_status lbvh_capsule_contacts(", "lbvh_sort_hit_segments is for 16-byte records"),
              ("Box contacts: HOW DEEP", "lbvh_status lbvh_obb_contacts(", "a device-side sort of 32-byte segments"),
              ("Triangle proximity: EVERY scene triangle", "lbvh_status lbvh_triangle_gather_within_distance(", "a device-side sort of 32-byte records"),
              ("Triangle intersection segments: WHERE", "lbvh_status lbvh_triangle_intersection_segments(", "a device-side sort of 32-byte record segments"),
              ("Plane sections: WHERE does a plane cut the mesh", "#define LBVH_PLANE_SECTIONS_MAX_COUNT", "a device-side sort of 32-byte segments"))
    for start, end, old in blocks:
        text = h[h.index(start):h.index(end)]
        assert old in text, old
        assert "lbvh_sort_record_segments" in text[text.index(old):], start  # the pointer follows the old sentence


def test_the_surface_in_every_host():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_sort_record_segments"]
    assert res is C.c_int32 and len(args) == 6 and args[2] is C.c_size_t and args[4] is C.c_uint64 and args[5] is C.c_uint32
    assert nat.lib.lbvh_sort_record_segments.argtypes is not None and nat.ABI_VERSION == 11
    assert (nat.SORT_RECORDS_ASCENDING, nat.SORT_RECORDS_DESCENDING, nat.SORT_RECORDS_BY_TRI) == (0, 1, 2)
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public static extern int lbvh_sort_record_segments\((.*?)\);", cs, re.S)
    assert m and len(m.group(1).split(",")) == 6
    assert re.match(r"IntPtr ctx, IntPtr dOffsets, UIntPtr count, IntPtr dRecords, ulong capacity,\s*uint order$", m.group(1))
    wrapper = open(os.path.join(ROOT, "bindings", "csharp", "SegmentSort.cs")).read()
    assert "lbvh_sort_record_segments" in wrapper and "public static void SortRecords(" in wrapper and "unsafe" not in wrapper
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void SortRecordSegments(" in hpp and "lbvh_sort_record_segments(" in hpp
    host = H()
    assert list(inspect.signature(host.sort_record_segments).parameters) == ["ctx", "offsets", "records", "order", "count"]
    for name in ("contacts", "proximity_pairs", "intersection_segments", "cross_sections"):
        p = inspect.signature(getattr(host.RaytracingMeshDrawer, name)).parameters
        assert "device_sort" in p and p["device_sort"].default is False, name
    orders = host._record_orders()
    lay = L()
    assert orders == {lay.TRI_CLOSEST: 0, lay.CONTACT: 1, lay.BOX_CONTACT: 1, lay.TRI_SEGMENT: 2, lay.PLANE_SEGMENT: 2}
    driver = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"sortedrecords", sortedrecords_main}' in driver


# ---- the producers' query sets and brute-force lists on the 80 x 80 grid ---------------------------------------------------------

def grid():
    tris = scenes.grid_scene()
    assert len(tris) == 12800
    return tris


def capsule_shapes(a, b, c):
    from test_shape_contacts import contact_shapes
    return contact_shapes(a, b, c, count=CAPSULES)


def box_shapes(a, b, c):
    from test_box_contacts import contact_shapes
    return contact_shapes(a, b, c, count=BOXES)


def prox_queries(a, b, c):
    from test_shape_overlaps import extent_of
    from test_triangle_closest import parity_queries
    q, r = parity_queries(a, b, c, count=PROX_QUERIES)
    rng = np.random.default_rng(41)
    fill = (extent_of(a, b, c) * rng.uniform(0.005, 0.05, len(q))).astype(F)
    r = np.where(np.isinf(r), fill, r).astype(F)
    q["max_dist2"] = r * r
    return q


def tri_queries(a, b, c):
    from test_triangle_segments import parity_queries
    return parity_queries(a, b, c, count=TRI_QUERIES)


def planes_of(a, b, c):
    """PLANES[0] random planes through the mesh, PLANES[1] far above it, PLANES[2] across the corner at the least x and y"""
    from test_plane_sections import random_planes
    rnd = random_planes(a, b, c, PLANES[0])
    pts = np.concatenate([a, b, c])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(44)
    up = np.tile(np.array([0.0, 0.0, 1.0]), (PLANES[1], 1))
    miss = H().planes(up, np.stack([np.zeros(PLANES[1]), np.zeros(PLANES[1]), hi[2] + ext * rng.uniform(1.0, 2.0, PLANES[1])], axis=1))
    cell = ext / 80.0
    step = cell * rng.uniform(0.2, 3.0, PLANES[2])
    corner = H().planes(np.tile(np.array([1.0, 1.0, 0.3]), (PLANES[2], 1)), np.stack([lo[0] + step, lo[1] + step, np.full(PLANES[2], lo[2])], axis=1))
    return np.concatenate([rnd, miss, corner])


# kind -> (query generator, brute force, its records field, query layout, record layout, the order the dtype names)
KINDS = {
    "contacts": (capsule_shapes, CK.reference, "contacts", "CAPSULE", "CONTACT", R.DESCENDING),
    "boxcontacts": (box_shapes, BK.reference, "contacts", "OBB", "BOX_CONTACT", R.DESCENDING),
    "triprox": (prox_queries, X.reference, "records", "TRI_DISTANCE_QUERY", "TRI_CLOSEST", R.ASCENDING),
    "trisegs": (tri_queries, TS.reference, "records", "TRI_QUERY", "TRI_SEGMENT", R.BY_TRI),
    "sections": (planes_of, PS.reference, "records", "PLANE", "PLANE_SEGMENT", R.BY_TRI),
}
_CASES = {}


def producer_case(kind, boxes=None):
    """(queries, offsets, records of the brute force, the same with every segment in the order of `kind`), once per kind and box set;
    asserts that the set has some empty, some short (1 .. 16 records: several of them share a wave's sub-run) and some multi-record
    (>= 2: something to sort) segments — on the flat grid a shape that touches the mesh at all touches several triangles"""
    key = (kind, boxes is not None)
    if key not in _CASES:
        a, b, c = positions(grid())
        lo, hi = padded_boxes(a, b, c) if boxes is None else boxes
        make, reference, field, _, _, order = KINDS[kind]
        q = make(a, b, c)
        ref = reference(q, a, b, c, lo, hi)
        off, rec = ref.offsets, getattr(ref, field)
        m = np.diff(off.astype(np.int64))
        assert len(rec) == int(off[-1]) and (m == 0).sum() >= 5 and ((m >= 1) & (m <= 16)).sum() >= 5 and (m >= 2).sum() >= 5, (kind, np.bincount(m)[:8])
        want = R.reference_records(off, rec, len(rec), order)
        _CASES[key] = (q, off, rec, want)
    return _CASES[key]


def python_sorted(off, rec, order):
    """an independent restatement of the three orders with Python's sorted() on fp32 values (no NaN among them)"""
    w = R.as_words(rec)
    out = w.copy()
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        value = w[lo:hi, 0].copy().view(F).astype(np.float64)
        assert not np.isnan(value).any()
        if order == R.BY_TRI:
            rank = sorted(range(hi - lo), key=lambda i: int(w[lo + i, 3]))
        else:
            sign = 1.0 if order == R.ASCENDING else -1.0
            rank = sorted(range(hi - lo), key=lambda i: (sign * value[i] + 0.0, int(w[lo + i, 1])))
        out[lo:hi] = w[lo:hi][rank]
    return out


@pytest.mark.parametrize("kind", ["contacts", "triprox", "sections"])
def test_reference_reproduces_the_sorted_brute_force_from_a_shuffled_input(kind):
    q, off, rec, want = producer_case(kind)
    order = KINDS[kind][5]
    rng = np.random.default_rng(6)
    shuffled = R.as_words(rec).copy()
    for k in range(len(off) - 1):
        lo, hi = int(off[k]), int(off[k + 1])
        shuffled[lo:hi] = shuffled[lo:hi][rng.permutation(hi - lo)]
    got = R.reference_records(off, shuffled, len(rec), order)
    assert (got == want).all() and (got == python_sorted(off, rec, order)).all()
    m = np.diff(off.astype(np.int64))
    capacity = len(rec) - 1                                                 # what does not fit is unchanged
    own = np.repeat(S.fitting(off, capacity), m)
    cut = R.reference_records(off, shuffled, capacity, order)
    assert not own.all() and (cut[~own] == shuffled[~own]).all() and (cut[own] == want[own]).all()
    first = want[off[:-1][m > 0].astype(np.int64)]
    if kind == "contacts":                                                  # the first record of a segment is the brute force's deepest
        assert (first == R.as_words(CK.deepest_of(off, rec))[m > 0]).all()
    if kind == "sections":
        assert (got == R.as_words(PS.sort_segments(off, rec))).all()
    if kind == "triprox":
        assert (got[:, [0, 1]] == R.as_words(rec[np.lexsort((rec["tri"], rec["dist2"], np.repeat(np.arange(len(m)), m)))])[:, [0, 1]]).all()


# ---- synthetic lists --------------------------------------------------------------------------------------------------------------

def random_records(total, rng):
    """(total, 8) words: word 0 from T_SET (many repeats), words 1 and 3 a permutation each (every key distinct, in every order),
    the other words a fingerprint of the record drawn at random"""
    w = rng.integers(0, 1 << 32, (total, 8), dtype=np.uint64).astype(np.uint32)
    w[:, 0] = T_SET[rng.integers(0, len(T_SET), total)].view(np.uint32)
    w[:, 1] = rng.permutation(total).astype(np.uint32)
    w[:, 3] = rng.permutation(total).astype(np.uint32)
    return w


def assert_distinct_keys(off, w):
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off.astype(np.int64)))
    for order in ORDERS:
        high, low = R.key_words(w[: len(seg)], order)
        rows = np.stack([seg.astype(np.uint64), high.astype(np.uint64), low.astype(np.uint64)], axis=1)
        assert len(np.unique(rows, axis=0)) == len(rows), order
    rows = w[:, [2, 4, 5, 6, 7]]
    assert len(np.unique(rows, axis=0)) == len(rows)                        # the fingerprints tell the records apart


_LISTS = {}


def every_length_class():
    """(offsets, words): the lengths 0 .. 3, 2^k - 1, 2^k, 2^k + 1 for k = 2 .. 15, and 2 500 and 7 001 (ragged, beyond two chunks of
    1 024: merge steps on device memory with a partner past the end), in an order shuffled by a fixed seed, with runs of 0, 1 and 200
    empty segments between them"""
    if "all" not in _LISTS:
        rng = np.random.default_rng(1)
        lengths = [0, 1, 2, 3] + [(1 << k) + d for k in range(2, 16) for d in (-1, 0, 1)] + [2500, 7001]
        lengths = [lengths[i] for i in rng.permutation(len(lengths))]
        full = []
        for i, n in enumerate(lengths):
            full += [n] + [0] * (0, 1, 200)[i % 3]
        off = offsets_of(full)
        assert max(full) == (1 << 15) + 1 and 200000 < int(off[-1]) < 220000
        w = random_records(int(off[-1]), rng)
        assert_distinct_keys(off, w)
        _LISTS["all"] = (off, w)
    return _LISTS["all"]


def device_sort(ctx, off, w, order, capacity=None, count=None, size=None, offsets_size=None):
    """uploads, calls the library, downloads: -> ((size, 8) words after, offsets after).  `size`: the buffer's length in records
    (the rest is poison); `capacity` defaults to len(w), `count` to len(off) - 1"""
    size = len(w) if size is None else size
    ob = H().DataBuffer(ctx, len(off), np.uint64)
    db = H().DataBuffer(ctx, max(size, 1), L().CONTACT)
    try:
        ob.local[:] = off
        ob.sync()
        db.local.view(np.uint32)[:] = POISON
        db.local.view(np.uint32).reshape(-1, 8)[: len(w)] = w
        db.sync()
        N().check(ctx.handle, N().lib.lbvh_sort_record_segments(ctx.handle, ob.device, len(off) - 1 if count is None else count, db.device,
                                                                len(w) if capacity is None else capacity, order))
        return R.as_words(db.get_data())[:size].copy(), ob.get_data().copy()
    finally:
        ob.dispose()
        db.dispose()


def assert_words(got, want, what=""):
    got, want = R.as_words(got), R.as_words(want)
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], want[bad[:3]])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_1_every_length_class(ctx, order):
    off, w = every_length_class()
    want = R.reference_records(off, w, len(w), order)
    got, off_after = device_sort(ctx, off, w, order)
    assert (off_after == off).all()
    assert_words(got, want, order)


def layouts_of_a_wave():
    """{name: lengths}: the layouts of the 64 queries of a wave that the sub-run cutting meets, and two counts that are multiples of
    neither 64 nor 1 024"""
    rng = np.random.default_rng(2)
    return {
        "64 of 4": [4] * 64,
        "one of 256 among empties": [0] * 20 + [256] + [0] * 43,
        "255 and 2": [255, 2] * 32,
        "count 100": rng.integers(0, 9, 100).tolist(),
        "count 1500": rng.integers(0, 7, 1499).tolist() + [5],
    }


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_2_layouts_of_the_64_queries_of_a_wave(ctx, order):
    rng = np.random.default_rng(3)
    for name, lengths in layouts_of_a_wave().items():
        off = offsets_of(lengths)
        w = random_records(int(off[-1]), rng)
        assert_distinct_keys(off, w)
        got, _ = device_sort(ctx, off, w, order)
        assert_words(got, R.reference_records(off, w, len(w), order), (name, order))
    lengths = layouts_of_a_wave()["count 1500"]                             # a count below the list's: the rest is not touched
    off = offsets_of(lengths)
    w = random_records(int(off[-1]), rng)
    for count in (1, 63, 65, 1025):
        got, _ = device_sort(ctx, off, w, order, count=count)
        assert_words(got, R.reference_records(off[: count + 1], w, len(w), order), (count, order))
        assert_words(got[int(off[count]):], w[int(off[count]):], "behind the last segment")


SPECIAL = bits(0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x7F800000, 0x7FC00000, 0xFFC00001, 0x7F800001)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_3_special_keys_and_the_fingerprints(ctx, order):
    """-inf, -0, +0, denormals, +inf and three NaN patterns in word 0, equally often in every segment: word 1 decides inside a class
    (-0 with +0, the NaNs together), and words 2 .. 7 arrive with their record"""
    rng = np.random.default_rng(4)
    lengths = [60, 300, 2100]
    off = offsets_of(lengths)
    w = random_records(int(off[-1]), rng)
    w[:, 0] = np.concatenate([np.tile(SPECIAL, n // len(SPECIAL))[rng.permutation(n)] for n in lengths]).view(np.uint32)
    assert_distinct_keys(off, w)
    got, _ = device_sort(ctx, off, w, order)
    assert_words(got, R.reference_records(off, w, len(w), order), order)
    index = {tuple(r[[2, 4, 5, 6, 7]]): i for i, r in enumerate(w)}         # the permutation, from the fingerprints
    src = np.array([index[tuple(r[[2, 4, 5, 6, 7]])] for r in got])
    assert (np.sort(src) == np.arange(len(w))).all() and (got == w[src]).all()
    for k in range(len(lengths)):                                           # and it stays inside the segment
        assert ((src[int(off[k]):int(off[k + 1])] >= off[k]) & (src[int(off[k]):int(off[k + 1])] < off[k + 1])).all()
    if order != R.BY_TRI:
        for k in range(len(lengths)):
            seg = got[int(off[k]):int(off[k + 1])]
            nan = np.isnan(seg[:, 0].copy().view(F))
            n_nan = 3 * (lengths[k] // len(SPECIAL))
            assert nan.sum() == n_nan and nan[-n_nan:].all()                # NaNs last in both orders
            assert (np.diff(seg[-n_nan:, 1].astype(np.int64)) > 0).all()    # one class: word 1 ascending
            zero = (seg[:, 0] & 0x7FFFFFFF) == 0
            at = np.nonzero(zero)[0]
            assert (np.diff(at) == 1).all() and (np.diff(seg[at, 1].astype(np.int64)) > 0).all()       # -0 with +0


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_4_capacity(ctx, order):
    """the segments that do not fit keep their own distinct, fingerprinted records (not a fill word: a kernel that permuted such a
    segment would show), and so does everything behind the list"""
    off, w = every_length_class()
    total = len(w)
    tail = random_records(64, np.random.default_rng(9))
    for capacity in (total, total - 1, total // 2, 1, 0):
        fit = S.fitting(off, capacity)
        own = np.repeat(fit, np.diff(off.astype(np.int64)))                # per record: its segment fits
        buf = np.concatenate([w, tail])
        want = R.reference_records(off, buf, capacity, order)
        assert (want[:total][~own] == w[~own]).all() and (want[total:] == tail).all()
        got, off_after = device_sort(ctx, off, buf, order, capacity=capacity)
        assert (off_after == off).all(), capacity
        assert_words(got, want, capacity)
        assert_words(got[:total][~own], w[~own], "a segment that does not fit stays byte for byte")
        assert_words(got[total:], tail, "behind the list")
        if capacity >= total // 2:
            assert fit.sum() > 10 and (capacity == total or not fit.all())
            if capacity < total:                                            # records BELOW the capacity in a segment that does not fit
                cut = np.nonzero(~fit & (off[:-1] < capacity) & (off[:-1] < off[1:]))[0]
                assert (off[cut + 1] - off[cut] >= 2).any()


@pytest.mark.gpu
def test_5_a_decreasing_pair_and_a_segment_that_does_not_fit_are_left_alone(ctx):
    """capacity 1 400 of a buffer of 2 000 fingerprinted records: [0, 300) fits; [300, 1400) fits (beyond one chunk); [1400, 2000)
    does not fit; [2000, 1700) decreases; [1700, 1700) is empty; [1700, 1990) does not fit either and overlaps no fitting segment"""
    rng = np.random.default_rng(5)
    off = np.array([0, 300, 1400, 2000, 1700, 1700, 1990], dtype=np.uint64)
    assert S.fitting(off, 1400).tolist() == [True, True, False, False, False, False]
    w = random_records(2000, rng)
    for order in ORDERS:
        want = R.reference_records(off, w, 1400, order)
        assert (want[:300] != w[:300]).any() and (want[300:1400] != w[300:1400]).any() and (want[1400:] == w[1400:]).all()
        got, off_after = device_sort(ctx, off, w, order, capacity=1400)
        assert (off_after == off).all()
        assert_words(got, want, order)
        assert_words(got[1400:], w[1400:], "what does not fit, and the decreasing pair, byte for byte")


@pytest.mark.gpu
def test_6_arguments(ctx):
    c2 = H().Context(0)                                # a context that never built a scene
    try:
        rng = np.random.default_rng(7)
        off = offsets_of(rng.integers(0, 9, 500).tolist() + [300])
        total = int(off[-1])
        w = random_records(total, rng)
        ob = H().DataBuffer(c2, len(off) + 1, np.uint64)
        rb = H().DataBuffer(c2, total, L().TRI_CLOSEST)
        lib, h, n = N().lib, c2.handle, len(off) - 1
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        ob.local[: len(off)] = off
        ob.sync()
        rb.local.view(np.uint32).reshape(-1, 8)[:] = w
        rb.sync()
        fn = lib.lbvh_sort_record_segments
        assert fn(None, ob.device, n, rb.device, total, 0) == -1
        assert fn(h, None, n, rb.device, total, 0) == -1
        assert fn(h, ob.device, n, None, total, 0) == -1
        assert fn(h, p(ob, 4), n, rb.device, total, 0) == -1
        for misaligned in (4, 8, 12):
            assert fn(h, ob.device, n, p(rb, misaligned), total, 0) == -1
        assert fn(h, ob.device, 1 << 32, rb.device, total, 0) == -1
        for order in (3, 4, 0xFFFFFFFF):
            assert fn(h, ob.device, n, rb.device, total, order) == -1
            assert fn(h, ob.device, 0, rb.device, total, order) == -1
        assert b"invalid argument" in lib.lbvh_last_error(h)
        for order in ORDERS:
            assert fn(h, ob.device, 0, rb.device, total, order) == 0        # count == 0 and capacity == 0: no-ops
            assert fn(h, ob.device, n, rb.device, 0, order) == 0
        assert lib.lbvh_sync(h) == 0
        assert (ob.get_data()[: len(off)] == off).all() and (R.as_words(rb.get_data()) == w).all()
        # and the call succeeds on this context, which has no scene; the Python host takes the order from the dtype
        H().sort_record_segments(c2, ob, rb, count=n)
        assert_words(rb.get_data(), R.reference_records(off, w, total, R.ASCENDING))
        H().sort_record_segments(c2, ob, rb, N().SORT_RECORDS_BY_TRI, n)
        assert_words(rb.get_data(), R.reference_records(off, w, total, R.BY_TRI))
        assert (ob.get_data()[: len(off)] == off).all()
        hb = H().DataBuffer(c2, 4, L().HIT)
        with pytest.raises(ValueError):
            H().sort_record_segments(c2, ob, hb, count=0)                   # the Python host checks the dtype
        with pytest.raises(ValueError):
            H().sort_record_segments(c2, ob, rb, 3, n)                      # and the order
        for buf in (ob, rb, hb):
            buf.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_7_the_live_path_list_is_kept(ctx):
    """test_segment_sort.py's check for the 16-byte call with the record sort between every pair of bounces: states and image equal
    the undisturbed frame's word for word, and bounces 2 and 3 and the last scatter still launch the list form of the scatter
    kernel (three launches; a dropped list launches none)."""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    count = 160 * 96
    st0 = pt.states.get_data()[:count].copy()
    rng = np.random.default_rng(8)
    off = offsets_of(rng.integers(0, 12, 3000).tolist() + [700])
    w = random_records(int(off[-1]), rng)
    ob = H().DataBuffer(ctx, len(off), np.uint64)
    rb = H().DataBuffer(ctx, len(w), L().CONTACT)
    ob.local[:] = off
    ob.sync()
    rb.local.view(np.uint32).reshape(-1, 8)[:] = w
    rb.sync()
    cam = N().Camera.from_dict(cam_d)
    h, s, lib = ctx.handle, pt.drawer.container.scene(), N().lib
    orders = iter([R.ASCENDING, R.BY_TRI, R.ASCENDING, R.BY_TRI, R.DESCENDING])

    def sort():
        H().sort_record_segments(ctx, ob, rb, next(orders))

    ctx.profile_begin()
    try:
        N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
        sort()
        N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
        for bnc in range(1, 4):
            sort()
            N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
        sort()
        N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
        N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    finally:
        prof = ctx.profile_end()
    assert (words(pt.states.get_data()[:count]) == words(st0)).all()
    assert (pt.image().view(np.uint16) == img0.view(np.uint16)).all()
    assert sum(n for name, (n, _) in prof.items() if "recsort_wave_kernel" in name) == 5
    assert sum(n for name, (n, _) in prof.items() if "recsort_block_kernel" in name) == 5
    assert sum(n for name, (n, _) in prof.items() if "path_scatter_kernel" in name and "kScatterItems" in name) == 3
    assert_words(rb.get_data(), R.reference_records(off, w, len(w), R.DESCENDING), "the list, sorted by the last call")
    ob.dispose()
    rb.dispose()
    pt.drawer.on_destroy()


# ---- GPU: the five producers on the grid ----------------------------------------------------------------------------------------

_GRID = {}


def grid_drawer(ctx):
    """(a, b, c, lo, hi, drawer) of the grid, once; a context keeps one derived traversal scene, so it is derived again"""
    if "d" not in _GRID:
        tris = grid()
        from query_support import library_boxes
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        _GRID["d"] = (*positions(tris), *library_boxes(d), d)
    _GRID["d"][-1].build_fast_scene()
    return _GRID["d"]


def produce(ctx, d, kind, queries, sort=True):
    """count only -> a buffer of exactly the total -> fill -> the device sort in the order of the dtype -> (offsets, records,
    the first-record call's output or None)"""
    _, _, _, q_layout, r_layout, _ = KINDS[kind]
    call = {"contacts": d.capsule_contacts, "boxcontacts": d.obb_contacts, "triprox": d.triangle_gather_within_distance,
            "trisegs": d.triangle_intersection_segments, "sections": d.plane_sections}[kind]
    one = {"contacts": d.capsule_deepest, "boxcontacts": d.obb_deepest, "triprox": d.triangle_closest_points}.get(kind)
    n = len(queries)
    qb = H().DataBuffer(ctx, n, getattr(L(), q_layout))
    ob = H().DataBuffer(ctx, n + 1, np.uint64)
    qb.local[:] = queries
    qb.sync()
    call(qb, ob)
    total = int(ob.get_data()[n])
    rb = H().DataBuffer(ctx, max(total, 1), getattr(L(), r_layout))
    rb.fill_u32(POISON)
    call(qb, ob, rb)
    if sort:
        H().sort_record_segments(ctx, ob, rb, count=n)
    first = None
    if one is not None:
        fb = H().DataBuffer(ctx, n, getattr(L(), r_layout))
        one(qb, fb)
        first = fb.get_data().copy()
        fb.dispose()
    off, rec = ob.get_data()[: n + 1].copy(), rb.get_data()[:total].copy()
    for buf in (qb, ob, rb):
        buf.dispose()
    return off, rec, first


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_8_after_a_producer_every_segment_is_the_sorted_brute_force(ctx, kind):
    a, b, c, lo, hi, d = grid_drawer(ctx)
    queries, ref_off, ref_rec, want = producer_case(kind, (lo, hi))
    off, rec, first = produce(ctx, d, kind, queries)
    assert (off == ref_off).all()
    assert_words(rec, want, kind)                                           # every sorted segment == the sorted reference list
    m = np.diff(off.astype(np.int64))
    got = R.as_words(rec)
    heads = off[:-1][m > 0].astype(np.int64)
    if first is not None:                                                   # the first record == the one-record call's, all eight words
        assert not np.isnan(rec[rec.dtype.names[0]]).any()                  # (no NaN depth: where the relation holds)
        assert_words(got[heads], R.as_words(first)[m > 0], kind + ": first record")
    else:                                                                   # tri strictly ascending inside every segment
        start = np.zeros(len(got), dtype=bool)
        start[heads] = True
        assert (np.diff(got[:, 3].astype(np.int64))[~start[1:]] > 0).all()
        sort_segments = TS.sort_segments if kind == "trisegs" else PS.sort_segments
        assert_words(rec, sort_segments(ref_off, ref_rec), kind + ": the numpy restatement sorted by tri")


@pytest.mark.gpu
def test_9_the_conveniences(ctx):
    a, b, c, lo, hi, d = grid_drawer(ctx)
    q, _, _, _ = producer_case("triprox", (lo, hi))
    off_h, rec_h = d.proximity_pairs(q, 0.0, sort=True)
    off_d, rec_d = d.proximity_pairs(q, 0.0, device_sort=True)
    assert (off_h == off_d).all() and len(rec_d) > 100
    assert_words(rec_d, rec_h, "proximity_pairs")
    q, _, _, _ = producer_case("trisegs", (lo, hi))
    qb = H().DataBuffer(ctx, len(q), L().TRI_QUERY)
    qb.local[:] = q
    qb.sync()
    off_h, rec_h = d.intersection_segments(qb, sort=True)
    off_d, rec_d = d.intersection_segments(qb, device_sort=True)
    assert (off_h == off_d).all() and len(rec_d) > 100
    assert_words(rec_d, rec_h, "intersection_segments")
    qb.dispose()
    q, _, _, _ = producer_case("sections", (lo, hi))
    off_h, rec_h = d.cross_sections(q)
    off_d, rec_d = d.cross_sections(q, device_sort=True)
    assert (off_h == off_d).all() and len(rec_d) > 100
    assert_words(rec_d, rec_h, "cross_sections")
    for kind, layout in (("contacts", "CAPSULE"), ("boxcontacts", "OBB")):
        q, ref_off, _, want = producer_case(kind, (lo, hi))
        qb = H().DataBuffer(ctx, len(q), getattr(L(), layout))
        qb.local[:] = q
        qb.sync()
        off_d, rec_d = d.contacts(qb, device_sort=True)
        assert (off_d == ref_off).all()
        assert_words(rec_d, want, kind + ": deepest first")
        off_w, rec_w = d.contacts(qb)                                       # the default: the walk's order, the same set
        assert_words(R.reference_records(off_w, rec_w, len(rec_w), R.DESCENDING), want, kind)
        qb.dispose()


def driver_records(kind, count, seed):
    """lbvh_driver sortedrecords' list, draw by draw -> (offsets, (total, 8) words, the order)"""
    order = KINDS[kind][5]
    set_seed, uni = splitmix()
    set_seed(seed)
    lengths = [300 + int(uni(0.0, 2000.0)) if q % 97 == 5 else int(uni(0.0, 24.0)) for q in range(count)]
    off = offsets_of(lengths)
    total = int(off[-1])
    i = np.arange(total, dtype=np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    w = (((i[:, None] * np.uint64(8) + np.arange(8, dtype=np.uint64)[None, :]) & mask) * np.uint64(2654435761) & mask).astype(np.uint32)
    q = np.repeat(np.arange(count, dtype=np.uint64), lengths)
    j = i - off[:-1][q.astype(np.int64)]
    w[:, 0] = np.array([np.floor(uni(0.0, 16.0)) * F(0.25) - F(2.0) for _ in range(total)], dtype=F).view(np.uint32)
    w[:, 1] = ((j * np.uint64(2654435761) + q) & mask).astype(np.uint32)
    w[:, 3] = ((j * np.uint64(2246822519) + np.uint64(7) * q) & mask).astype(np.uint32)
    return off, w, order


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_10_cpp_host_driver_sortedrecords(ctx, kind):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count, seed = 1000, 9
    res = json.loads(subprocess.run([exe, "sortedrecords", kind, str(count), str(seed)], check=True, capture_output=True, text=True).stdout)
    off, w, order = driver_records(kind, count, seed)
    assert_distinct_keys(off, w)
    want = R.reference_records(off, w, len(w), order)
    m = np.diff(off.astype(np.int64))
    assert res["kind"] == kind and res["order"] == order and res["segments"] == count
    assert res["total"] == len(w) and res["nonempty"] == int((m > 0).sum()) and m.max() > 1024 > 256 > m.min()
    assert res["word_sum"] == int(want.astype(np.uint64).sum())
    weighted = sum((i + 1) * int(x) for i, x in enumerate((want[:, 1] ^ want[:, 7]).tolist())) & ((1 << 64) - 1)
    assert res["weighted_sum"] == weighted
    assert weighted != sum((i + 1) * int(x) for i, x in enumerate((w[:, 1] ^ w[:, 7]).tolist())) & ((1 << 64) - 1)      # the order shows in it
