"""lbvh_capsule_overlaps / lbvh_obb_overlaps and their _any forms: which triangles a capsule or an oriented box touches where it
stands, as a CSR list and as a flag, over the four-wide derived traversal scene.  The expectation is
tests/shape_overlap_reference.py: the header's definition in numpy float32 (rule 1 over every pair with the triangles' own boxes as
the library produced them, rule 2 on the pairs that pass) — no tree.  The order inside a segment is not part of the contract, so
every GPU comparison is word for word AFTER lbvh_sort_index_segments or a host sort of each segment.
  CPU  the surface in every host; hand-built pairs with known answers, just inside and just outside; the definition against a
       float64 evaluation that shares no line with it; the one-way relation to the casts on the references; the parity sets are
       not vacuous
  T1   parity of all four calls on grid_80x80 and cfg1_4096     T2  shape counts around a wave; wave caps (the lane refill)
  T3   inactive shapes                                          T4  count-only and overflow
  T5   count == 0, every rejection, a stale scene, the live-path list     T6  the subset relations
  T7   the cast relation on the device                          T8  a small LDS stack; statistics
  T9   lbvh_driver shapes: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import box_cast_reference as BR
import capsule_reference as CR
import overlap_reference as V
import shape_overlap_reference as S
from query_support import driver_mesh, H, L, library_boxes, N, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNT = 2000
PARITY = ["grid_80x80", "cfg1_4096"]
KINDS = ["capsule", "obb"]
# The margin of the float64 check and of the enlarged region of T6, in units of 2^-24 * extent: DESIGN §33's bound, four times the
# least K at which the box cast's fp32 restatement passes its float64 clip (test_box_cast.py K_EPS).  It is the bound of a static
# overlap test on these operations — projections, one point-triangle distance —, which is what rule 2 of both shapes is.  §22's
# K = 81536 bounds the TIME of a grazing contact (its error grows as reach^2 / r in the cylinder quadratic), which nothing here
# evaluates; at these sizes its band would be as wide as the smallest shapes.
K_EPS = 4 * 3.86
NAMES = {"capsule": ("lbvh_capsule_overlaps", "lbvh_capsule_overlaps_any"), "obb": ("lbvh_obb_overlaps", "lbvh_obb_overlaps_any")}


def scene(name):
    """the triangles of the two goldens, from the seeded generators that made them (tests/test_gpu_parity.py checks they still do)"""
    tris = scenes.grid_scene() if name == "grid_80x80" else scenes.random_triangles(4096, seed=1)
    assert len(tris) == (12800 if name == "grid_80x80" else 4096)
    return tris


def extent_of(a, b, c):
    pts = np.concatenate([a, b, c]).astype(np.float64)
    return float((pts.max(axis=0) - pts.min(axis=0)).max())


def parity_shapes(kind, a, b, c, count=COUNT, seed=17):
    """Shapes of 0.5 .. 5 % of the scene's extent about points of the surface: per shape a size s and a surface point; 45 % are moved
    off by 2.5 .. 8 sizes along a random direction (most of them touch nothing), the others by up to 0.8 sizes.
    Capsules: the axis a random direction of length 0.5 .. 2 s through that point (its middle there), radius 0.2 .. 0.6 s; every
    eighth is a needle through the surface point itself (radius s / 100: where it touches, mostly the pierce alone says so).
    Boxes: half extents 0.3 .. 1 s each, turned by a random rotation; every fifth sheared (ax += 0.5 ay, az += 0.3 ax).
    -> (records, for the boxes also (rotation matrices with the axes in their COLUMNS, half extents, sheared?))"""
    rng = np.random.default_rng(seed + len(a) + (0 if kind == "capsule" else 1))
    ext = extent_of(a, b, c)
    k = rng.integers(0, len(a), count)
    w = rng.dirichlet((1, 1, 1), count)
    target = a[k].astype(np.float64) * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
    size = ext * rng.uniform(0.005, 0.05, count)
    d = rng.normal(size=(count, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    away = rng.random(count) < 0.45
    centre = target + d * (size * np.where(away, rng.uniform(2.5, 8.0, count), rng.uniform(0.0, 0.8, count)))[:, None]
    if kind == "capsule":
        h = rng.normal(size=(count, 3))
        h *= (size * rng.uniform(0.5, 2.0, count) / np.linalg.norm(h, axis=1))[:, None]
        radius = size * rng.uniform(0.2, 0.6, count)
        needle = np.arange(count) % 8 == 3
        centre[needle] = target[needle]
        radius[needle] = size[needle] / 100.0
        return S.make_capsules((centre - 0.5 * h).astype(F), h.astype(F), radius.astype(F)), None
    rot = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
    he = size[:, None] * rng.uniform(0.3, 1.0, (count, 3))
    ax, ay, az = (rot[:, :, j] * he[:, j:j + 1] for j in range(3))
    sheared = np.arange(count) % 5 == 2
    ax = np.where(sheared[:, None], ax + 0.5 * ay, ax)
    az = np.where(sheared[:, None], az + 0.3 * ax, az)
    return S.make_obbs(centre.astype(F), ax.astype(F), ay.astype(F), az.astype(F)), (rot, he, sheared)


_CPU = {}


def cpu_case(kind, name):
    """(a, b, c, box_lo, box_hi, shapes, reference with the CPU tests' padded boxes), once per kind and scene"""
    if (kind, name) not in _CPU:
        a, b, c = positions(scene(name))
        lo, hi = padded_boxes(a, b, c)
        q = parity_shapes(kind, a, b, c)[0]
        _CPU[kind, name] = (a, b, c, lo, hi, q, S.reference(q, a, b, c, lo, hi))
    return _CPU[kind, name]


def sorted_lists(offsets, tris):
    return V.sort_segments(offsets, tris)


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_structs_and_the_four_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_capsule \{ float origin\[3\]; float radius; float axis\[3\]; uint32_t _pad; \} lbvh_capsule;", h)
    assert re.search(r"typedef struct lbvh_obb \{ float centre\[3\]; uint32_t _pad0; float ax\[3\]; uint32_t _pad1;\s+"
                     r"float ay\[3\]; uint32_t _pad2; float az\[3\]; uint32_t _pad3; \} lbvh_obb;", h)
    for shape in ("capsule", "obb"):
        assert re.search(r"lbvh_status lbvh_%s_overlaps\(lbvh_context\* ctx, const lbvh_%s\* d_shapes, size_t count, const lbvh_scene\* h_scene,"
                         r"\s+uint64_t\* d_offsets, uint32_t\* d_tris, uint64_t capacity\);" % (shape, shape), h)
        assert re.search(r"lbvh_status lbvh_%s_overlaps_any\(lbvh_context\* ctx, const lbvh_%s\* d_shapes, size_t count, const lbvh_scene\* h_scene,"
                         r"\s+uint32_t\* d_flags\);" % (shape, shape), h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert all(n in bounce for pair in NAMES.values() for n in pair)
    text = h[h.index("Shape overlaps: WHICH"):h.index("lbvh_status lbvh_capsule_overlaps(")]
    for must in ("Rule 1, own box", "Rule 2, touch", "ONE WAY", "The converse is NOT promised", "NOT PART OF THE CONTRACT", "axis = 0 is allowed",
                 "SUBSET of lbvh_gather_within_distance", "d_offsets[0] included", "A NaN never counts", "LBVH_BOX_AXIS_START"):
        assert must in text, must


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    for lists, flag in NAMES.values():
        res, args = nat.SIGNATURES[lists]
        assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
        res, args = nat.SIGNATURES[flag]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
        assert hasattr(nat.lib, lists) and hasattr(nat.lib, flag)
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.CAPSULE.itemsize == 32 and lay.OBB.itemsize == 64
    assert [lay.CAPSULE.fields[f][1] for f in ("origin", "radius", "axis", "_pad")] == [0, 12, 16, 28]
    assert [lay.OBB.fields[f][1] for f in ("centre", "_pad0", "ax", "_pad1", "ay", "_pad2", "az", "_pad3")] == [0, 12, 16, 28, 32, 44, 48, 60]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    for lists, flag in NAMES.values():
        assert re.search(r"public static extern int %s\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+,"
                         r"\s+IntPtr \w+,\s+ulong capacity\);" % lists, cs)
        assert re.search(r"public static extern int %s\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);" % flag, cs)
    assert "public struct Capsule " in cs and "public struct Obb " in cs
    so = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "ShapeOverlaps.cs")).read())
    assert all(n in so for pair in NAMES.values() for n in pair) and "unsafe" not in so
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert all(f"void {m}(" in hpp for m in ("CapsuleOverlaps", "CapsuleOverlapsAny", "ObbOverlaps", "ObbOverlapsAny"))
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"shapes", shapes_main}' in drv and "lbvh_driver shapes <n_shapes> [seed]" in drv
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("capsule_overlaps", "capsule_overlaps_any", "obb_overlaps", "obb_overlaps_any", "touching"))
    caps = H().capsule_shapes([[1, 2, 3], [4, 5, 6]], [0, 0, 2], [0.5, 0.25])
    assert caps.dtype == lay.CAPSULE and caps["axis"].tolist() == [[0, 0, 2]] * 2 and caps["radius"].tolist() == [0.5, 0.25]
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])      # x -> y
    box = H().obb_shapes([1, 2, 3], [2, 3, 4], turn)
    assert box.dtype == lay.OBB and box.shape == (1,) and box["centre"][0].tolist() == [1, 2, 3]
    assert box["ax"][0].tolist() == [0, 2, 0] and box["ay"][0].tolist() == [-3, 0, 0] and box["az"][0].tolist() == [0, 0, 4]


# ---- CPU: the restatement on pairs with known answers ------------------------------------------------------------------------

TRI = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


def one_pair(shape, tri=TRI):
    """-> the reference's Result for one shape record and one scene triangle (its own box padded as the Morton stage pads it)"""
    t = np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    r = S.reference(shape, a, b, c, *padded_boxes(a, b, c))
    assert r.flags[0] == (int(r.offsets[1]) > 0) and int(r.offsets[1]) in (0, 1)
    return r


def capsule(origin, axis, radius):
    return S.make_capsules(np.array([origin], dtype=F), np.array([axis], dtype=F), F(radius))


def obb(centre, ax, ay, az):
    return S.make_obbs(*(np.array([x], dtype=F) for x in (centre, ax, ay, az)))


def test_reference_capsule_flat_on_the_face_across_an_edge_and_end_on_at_a_vertex():
    # lying over the face, parallel to it, at the height z: the triangle's own plane is its nearest feature
    for z, touches in ((0.4999, 1), (0.5001, 0), (-0.4999, 1), (-0.5001, 0)):
        assert one_pair(capsule((1, 1, z), (1, 0.5, 0), 0.5)).flags[0] == touches, z
    # a vertical axis beside the hypotenuse (4,0,0)-(0,4,0), at the horizontal distance d * sqrt(2) from it: the interior of the axis
    # is nearest to the interior of the edge — a side of the prism —, and the axis does not pass through the face
    for d, touches in ((0.49 / np.sqrt(2), 1), (0.51 / np.sqrt(2), 0)):
        r = one_pair(capsule((2 + d, 2 + d, -1), (0, 0, 2), 0.5))
        assert r.flags[0] == touches and not r.pierce_only.any(), d
    # end-on at the vertex (0, 0, 0): the axis points away from it along (-3, -4, 0) / 5, either end first
    for s, touches in ((0.999, 1), (1.001, 0)):
        assert one_pair(capsule((-0.3 * s, -0.4 * s, 0), (-3, -4, 0), 0.5)).flags[0] == touches, s
        assert one_pair(capsule((-0.3 * s - 3, -0.4 * s - 4, 0), (3, 4, 0), 0.5)).flags[0] == touches, s


def test_reference_capsule_the_pierce_alone_decides():
    # the axis goes through the face 0.51 from the nearest edge with both ends 3 away: no derived triangle is within 0.5
    r = one_pair(capsule((0.51, 1, -3), (0, 0, 6), 0.5))
    assert r.flags[0] == 1 and r.pierce_only.tolist() == [True]
    a, e1, e2 = (np.array([x], dtype=F) for x in ((0, 0, 0), (4, 0, 0), (0, 4, 0)))
    within, pierced = S.capsule_touch(np.array([[0.51, 1, -3]], dtype=F), np.array([0.5], dtype=F), np.array([[0, 0, 6]], dtype=F), a, e1, e2)
    assert not within[0] and pierced[0]
    # the same axis 0.51 outside the edge x = 0: it passes the triangle by; and one that stops short of the face
    assert one_pair(capsule((-0.51, 1, -3), (0, 0, 6), 0.5)).flags[0] == 0
    assert one_pair(capsule((0.51, 1, -3), (0, 0, 2.49), 0.5)).flags[0] == 0
    assert one_pair(capsule((0.51, 1, -3), (0, 0, 2.51), 0.5)).flags[0] == 1
    # axis = 0: a sphere
    assert one_pair(capsule((1, 1, 0.4999), (0, 0, 0), 0.5)).flags[0] == 1 and one_pair(capsule((1, 1, 0.5001), (0, 0, 0), 0.5)).flags[0] == 0


BIG = [(0, 0, 0), (8, 0, 0), (0, 8, 0)]
ROOT2 = float(np.sqrt(2.0))


def test_reference_box_a_face_against_the_triangle_and_an_edge_pair_axis_alone():
    for z, touches in ((0.9999, 1), (1.0001, 0), (-0.9999, 1), (-1.0001, 0)):
        assert one_pair(obb((2, 2, z), (1, 0, 0), (0, 1, 0), (0, 0, 1)), BIG).flags[0] == touches, z
    # a unit cube turned by 45 degrees about z: its vertical edge at x = sqrt(2) against the triangle's edge along y at
    # x = sqrt(2) + d, z = 0; the triangle's third vertex is behind and above, so its plane cuts the box's projections and no face
    # normal separates: only cross(az, e1) = the x axis does, for d > 0
    c = 1.0 / ROOT2
    box = obb((0, 0, 0), (c, c, 0), (-c, c, 0), (0, 0, 1))
    for d, touches in ((-1e-3, 1), (1e-3, 0)):
        tri = [(ROOT2 + d, -3, 0), (ROOT2 + d, 3, 0), (10, 0, 5)]
        r = one_pair(box, tri)
        assert r.flags[0] == touches and r.pairs == 1
        assert r.edge_rejected == (0 if touches else 1)
        t = np.array(tri, dtype=F)
        gaps = S.obb_gaps(box["centre"], box["ax"], box["ay"], box["az"], t[None, 0], t[None, 1] - t[None, 0], t[None, 2] - t[None, 0])[:, 0]
        assert gaps[:4].all() and (gaps[4:].all() == bool(touches))
        if not touches:
            assert not gaps[4 + 3 * 2 + 0]                                    # cross(b_2 = az, E_0 = e1)


def test_reference_a_sheared_box_is_taken_as_it_is():
    # ax = (1, 0, 0), ay = (0.5, 1, 0), az = (0, 0, 1): the faces at +-ax have the normal n = cross(ay, az) = (1, -0.5, 0), n . ax = 1.
    # A triangle in the plane n . x = 1 + d, spanned by ay and az about (1 + d, 0, 0): beside the face for d > 0.  The AABB of the
    # same box (half extents 1.5, 1, 1) contains the triangle's middle in both cases.
    ay, az = np.array([0.5, 1.0, 0.0]), np.array([0.0, 0.0, 1.0])
    box = obb((0, 0, 0), (1, 0, 0), ay, az)
    for d, touches in ((-1e-3, 1), (1e-3, 0)):
        p0 = np.array([1.0 + d, 0.0, 0.0])
        tri = [p0 + 0.3 * ay - 0.3 * az, p0 - 0.3 * ay - 0.3 * az, p0 + 0.6 * az]
        assert one_pair(box, tri).flags[0] == touches, d
        assert one_pair(obb((0, 0, 0), (1.5, 0, 0), (0, 1, 0), (0, 0, 1)), tri).flags[0] == 1


def test_reference_inactive_shapes_have_nothing():
    t = np.array(TRI, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    lo, hi = padded_boxes(a, b, c)
    caps = np.repeat(capsule((1, 1, 0.2), (1, 0, 0), 0.5), 10)
    caps["radius"][1:6] = [0.0, -1.0, np.nan, np.inf, -np.inf]
    caps["origin"][6, 1] = np.nan
    caps["axis"][7, 0], caps["axis"][8, 2], caps["axis"][9, 1] = np.nan, np.inf, -np.inf
    assert S.active(caps).tolist() == [True] + [False] * 9 and S.reference(caps, a, b, c, lo, hi).flags.tolist() == [1] + [0] * 9
    boxes = np.repeat(obb((1, 1, 0.2), (1, 0, 0), (0, 1, 0), (0, 0, 1)), 8)
    boxes["centre"][1, 0] = np.nan
    boxes["ax"][2, 1], boxes["ay"][3, 2], boxes["az"][4, 0] = np.nan, np.inf, -np.inf
    boxes["az"][5] = (1, 1, 0)                                                # flat: det == 0
    boxes["ax"][6], boxes["ay"][6], boxes["az"][6] = (3e20, 0, 0), (0, 3e20, 0), (0, 0, 3e20)      # det overflows
    boxes["az"][7] = (0, 0, -1)                                               # left-handed: det < 0 is fine
    assert S.active(boxes).tolist() == [True] + [False] * 6 + [True]
    assert S.reference(boxes, a, b, c, lo, hi).flags.tolist() == [1] + [0] * 6 + [1]


# ---- CPU: the definition against a float64 evaluation that shares no line with it ---------------------------------------------

def point_triangle_distance64(p, a, b, c):
    """rows of points and triangles, float64: the foot of the perpendicular if it is inside the triangle, else the nearest of the
    three edges"""
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(axis=1)
    foot = p - n * (((p - a) * n).sum(axis=1) / nn)[:, None]
    inside = np.ones(len(p), dtype=bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, foot - u) * n).sum(axis=1) >= 0
    best = np.where(inside, np.linalg.norm(p - foot, axis=1), np.inf)
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        s = np.clip(((p - u) * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (u + e * s[:, None]), axis=1))
    return best


def segment_segment_distance64(p, d, q, e):
    """rows of segments [p, p + d] and [q, q + e], float64 (d may be 0): the least distance, by clamping the closest points of the
    two lines and re-projecting (the candidates: the clamped line solution and the four end-to-segment distances)"""
    def to_segment(x, u, w):
        ww = (w * w).sum(axis=1)
        s = np.clip(np.where(ww > 0, ((x - u) * w).sum(axis=1) / np.where(ww > 0, ww, 1.0), 0.0), 0.0, 1.0)
        return np.linalg.norm(x - (u + w * s[:, None]), axis=1)
    best = np.minimum(np.minimum(to_segment(p, q, e), to_segment(p + d, q, e)), np.minimum(to_segment(q, p, d), to_segment(q + e, p, d)))
    dd, ee, de = (d * d).sum(axis=1), (e * e).sum(axis=1), (d * e).sum(axis=1)
    r = p - q
    den = dd * ee - de * de
    ok = den > 1e-30 * np.maximum(dd * ee, 1e-300)
    s = np.where(ok, (de * (e * r).sum(axis=1) - ee * (d * r).sum(axis=1)) / np.where(ok, den, 1.0), 0.0)
    t = np.where(ok, (dd * (e * r).sum(axis=1) - de * (d * r).sum(axis=1)) / np.where(ok, den, 1.0), 0.0)
    inner = ok & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    return np.where(inner, np.minimum(best, np.linalg.norm(r + d * s[:, None] - e * t[:, None], axis=1)), best)


def segment_triangle_distance64(o, h, a, b, c):
    """0 where the segment [o, o + h] passes through the triangle, else the least of: its ends against the triangle, it against the
    three edges"""
    best = np.minimum(point_triangle_distance64(o, a, b, c), point_triangle_distance64(o + h, a, b, c))
    for u, v in ((a, b), (b, c), (c, a)):
        best = np.minimum(best, segment_segment_distance64(o, h, u, v - u))
    n = np.cross(b - a, c - a)
    s0, s1 = ((o - a) * n).sum(axis=1), ((o + h - a) * n).sum(axis=1)
    crosses = (s0 * s1 <= 0) & (s0 != s1)
    x = o + h * np.where(crosses, s0 / np.where(crosses, s0 - s1, 1.0), 0.0)[:, None]
    inside = crosses.copy()
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, x - u) * n).sum(axis=1) >= 0
    return np.where(inside, 0.0, best)


def clip_overlaps(tri, h):
    """tri: (3, 3) in the box's own coordinates.  True iff the cube |s_i| <= h and the triangle share a point (Sutherland-Hodgman, as
    tests/test_box_cast.py does)"""
    poly = [np.asarray(p, dtype=np.float64) for p in tri]
    for i in range(3):
        for sign in (1.0, -1.0):
            out = []
            for n, p in enumerate(poly):
                q = poly[(n + 1) % len(poly)]
                dp, dq = h - sign * p[i], h - sign * q[i]
                if dp >= 0:
                    out.append(p)
                if (dp >= 0) != (dq >= 0):
                    out.append(p + (q - p) * (dp / (dp - dq)))
            poly = out
            if not poly:
                return False
    return True


def test_the_float64_helpers_know_their_own_answers():
    tri = [np.array([x], dtype=np.float64) for x in TRI]
    at = lambda *p: np.array([p], dtype=np.float64)
    assert abs(point_triangle_distance64(at(1, 1, 2), *tri)[0] - 2) < 1e-12 and abs(point_triangle_distance64(at(-3, -4, 0), *tri)[0] - 5) < 1e-12
    assert abs(point_triangle_distance64(at(3, 3, 0), *tri)[0] - ROOT2) < 1e-12
    assert segment_triangle_distance64(at(1, 1, -3), at(0, 0, 6), *tri)[0] == 0.0
    assert abs(segment_triangle_distance64(at(1, 1, 1), at(0, 0, 6), *tri)[0] - 1) < 1e-12
    assert abs(segment_triangle_distance64(at(3, 3, -1), at(0, 0, 2), *tri)[0] - ROOT2) < 1e-12          # skew to the hypotenuse
    assert abs(segment_triangle_distance64(at(-1, -5, 0.5), at(0, 10, 0), *tri)[0] - np.sqrt(1.25)) < 1e-12
    assert abs(segment_triangle_distance64(at(1, 1, 0.25), at(0, 0, 0), *tri)[0] - 0.25) < 1e-12          # a point
    assert clip_overlaps(np.array(BIG, dtype=float) - [2, 2, 1.0], 1.0) and not clip_overlaps(np.array(BIG, dtype=float) - [2, 2, 1.0], 0.999)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_an_independent_float64_evaluation(kind):
    """Every rule-1 pair of the first 700 parity shapes of cfg1_4096 and of the first 250 of grid_80x80 whose float64 margin exceeds
    K_EPS * 2^-24 * extent is decided by the fp32 definition as float64 geometry decides it: the capsule by |distance of the axis from
    the triangle - r|, the box by clipping the triangle in the box's own coordinates against the cube of half width 1 -+ eps,
    eps = the margin over the shortest half-axis vector (test_box_cast.py's measure).  At most 1 % of the pairs lie inside the band
    (sizes of 0.5 .. 5 % of the extent against a band of 10^-6 of it: the expected share is near 10^-3 or below)."""
    for name, first in (("cfg1_4096", 700), ("grid_80x80", 250)):
        a, b, c, lo, hi, shapes, _ = cpu_case(kind, name)
        shapes = shapes[:first]
        margin = K_EPS * 2.0 ** -24 * extent_of(a, b, c)
        rows, tri = np.nonzero(S.rule1(shapes, lo, hi) & S.active(shapes)[:, None])
        e1, e2 = b - a, c - a
        a64, b64, c64 = (x[tri].astype(np.float64) for x in (a, b, c))
        if kind == "capsule":
            within, pierced = S.capsule_touch(shapes["origin"][rows], shapes["radius"][rows], shapes["axis"][rows], a[tri], e1[tri], e2[tri])
            got = within | pierced
            dist = segment_triangle_distance64(shapes["origin"][rows].astype(np.float64), shapes["axis"][rows].astype(np.float64), a64, b64, c64)
            gap = dist - shapes["radius"][rows].astype(np.float64)
            sure_in, sure_out = gap < -margin, gap > margin
        else:
            got = S.obb_gaps(shapes["centre"][rows], shapes["ax"][rows], shapes["ay"][rows], shapes["az"][rows], a[tri], e1[tri], e2[tri]).all(axis=0)
            sure_in, sure_out = np.zeros(len(rows), dtype=bool), np.zeros(len(rows), dtype=bool)
            for i, (s, t) in enumerate(zip(rows, tri)):
                box = shapes[s]
                m = np.stack([box[k].astype(np.float64) for k in ("ax", "ay", "az")], axis=1)
                eps = margin / min(np.linalg.norm(m, axis=0))
                local = np.linalg.solve(m, (np.stack([a64[i], b64[i], c64[i]]) - box["centre"].astype(np.float64)).T).T
                sure_in[i] = clip_overlaps(local, 1.0 - eps)
                sure_out[i] = not sure_in[i] and not clip_overlaps(local, 1.0 + eps)
        band = ~(sure_in | sure_out)
        print(f"{kind}, {name}: {len(rows)} rule-1 pairs, {int(sure_in.sum())} touch, {int(sure_out.sum())} apart, {int(band.sum())} inside the band "
              f"({100.0 * band.mean():.3f} %)")
        assert len(rows) > 500 and sure_in.sum() > 100 and sure_out.sum() > 100
        assert band.mean() <= 0.01
        wrong = np.nonzero((sure_in & ~got) | (sure_out & got))[0]
        assert len(wrong) == 0, (kind, name, rows[wrong[:5]], tri[wrong[:5]])


# ---- CPU: the one-way relation to the casts, and the parity sets --------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_every_candidate_gives_the_cast_the_time_plus_zero(kind):
    """On the references: for every candidate pair of the parity sets, capsule_reference.capsule_time / box_cast_reference.box_time
    with a direction of three non-zero components is +0 (for the box from axis 13, LBVH_BOX_AXIS_START)."""
    dirs = np.array([[1.0, -2.0, 0.5], [-0.3, 0.7, -1.1], [1e-3, 5.0, -40.0]], dtype=F)
    for name in PARITY:
        a, b, c, lo, hi, shapes, ref = cpu_case(kind, name)
        seg = np.repeat(np.arange(len(shapes)), np.diff(ref.offsets).astype(np.int64))
        tri = ref.tris.astype(np.int64)
        e1, e2 = b - a, c - a
        assert len(seg) > 1000
        for d in dirs:
            dd = np.broadcast_to(d, (len(seg), 3)).copy()
            if kind == "capsule":
                t = CR.capsule_time(shapes["origin"][seg], dd, shapes["radius"][seg], shapes["axis"][seg], a[tri], e1[tri], e2[tri])[0]
            else:
                t, axis = BR.box_time(shapes["centre"][seg], dd, shapes["ax"][seg], shapes["ay"][seg], shapes["az"][seg], a[tri], e1[tri], e2[tri])
                assert (axis == L().BOX_AXIS_START).all()
            assert (words(t) == 0).all(), (kind, name, d, np.nonzero(words(t) != 0)[0][:5])


def test_the_parity_sets_are_not_vacuous():
    """Conditions on the REFERENCE alone: per kind and scene at least a third of the shapes have a non-empty segment and at least a
    quarter an empty one; some capsule candidates come from the pierce alone; some box pairs are rejected only by an edge-pair axis."""
    for kind in KINDS:
        for name in PARITY:
            a, b, c, lo, hi, q, r = cpu_case(kind, name)
            n = np.diff(r.offsets).astype(np.int64)
            print(f"{kind}, {name}: {100.0 * (n > 0).mean():.1f} % non-empty, longest {int(n.max())}, total {int(n.sum())} of {r.pairs} rule-1 pairs, "
                  f"pierce-only {int(r.pierce_only.sum())}, rejected by an edge-pair axis alone {r.edge_rejected}")
            assert S.active(q).all() and len(q) == COUNT
            assert (n > 0).mean() >= 1 / 3 and (n == 0).mean() >= 0.25
            assert r.pairs > int(n.sum())                            # rule 2 rejects pairs that rule 1 passed
            if kind == "capsule":
                assert r.pierce_only.sum() > 10
            else:
                assert r.edge_rejected > 10
    assert max(int(np.diff(cpu_case(k, "grid_80x80")[6].offsets).max()) for k in KINDS) >= 8


def test_driver_generator_is_deterministic_and_inside_the_box():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    caps, boxes = S.driver_shapes(lo, hi, 50, seed=5)
    caps2, boxes2 = S.driver_shapes(lo, hi, 50, seed=5)
    assert (words(caps) == words(caps2)).all() and (words(boxes) == words(boxes2)).all()
    assert (caps["origin"] >= lo).all() and (caps["origin"] <= hi).all() and (boxes["centre"] >= lo).all() and (boxes["centre"] <= hi).all()
    assert (np.abs(caps["axis"]) <= 6).all() and (caps["radius"] == 3).all() and S.active(caps).all() and S.active(boxes).all()
    assert (words(caps) != words(S.driver_shapes(lo, hi, 50, seed=6)[0])).any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Shapes:
    """device buffers of one shape set; run() = one CSR call on caller-owned buffers"""

    def __init__(self, ctx, drawer, shapes):
        self.ctx, self.drawer, self.count = ctx, drawer, len(shapes)
        self.kind = "capsule" if shapes.dtype == L().CAPSULE else "obb"
        self.fn, self.fn_any = (getattr(N().lib, n) for n in NAMES[self.kind])
        self.shapes = H().DataBuffer(ctx, max(len(shapes), 1), shapes.dtype)
        self.shapes.local[:len(shapes)] = shapes
        self.shapes.sync()
        self.offsets = H().DataBuffer(ctx, len(shapes) + 1, np.uint64)
        self.flags = H().DataBuffer(ctx, max(len(shapes), 1), np.uint32)

    def run(self, tris=None, capacity=None):
        """offsets (host copy) after one call; tris: a uint32 DataBuffer or None, capacity defaults to its size"""
        self.offsets.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        cap = 0 if tris is None else (tris.size if capacity is None else capacity)
        N().check(self.ctx.handle, self.fn(self.ctx.handle, self.shapes.device, self.count, C.byref(s), self.offsets.device,
                                           tris.device if tris is not None else None, cap))
        return self.offsets.get_data().copy()

    def lists(self, device_sort=True):
        """(offsets, tris) through the count -> allocate -> fill convenience, every segment ascending"""
        off, tris = self.drawer._csr_lists(self._call, self.shapes, 1, device_sort)
        return (off, tris) if device_sort else (off, sorted_lists(off, tris))

    def _call(self, shapes, offsets, tris=None):
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, self.fn(self.ctx.handle, shapes.device, self.count, C.byref(s), offsets.device,
                                           tris.device if tris is not None else None, tris.size if tris is not None else 0))

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        N().check(self.ctx.handle, self.fn_any(self.ctx.handle, self.shapes.device, self.count, C.byref(s), self.flags.device))
        return self.flags.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.shapes, self.offsets, self.flags):
            b.dispose()


def assert_equal_lists(got, ref, what=""):
    (go, gt), ro, rt = got, ref.offsets, ref.tris
    assert (go[:len(ro)] == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gt) == len(rt) == int(ro[-1]), what
    bad = np.nonzero(gt != rt)[0]
    assert len(bad) == 0, (what, bad[:10], gt[bad[:10]], rt[bad[:10]])


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


def gpu_case(ctx, kind, name):
    """(a, b, c, lo, hi, shapes, reference with the library's boxes, drawer): the reference once per kind and scene"""
    a, b, c, lo, hi, d = gpu_scene(ctx, name)
    if (kind, name) not in _GPU:
        q = parity_shapes(kind, a, b, c)[0]
        _GPU[kind, name] = (q, S.reference(q, a, b, c, lo, hi))
    return (a, b, c, lo, hi) + _GPU[kind, name] + (d,)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
@pytest.mark.parametrize("kind", KINDS)
def test_t1_parity_with_the_brute_force(ctx, kind, name):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, name)
    n = np.diff(ref.offsets).astype(np.int64)
    print(f"{kind}, {name}: {100.0 * (n > 0).mean():.1f} % non-empty, longest {int(n.max())}, total {int(n.sum())}")
    assert (n > 0).mean() >= 1 / 3 and (n == 0).mean() >= 0.25
    q = Shapes(ctx, d, shapes)
    assert_equal_lists(q.lists(device_sort=True), ref, "device sort")
    assert_equal_lists(q.lists(device_sort=False), ref, "host sort")
    flags = q.any()
    assert (flags == ref.flags).all() and (flags == (n > 0)).all()
    # the public conveniences of the drawer give the same lists and flags
    assert_equal_lists(d.touching(q.shapes, device_sort=True), ref, "touching()")
    q.flags.fill_u32(0xDEADBEEF)
    (d.capsule_overlaps_any if kind == "capsule" else d.obb_overlaps_any)(q.shapes, q.flags)
    assert (q.flags.get_data()[:COUNT] == ref.flags).all()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("kind", KINDS)
def test_t2_shape_counts_around_a_wave(ctx, kind, count):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "grid_80x80")
    first = int(np.nonzero(ref.flags)[0][0])                          # (the single shape is one that touches)
    sub = shapes[first:first + count]
    r = S.reference(sub, a, b, c, lo, hi)
    assert int(r.offsets[-1]) > 0
    q = Shapes(ctx, d, sub)
    assert_equal_lists(q.lists(), r, count)
    assert (q.any() == r.flags).all()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
@pytest.mark.parametrize("kind", KINDS)
def test_t2_wave_caps_refill_the_lanes(ctx, kind, waves):
    """1 500 shapes on 1, 2, 3 or 7 waves: runs of 1 500 .. 215, every lane refilled many times"""
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "grid_80x80")
    sub = shapes[:1500].copy()
    sub["origin" if kind == "capsule" else "centre"][100:235, 0] = np.nan      # a block of inactive shapes inside a run
    r = S.reference(sub, a, b, c, lo, hi)
    q = Shapes(ctx, d, sub)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        got, flags = q.lists(), q.any()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal_lists(got, r, waves)
    assert (flags == r.flags).all()
    q.dispose()


def spoiled(kind, shapes):
    """`shapes` with an inactive record at every 20th place from the 5th on, each between active neighbours: NaN and infinite
    fields, radius <= 0, det == 0; the pads (not read) filled -> (records, the places)"""
    sub = shapes.copy()
    nan, inf = F(np.nan), F(np.inf)
    if kind == "capsule":
        edits = [("radius", None, v) for v in (F(0), F(-1), nan, inf, -inf)] + [("origin", x, nan) for x in range(3)] + \
            [("axis", x, v) for x in range(3) for v in (nan, inf, -inf)]
    else:
        edits = [("centre", x, nan) for x in range(3)] + [(f, x, v) for f in ("ax", "ay", "az") for x in range(3) for v in (nan, inf, -inf)] + \
            [("flat", None, None), ("huge", None, None)]
    places = 5 + 20 * np.arange(len(edits))
    for at, (field, x, v) in zip(places, edits):
        if field == "flat":
            sub["ax"][at], sub["ay"][at], sub["az"][at] = (1, 0, 0), (0, 1, 0), (1, 1, 0)                 # det == 0 exactly
        elif field == "huge":
            sub["ax"][at], sub["ay"][at], sub["az"][at] = (3e20, 0, 0), (0, 3e20, 0), (0, 0, 3e20)       # det overflows to +inf
        elif x is None:
            sub[field][at] = v
        else:
            sub[field][at, x] = v
    for pad in [f for f in sub.dtype.names if f.startswith("_pad")]:
        sub[pad] = 0x7FC00000 if pad in ("_pad", "_pad0") else 0xFFFFFFFF
    return sub, places


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_t3_inactive_shapes_among_active_ones(ctx, kind):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "grid_80x80")
    sub, places = spoiled(kind, shapes[:700])
    act = S.active(sub)
    assert (~act).sum() == len(places) and not act[places].any()
    r = S.reference(sub, a, b, c, lo, hi)
    q = Shapes(ctx, d, sub)
    off, tris = q.lists()
    assert_equal_lists((off, tris), r)
    flags = q.any()
    assert (np.diff(off)[~act] == 0).all() and (flags[~act] == 0).all() and (flags == r.flags).all()
    # the neighbours are what they were in the full set; an inactive shape is never walked: the set of only them fetches no node
    full = np.diff(ref.offsets)[:700]
    assert (np.diff(off)[act] == full[act]).all() and np.diff(off)[act].sum() > 0
    q.dispose()
    idle = Shapes(ctx, d, sub[~act])
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    stats.fill_u32(0)
    N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    try:
        off, flags = idle.run(None), idle.any()
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    st = stats.get_data()[0]
    assert (off == 0).all() and (flags == 0).all() and (st["rays"], st["node_fetches"], st["triangle_tests"]) == (0, 0, 0)
    stats.dispose()
    idle.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_t4_count_only_and_overflow(ctx, kind):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "grid_80x80")
    total, guard = int(ref.offsets[-1]), 4096
    q = Shapes(ctx, d, shapes)
    assert (q.run(None) == ref.offsets).all()                            # capacity == 0, d_tris == NULL
    buf = H().DataBuffer(ctx, total + guard, np.uint32)
    for cap in (0, 1, total // 2, total - 1):
        buf.fill_u32(0xABABABAB)
        off = q.run(buf, capacity=cap)                                   # (capacity 0 with a buffer: still count-only)
        got = buf.get_data().copy()
        assert (off == ref.offsets).all() and int(off[-1]) == total
        assert (got[cap:] == 0xABABABAB).all(), cap                      # nothing at the capacity or beyond
        fits = np.nonzero(ref.offsets[1:] <= cap)[0]
        assert len(fits) < COUNT
        last = int(ref.offsets[fits[-1] + 1]) if len(fits) else 0
        assert (sorted_lists(ref.offsets[:(fits[-1] + 2) if len(fits) else 1], got[:last]) == ref.tris[:last]).all(), cap
    assert 0 < len(np.nonzero(ref.offsets[1:] <= total // 2)[0])
    # the retry with what the offsets asked for, twice: the same bytes
    runs = []
    for _ in range(2):
        buf.fill_u32(0xABABABAB)
        off = q.run(buf, capacity=total)
        runs.append((off, buf.get_data().copy()))
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all()
    assert (runs[0][1][total:] == 0xABABABAB).all()
    assert_equal_lists((runs[0][0], sorted_lists(runs[0][0], runs[0][1][:total])), ref)
    buf.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_t5_count_zero_rejections_a_stale_scene_and_the_live_path_list(kind):
    """the rows test_query_entry_contract.py has for the other entry points, for these four: on a context of its own"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        centre = a[rng.integers(0, 64, 130)] + rng.normal(size=(130, 3)).astype(F) * F(2)
        if kind == "capsule":
            shapes = S.make_capsules(centre, rng.normal(size=(130, 3)).astype(F), F(0.7))
        else:
            shapes = S.make_obbs(centre, *(np.broadcast_to(np.array(v, dtype=F), (130, 3)) for v in ((0.8, 0.1, 0), (0, 0.7, 0.2), (0.1, 0, 0.9))))
        ref = S.reference(shapes, a, b, c, lo, hi)
        assert 0 < ref.flags.sum() < 130
        q = Shapes(ctx, d, shapes)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, np.uint32)
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        both, flag = q.fn, q.fn_any
        dq, do, df, dl = q.shapes.device, q.offsets.device, q.flags.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, q.flags, lst)
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
        assert both(h, dq, 0, C.byref(s), do, dl, 64) == 0 and flag(h, dq, 0, C.byref(s), df) == 0     # count == 0: a no-op
        for args in ((None, 10, C.byref(s), do, None, 0), (dq, 10, None, do, None, 0), (dq, 10, C.byref(s), None, None, 0),
                     (dq, 10, C.byref(s), do, None, 5), (at(q.shapes, 4), 10, C.byref(s), do, None, 0),
                     (dq, 10, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, C.byref(s), do, at(lst, 2), 8),
                     (dq, 1 << 32, C.byref(s), do, None, 0)):
            assert both(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(NAMES[kind][0].encode() + b": invalid argument")
        for args in ((None, 10, C.byref(s), df), (dq, 10, None, df), (dq, 10, C.byref(s), None), (at(q.shapes, 8), 10, C.byref(s), df),
                     (dq, 10, C.byref(s), at(q.flags, 2)), (dq, 1 << 32, C.byref(s), df)):
            assert flag(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(NAMES[kind][1].encode() + b": invalid argument")
        assert both(None, dq, 10, C.byref(s), do, None, 0) == -1 and flag(None, dq, 10, C.byref(s), df) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        for fn, args, name in ((both, (do, None, 0), NAMES[kind][0].encode()), (flag, (df,), NAMES[kind][1].encode())):
            assert fn(h, dq, 130, C.byref(s), *args) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        assert (trace_rays() == expected_path).all()
        # aligned sub-ranges are fine; the plain and the counting instantiation write the same words, and the latter counts
        stride = shapes.dtype.itemsize
        assert both(h, at(q.shapes, stride), 10, C.byref(s), at(q.offsets, 8), at(lst, 4), 8) == 0
        assert flag(h, at(q.shapes, stride), 10, C.byref(s), at(q.flags, 4)) == 0
        stats.fill_u32(0x7FC0DEAD)
        for form in (q.lists, q.any):
            # each call drops the live-ray list the trace before it left: lbvh_trace_rays makes its own again
            assert (trace_rays() == expected_path).all()
            form()
        assert (trace_rays() == expected_path).all()
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
        got = stats.get_data()[0]
        assert (counted[0][0] == plain[0][0]).all() and (counted[0][1] == plain[0][1]).all() and (counted[1] == plain[1]).all()
        assert got["rays"] > 0 and got["node_fetches"] > 0 and got["triangle_tests"] > 0, got
        for buf in (lst, stats, states, path_hits):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


def pairs_of(offsets, tris, n):
    seg = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets).astype(np.int64))
    return seg * n + tris


@pytest.mark.gpu
def test_t6_capsule_lists_are_subsets_of_the_broad_phase_and_of_the_sphere_gather(ctx):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "capsule", "grid_80x80")
    n = len(a)
    q = Shapes(ctx, d, shapes)
    off, tris = q.lists()
    # lbvh_box_overlaps on the capsule's AABB, min / max of the two ends -+ r in float64, rounded to fp32 and padded by 2^-21 of the
    # largest coordinate: rule 1 rounds twice per bound on the triangle's side, the AABB is rounded on the capsule's
    o, h, r = shapes["origin"].astype(np.float64), shapes["axis"].astype(np.float64), shapes["radius"].astype(np.float64)[:, None]
    pad = 2.0 ** -21 * float(np.abs(np.concatenate([a, b, c])).max() + np.abs(o).max())
    boxes = H().DataBuffer(ctx, COUNT, L().AABB)
    boxes.local[:] = V.make_boxes((np.minimum(o, o + h) - r - pad).astype(F), (np.maximum(o, o + h) + r + pad).astype(F))
    boxes.sync()
    boff, btris = d.overlaps(boxes, device_sort=True)
    assert np.isin(pairs_of(off, tris, n), pairs_of(boff, btris, n)).all() and len(tris) < len(btris)
    print(f"capsules: {len(tris)} candidates of {len(btris)} box overlaps ({len(btris) / len(tris):.2f} x)")
    boxes.dispose()
    q.dispose()
    # axis = 0: a subset of lbvh_gather_within_distance at the same points with r2 = r * r
    balls = shapes.copy()
    balls["axis"] = 0
    q = Shapes(ctx, d, balls)
    off, tris = q.lists()
    pq = H().DataBuffer(ctx, COUNT, L().POINT_QUERY)
    pq.local["p"], pq.local["max_dist2"] = balls["origin"], balls["radius"] * balls["radius"]
    pq.sync()
    goff, gtris = d.overlaps(pq, device_sort=True)
    assert len(tris) > 1000 and np.isin(pairs_of(off, tris, n), pairs_of(goff, gtris, n)).all()
    assert_equal_lists((off, tris), S.reference(balls, a, b, c, lo, hi), "axis = 0")
    pq.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t6_box_lists_are_subsets_of_the_region_query_on_an_enlarged_box(ctx):
    """lbvh_region_overlaps(TOUCHING) keeps every triangle whose own box is not wholly outside a plane: a triangle that touches the box
    has a point inside all six.  obb_planes takes orthogonal axes, so the sheared fifth of the set is left out; the half extents are
    enlarged by K_EPS * 2^-24 * extent, the bound the float64 check of the definition holds at, plus the planes' own fp32 rounding
    (2^-22 of the largest coordinate)."""
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "obb", "grid_80x80")
    rot, he, sheared = parity_shapes("obb", a, b, c)[1]
    keep = np.nonzero(~sheared)[0]
    n = len(a)
    q = Shapes(ctx, d, shapes[keep])
    off, tris = q.lists()
    grow = K_EPS * 2.0 ** -24 * extent_of(a, b, c) + 2.0 ** -22 * float(np.abs(np.concatenate([a, b, c])).max())
    regions = H().DataBuffer(ctx, len(keep), L().REGION)
    regions.local[:] = H().obb_planes(shapes["centre"][keep], np.swapaxes(rot[keep], 1, 2), he[keep] + grow)
    regions.sync()
    roff, rtris = d.in_regions(regions, L().REGION_TOUCHING, device_sort=True)
    assert len(tris) > 1000 and np.isin(pairs_of(off, tris, n), pairs_of(roff, rtris, n)).all() and len(tris) < len(rtris)
    regions.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_t7_a_shape_that_touches_makes_the_cast_start_in_overlap(ctx, kind):
    """On the device: every shape with a non-empty segment gives t == +0 in lbvh_capsule_cast / lbvh_box_cast (axis 13) for a
    direction of three non-zero components, and the cast's triangle is <= the least index of the segment."""
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "cfg1_4096")
    q = Shapes(ctx, d, shapes)
    off, tris = q.lists()
    q.dispose()
    lay = L()
    casts = H().DataBuffer(ctx, COUNT, lay.CAPSULE_RAY if kind == "capsule" else lay.BOX_RAY)
    hits = H().DataBuffer(ctx, COUNT, lay.HIT if kind == "capsule" else lay.BOX_HIT)
    for f in shapes.dtype.names:
        if not f.startswith("_pad"):
            casts.local[f] = shapes[f]
    casts.local["dir"], casts.local["t_max"] = (0.5, -1.0, 2.0), 1.0
    casts.sync()
    (d.capsule_cast if kind == "capsule" else d.box_cast)(casts, hits)
    got = hits.get_data()[:COUNT]
    has = np.nonzero(np.diff(off) > 0)[0]
    least = np.array([tris[int(off[k]):int(off[k + 1])].min() for k in has])
    assert len(has) > COUNT // 3
    assert (words(got["t"][has]) == 0).all() and (got["tri"][has] <= least).all()
    if kind == "obb":
        assert (got["axis"][has] == lay.BOX_AXIS_START).all()
    casts.dispose()
    hits.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_t8_a_small_lds_stack_and_the_statistics(ctx, kind):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, kind, "grid_80x80")
    q = Shapes(ctx, d, shapes)
    h, lib = ctx.handle, N().lib
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
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("shapes, node fetches, triangle lines: count-only %s, full %s, any %s" % tuple(seen))
    assert seen[0][0] == COUNT and seen[1] == tuple(2 * x for x in seen[0]) and seen[2][0] == COUNT
    assert seen[0][2] == ref.pairs                                   # one triangle line per pair that passes rule 1
    assert 0 < seen[2][1] <= seen[0][1] and 0 < seen[2][2] <= seen[0][2]
    for buf in (stats, big):
        buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t9_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver shapes 2000 7`: CapsuleOverlaps / ObbOverlaps, SortIndexSegments and the _any forms of lbvh_host.hpp on the driver's own
    mesh and shapes, against the brute force on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "shapes", str(count), "7"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    boxes = library_boxes(d)
    d.on_destroy()
    assert (res["triangles"], res["shapes"]) == (4096, count)
    for kind, shapes in zip(KINDS, S.driver_shapes(lo, hi, count, seed=7)):
        r = S.reference(shapes, a, b, c, *boxes)
        n = np.diff(r.offsets).astype(np.int64)
        weighted = int(((np.arange(len(r.tris), dtype=np.uint64) + np.uint64(1)) * r.tris.astype(np.uint64)).sum())
        got = res[kind]
        assert int(r.offsets[-1]) > 100
        assert (got["total"], got["non_empty"], got["flagged"], got["weighted_index_sum"]) == \
            (int(r.offsets[-1]), int((n > 0).sum()), int(r.flags.sum()), weighted), kind
        first = np.nonzero(n)[0][:3]
        assert got["segments"] == [[int(k)] + r.tris[int(r.offsets[k]):int(r.offsets[k + 1])].tolist() for k in first], kind
