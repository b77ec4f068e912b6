"""lbvh_box_cast / lbvh_box_cast_any: first contact of a moving oriented box with the mesh, over the four-wide derived traversal
scene.  The expectation is tests/box_cast_reference.py: the header's swept separating-axis test in numpy float32, brute force over
every (cast, triangle) pair with the boxes the library produced.  Every GPU comparison is word for word on uint32 views, no
tolerance.  The restatement itself is checked against a float64 polygon clip that shares no line with it."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import box_cast_reference as BR
from query_support import driver_mesh, golden, H, L, library_boxes, N, pack, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
SIZES = (0.005, 0.02, 0.1)                  # half extents, of the scene's extent
MISS_WORDS = words(np.array([BR.MISS]))
START = 13                                  # LBVH_BOX_AXIS_START


def extent_of(a, b, c):
    pts = np.concatenate([a, b, c])
    return float((pts.max(axis=0) - pts.min(axis=0)).max())


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_both_structs_and_both_prototypes_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    m = re.search(r"typedef struct lbvh_box_ray \{(.*?)\} lbvh_box_ray;", h, re.S)
    assert m and re.findall(r"(?:float|uint32_t)\s+(\w+)", m.group(1)) == ["centre", "t_max", "dir", "_pad0", "ax", "_pad1", "ay", "_pad2",
                                                                           "az", "_pad3"]
    m = re.search(r"typedef struct lbvh_box_hit \{(.*?)\} lbvh_box_hit;", h, re.S)
    assert m and re.findall(r"(?:float|uint32_t)\s+(\w+)", m.group(1)) == ["t", "tri", "axis", "_zero"]
    assert re.search(r"#define LBVH_BOX_AXIS_START 13u", h)
    for fn, out in (("lbvh_box_cast", r"lbvh_box_hit\* d_hits"), ("lbvh_box_cast_any", r"uint32_t\* d_flags")):
        assert re.search(r"lbvh_status " + fn + r"\(lbvh_context\* ctx, const lbvh_box_ray\* d_casts, size_t count, "
                         r"const lbvh_scene\* h_scene,\s+" + out + r"\);", h), fn
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_box_cast" in bounce and "lbvh_box_cast_any" in bounce


def test_layout_signatures_csharp_and_cpp_host():
    lay, nat = L(), N()
    assert lay.BOX_RAY.itemsize == 80 and lay.BOX_HIT.itemsize == 16 and lay.BOX_AXIS_START == START
    names = ("centre", "t_max", "dir", "_pad0", "ax", "_pad1", "ay", "_pad2", "az", "_pad3")
    assert [lay.BOX_RAY.fields[k][1] for k in names] == [0, 12, 16, 28, 32, 44, 48, 60, 64, 76]
    assert [lay.BOX_HIT.fields[k][1] for k in ("t", "tri", "axis", "_zero")] == [0, 4, 8, 12]
    assert lay.BOX_RAY is BR.BOX_RAY
    for fn in ("lbvh_box_cast", "lbvh_box_cast_any"):
        res, args = nat.SIGNATURES[fn]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
        assert getattr(nat.lib, fn).argtypes is not None
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public struct BoxRay \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["centreX", "centreY", "centreZ", "tMax", "dirX", "dirY", "dirZ", "pad0", "axX", "axY",
                                                                 "axZ", "pad1", "ayX", "ayY", "ayZ", "pad2", "azX", "azY", "azZ", "pad3"]
    m = re.search(r"public struct BoxHit \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["t", "tri", "axis", "zero"]
    for fn in ("lbvh_box_cast", "lbvh_box_cast_any"):
        assert re.search(r"public static extern int " + fn + r"\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+\);", cs)
    cc = open(os.path.join(ROOT, "bindings", "csharp", "BoxCasts.cs")).read()
    assert "lbvh_box_cast(" in cc and "lbvh_box_cast_any(" in cc and "unsafe" not in cc and "stride != 80" in cc
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void BoxCast(" in hpp and "void BoxCastAny(" in hpp
    assert hasattr(H().RaytracingMeshDrawer, "box_cast") and hasattr(H().RaytracingMeshDrawer, "box_cast_any")
    assert "boxcast_main" in open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()


def test_half_axes_builder_and_the_normal():
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    ax, ay, az = H().obb_half_axes([1.0, 2.0, 3.0], rot)
    assert ax.dtype == F and np.allclose(ax, [c, s, 0]) and np.allclose(ay, [-2 * s, 2 * c, 0]) and np.allclose(az, [0, 0, 3])
    ax, ay, az = H().obb_half_axes([[1, 2, 3], [4, 5, 6]])
    assert ax.tolist() == [[1, 0, 0], [4, 0, 0]] and ay.tolist() == [[0, 2, 0], [0, 5, 0]] and az.tolist() == [[0, 0, 3], [0, 0, 6]]
    # the normal points from the triangle to the box: a box dropped on the face z = 0 from above has +z, from below -z; a vertical
    # box edge pushed in +y against the edge y = 0 has -y
    line = (np.zeros(3), np.array([8.0, 0, 0]), np.array([0, 8.0, 0]))
    cast = BR.make_casts(np.array([[2, 2, 5], [2, 2, -5], [4, -6, 0]], dtype=F), np.array([[0, 0, -1], [0, 0, 1], [0, 1, 0]], dtype=F),
                         np.array([[1, 0, 0], [1, 0, 0], [1, 1, 0]], dtype=F), np.array([[0, 1, 0], [0, 1, 0], [-1, 1, 0]], dtype=F),
                         np.array([[0, 0, 1]] * 3, dtype=F))
    assert H().box_cast_normal(cast[0], line, 0).tolist() == [0, 0, 1] and H().box_cast_normal(cast[1], line, 0).tolist() == [0, 0, -1]
    assert H().box_cast_normal(cast[2], line, 10).tolist() == [0, -1, 0] and H().box_cast_normal(cast[0], line, START) is None


# ---- CPU: known answers of the restatement, exact in fp32 ---------------------------------------------------------------

BIG = (np.array([[0, 0, 0], [500, 500, 500]], dtype=F), np.array([[8, 0, 0], [501, 500, 500]], dtype=F),
       np.array([[0, 8, 0], [500, 501, 500]], dtype=F))        # one big triangle in z = 0 and a far dummy (scenes need n >= 2)
SKEW = (np.array([[0, 0, 0], [500, 500, 500]], dtype=F), np.array([[8, 2, 1], [501, 500, 500]], dtype=F),
        np.array([[2, 8, 4], [500, 501, 500]], dtype=F))       # every extreme along x, y and z is one vertex: a lowest, b or c highest
UNIT = ([1, 0, 0], [0, 1, 0], [0, 0, 1])
TURNED = ([1, 1, 0], [-1, 1, 0], [0, 0, 1])                    # 45 degrees about z: the edges along az stand upright in front


def _face_onto_vertex():
    """an AABB of half extents (1, 2, 3) pushed along +-x, +-y, +-z onto the extreme vertex of SKEW in that direction, from 4 away:
    (centre, dir, expected axis)"""
    half = (1.0, 2.0, 3.0)
    a, b, c = (np.array(x[0], dtype=float) for x in SKEW)
    out = []
    for k, high in enumerate((b, c, c)):
        for sign, vertex in ((1.0, a), (-1.0, high)):
            e = np.eye(3)[k] * sign
            out.append(((vertex - e * (half[k] + 4.0)).tolist(), e.tolist(), 1 + k))
    return out


# (scene, centre, dir, (ax, ay, az), t_max, expected t or None for the miss record, expected axis)
KNOWN = [
    # a corner of a cube of half extent 3, turned so that (-1, 1, -5) is its lowest corner, onto the face: axis 0
    (BIG, [3, 2, 10], [0, 0, -1], ([1, 2, 2], [2, 1, -2], [2, -2, 1]), INF, 5.0, 0),
    # upright box edges against the triangle's edges: (az, e1), (az, e2), and with the axes renamed (ax, e1), (ay, e2)
    (BIG, [4, -6, 0], [0, 1, 0], TURNED, INF, 4.0, 10),
    (BIG, [-6, 4, 0], [1, 0, 0], TURNED, INF, 4.0, 11),
    (BIG, [4, -6, 0], [0, 1, 0], ([0, 0, 1], [1, 1, 0], [-1, 1, 0]), INF, 4.0, 4),
    (BIG, [-6, 4, 0], [1, 0, 0], ([1, 1, 0], [0, 0, 1], [-1, 1, 0]), INF, 4.0, 8),
    # the turned box coming at the hypotenuse face on: its face and the edge pair (az, e2 - e1) tie, the earlier axis keeps it
    (BIG, [8, 8, 0], [-1, -1, 0], TURNED, INF, 3.0, 1),
    # a start in overlap, whatever the direction
    (BIG, [2, 2, 0.5], [1, 0, 0], UNIT, INF, 0.0, START),
    (BIG, [2, 2, 0.5], [0, 0, 1], UNIT, INF, 0.0, START),
    # sliding beside the triangle, a gap of 1 in y and v = 0 on that axis: no time; sliding flush (touching in y) has one
    (BIG, [-4, -2, 0], [1, 0, 0], UNIT, INF, None, 0),
    (BIG, [-4, -1, 0], [1, 0, 0], UNIT, INF, 3.0, 1),
    # box edges parallel to triangle edges: cross(ax, e1) = cross(ay, e2) = 0 constrain nothing
    (BIG, [2, 2, 5], [0, 0, -1], UNIT, INF, 4.0, 0),
    # a sheared box (ax leans in z): its lowest edge is 2 below the centre, the unsheared box's face 1
    (BIG, [3, 3, 6], [0, 0, -1], ([1, 0, 1], [0, 1, 0], [0, 0, 1]), INF, 4.0, 0),
    (BIG, [3, 3, 6], [0, 0, -1], UNIT, INF, 5.0, 0),
    # moving away; a contact exactly at T is no candidate, the float above it is
    (BIG, [2, 2, 5], [0, 0, 1], UNIT, INF, None, 0),
    (BIG, [2, 2, 5], [0, 0, -1], UNIT, np.nextafter(F(4), F(0)), None, 0),
    (BIG, [2, 2, 5], [0, 0, -1], UNIT, F(4), None, 0),
    (BIG, [2, 2, 5], [0, 0, -1], UNIT, np.nextafter(F(4), INF), 4.0, 0),
    # a non-unit direction: t is in units of dir
    (BIG, [2, 2, 5], [0, 0, -8], UNIT, INF, 0.5, 0),
] + [(SKEW, centre, d, ([1, 0, 0], [0, 2, 0], [0, 0, 3]), INF, 4.0, axis) for centre, d, axis in _face_onto_vertex()]


def _casts(rows):
    """rows of (centre, dir, (ax, ay, az), t_max)"""
    col = lambda k: np.array([r[k] for r in rows], dtype=F).reshape(-1, 3)
    return BR.make_casts(col(0), col(1), np.array([r[2][0] for r in rows], dtype=F), np.array([r[2][1] for r in rows], dtype=F),
                         np.array([r[2][2] for r in rows], dtype=F), np.array([r[3] for r in rows], dtype=F))


def _known(scene):
    rows = [k for k in KNOWN if k[0] is scene]
    expected = [(float(L().MAX_FLOAT), 0, 0) if k[5] is None else (k[5], 0, k[6]) for k in rows]
    return _casts([k[1:5] for k in rows]), expected


def _triples(records):
    return [(float(r["t"]), int(r["tri"]), int(r["axis"])) for r in records]


@pytest.mark.parametrize("scene", [BIG, SKEW], ids=["big", "skew"])
def test_known_answers_on_one_triangle(scene):
    casts, expected = _known(scene)
    a, b, c = scene
    r = BR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert _triples(r.records) == expected
    assert r.flags.tolist() == [int(e[0] < L().MAX_FLOAT) for e in expected]
    assert not np.signbit(r.records["t"]).any() and (r.records["_zero"] == 0).all()
    if scene is SKEW:                                             # axes 1, 2, 3 with both signs of v
        assert [e[2] for e in expected] == [1, 1, 2, 2, 3, 3]
        v = [float(np.dot(casts["dir"][i], H().box_cast_axis(casts[i], (a[0], b[0] - a[0], c[0] - a[0]), expected[i][2]))) for i in range(6)]
        assert [np.sign(x) for x in v] == [1, -1, 1, -1, 1, -1]


SHARED = (([0, 0, 0], [4, 0, 0], [0, 4, 0]), ([4, 0, 0], [4, 4, 0], [0, 4, 0]))   # coplanar, sharing the edge (4, 0, 0) - (0, 4, 0)
SHARED_CASTS = [([2, 2, 5], [0, 0, -1], ([0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]), t_max) for t_max in (INF, F(4.0), F(4.5))]


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_equal_times_on_a_shared_edge_go_to_the_lower_index(order):
    a, b, c = (np.array([SHARED[o][k] for o in order], dtype=F) for k in range(3))
    r = BR.reference(_casts(SHARED_CASTS), a, b, c, *padded_boxes(a, b, c))
    assert r.ties.tolist() == [2, 0, 2] and r.records["tri"].tolist() == [0, 0, 0] and r.records["t"].tolist()[::2] == [4.0, 4.0]
    assert r.flags.tolist() == [1, 0, 1]


def inactive_forms():
    o, d, box = [2, 2, 5], [0, 0, -1], UNIT
    nan, inf = np.nan, np.inf
    return _casts([(o, d, box, 0.0), (o, d, box, -1.0), (o, d, box, nan), ([nan, 2, 5], d, box, INF), ([2, nan, 5], d, box, INF),
                   ([2, 2, nan], d, box, INF), (o, [0, inf, -1], box, INF), (o, [nan, 0, -1], box, INF), (o, [0, 0, -inf], box, INF),
                   (o, [0, 0, 0], box, INF), (o, [0, 0, -1e-30], box, INF)] +
                  [(o, d, tuple([bad if (i, k) == (row, col) else UNIT[i][k] for k in range(3)] for i in range(3)), INF)
                   for row in range(3) for col in range(3) for bad in (nan, inf, -inf)] +
                  [(o, d, ([1, 0, 0], [0, 1, 0], [1, 1, 0]), INF), (o, d, ([1, 0, 0], [0, 1, 0], [0, 0, 0]), INF),      # flat: det = 0
                   (o, d, ([1, 2, 3], [2, 4, 6], [0, 0, 1]), INF), (o, d, ([1e30, 0, 0], [0, 1e30, 0], [0, 0, 1e30]), INF)])   # det = inf


def test_every_inactive_form_is_a_miss_record():
    casts = inactive_forms()
    assert len(casts) == 11 + 27 + 4 and not BR.active(casts).any()
    a, b, c = BIG
    r = BR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert (r.flags == 0).all() and (words(r.records).reshape(-1, 4) == MISS_WORDS).all()
    live = _casts([([2, 2, 5], [0, 0, -1], UNIT, INF), ([np.inf, 2, 5], [0, 0, -1], UNIT, INF), ([2, 2, 5], [0, 0, -1], ([1, 0, 0], [1, 1, 0], [0, 0, -1]), 1e-30)])
    assert BR.active(live).all()


# ---- cast sets ----------------------------------------------------------------------------------------------------------

def random_boxes(count, half, rng):
    """(ax, ay, az) float64 (count, 3): half extents `half` * uniform(0.5, 1.5) per axis; a third each turned at random (OBB), axis
    aligned (AABB), and turned and sheared (the axes no longer orthogonal)"""
    he = half[:, None] * rng.uniform(0.5, 1.5, (count, 3))
    q = np.linalg.qr(rng.normal(size=(count, 3, 3)))[0]
    kind = np.arange(count) % 3
    q[kind == 1] = np.eye(3)
    shear = np.tile(np.eye(3), (count, 1, 1))
    for i, j in ((0, 1), (0, 2), (1, 2)):
        shear[:, i, j] = np.where(kind == 2, rng.uniform(-0.7, 0.7, count), 0.0)
    m = (q @ shear) * he[:, None, :]                                # columns: the half-axis vectors
    return m[:, :, 0], m[:, :, 1], m[:, :, 2]


def aimed_casts(a, b, c, count, rng, sizes=SIZES, plain=False):
    """Boxes that start outside the mesh's box and aim at points of its surface, the sizes in turn, random_boxes' three kinds.
    plain: unit directions, t_max = +inf and active casts only (the float64 comparison).  Otherwise a mix as the other casts'
    tests: 15 % axis-aligned directions, 40 % non-unit, half with a finite t_max around the contact, 10 % starting on a surface (in
    overlap), and inactive forms — scattered ones and one run of 70 in a row."""
    ext = extent_of(a, b, c)
    pts = np.concatenate([a, b, c])
    k = rng.integers(0, len(a), count)
    w = rng.dirichlet((1, 1, 1), count)
    target = a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
    d = rng.normal(size=(count, 3))
    if not plain:
        along = rng.random(count) < 0.15
        d[along] = np.eye(3)[rng.integers(0, 3, along.sum())] * rng.choice([-1.0, 1.0], along.sum())[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    reach = 1.25 * np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)) + 0.4 * ext
    half = np.array(sizes)[np.arange(count) % len(sizes)] * ext
    ax, ay, az = random_boxes(count, half, rng)
    origin = target - d * reach
    t_max = np.full(count, INF, dtype=F)
    if not plain:
        scale = np.where(rng.random(count) < 0.4, rng.uniform(0.25, 4.0, count), 1.0)
        d = d * scale[:, None]
        finite = rng.random(count) < 0.5
        t_max[finite] = (reach / scale * rng.uniform(0.6, 1.3, count))[finite]
        inside = rng.random(count) < 0.1
        origin[inside] = target[inside] + rng.normal(size=(inside.sum(), 3)) * (0.4 * half[inside])[:, None]
    casts = BR.make_casts(origin.astype(F), d.astype(F), ax.astype(F), ay.astype(F), az.astype(F), t_max)
    if not plain:
        dead = rng.random(count) < 0.05
        dead[count // 2: count // 2 + 70] = True
        form = rng.integers(0, 7, count)
        casts["t_max"][dead & (form == 0)] = 0.0
        casts["t_max"][dead & (form == 1)] = np.nan
        casts["t_max"][dead & (form == 2)] = -1.0
        casts["dir"][dead & (form == 3)] = 0.0
        casts["centre"][dead & (form == 4), 1] = np.nan
        casts["ay"][dead & (form == 5), 2] = np.inf
        casts["az"][dead & (form == 6)] = casts["ax"][dead & (form == 6)]                   # flat: det = 0
    return casts


def scene_positions(name):
    if name == "cfg1_4096":
        pos = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["positions"]
        return tuple(np.ascontiguousarray(pos[:, k], dtype=F) for k in range(3))
    if name == "grid_80x80":
        return positions(scenes.grid_scene())
    return positions(golden(name))


def parity_casts(name, a, b, c):
    return aimed_casts(a, b, c, 1500, np.random.default_rng(13 + len(a)))


# ---- CPU: the restatement against an independent float64 evaluation -----------------------------------------------------------
# Geometry, sharing nothing with the definition: the triangle is mapped into the box's own coordinates (numpy.linalg.solve on the
# matrix of the half-axis vectors), where the box is the cube |s_i| <= 1, and clipped against the six planes |s_i| <= h
# (Sutherland-Hodgman).  The box scaled by h overlaps the triangle iff a polygon is left.

def local_triangles(cast, time, a, b, c):
    """(T, 3 vertices, 3) float64: the triangles in the coordinates of `cast`'s box at `time`"""
    m = np.stack([cast[k].astype(np.float64) for k in ("ax", "ay", "az")], axis=1)
    centre = cast["centre"].astype(np.float64) + cast["dir"].astype(np.float64) * time
    pts = np.stack([a, b, c], axis=1).astype(np.float64) - centre
    return np.linalg.solve(m, pts.reshape(-1, 3).T).T.reshape(-1, 3, 3)


def clip_overlaps(tri, h):
    """tri: (3, 3) local coordinates.  True iff the cube |s_i| <= h and the triangle share a point."""
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


def cube_distance(tri):
    """the least h at which clip_overlaps(tri, h): the distance of the triangle from the box's centre in the box's own max-norm
    (1 = touching), by bisection to 2^-46 relative"""
    lo, hi = 0.0, float(np.abs(tri).max())
    for _ in range(46):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if clip_overlaps(tri, mid) else (mid, hi)
    return hi


def nearest_cube_distance(cast, time, a, b, c, below):
    """the least cube_distance over all triangles, as far as it is below `below` (else `below`): triangles with all three vertices
    beyond one plane |s_i| = below are farther and are not clipped"""
    loc = local_triangles(cast, time, a, b, c)
    near = ~((loc > below).all(axis=1) | (loc < -below).all(axis=1)).any(axis=1)
    return min([below] + [cube_distance(t) for t in loc[near]])


def test_the_independent_clip_knows_its_own_answers():
    tri = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0]], dtype=float)
    at = lambda centre: tri - np.array(centre, dtype=float)
    assert clip_overlaps(at([2, 2, 0.5]), 1.0) and clip_overlaps(at([2, 2, 1.0]), 1.0) and not clip_overlaps(at([2, 2, 1.0]), 0.999)
    assert not clip_overlaps(at([5, 5, 0]), 0.999) and clip_overlaps(at([5, 5, 0]), 1.0)         # a corner against the hypotenuse
    assert not clip_overlaps(at([-2, -2, 0]), 1.999) and clip_overlaps(at([-2, -2, 0]), 2.0)     # a corner against a vertex
    assert clip_overlaps(at([2, 2, 0]), 0.001) and not clip_overlaps(at([30, 2, 0]), 20.0)
    assert abs(cube_distance(at([2, 2, 3])) - 3.0) < 1e-12 and abs(cube_distance(at([5, 5, 0])) - 1.0) < 1e-12
    assert abs(cube_distance(at([-3, 4, 0])) - 3.0) < 1e-12 and cube_distance(at([2, 2, 0])) < 1e-12
    # a triangle that passes between the cube's faces without a vertex inside: the edge (3, -1, 0) - (-1, 3, 0) cuts the corner
    cut = np.array([[3, -1, 0], [-1, 3, 0], [5, 5, 0]], dtype=float)
    assert clip_overlaps(cut, 1.0) and not clip_overlaps(cut, 0.99) and abs(cube_distance(cut) - 1.0) < 1e-12
    # in a sheared box's coordinates: local_triangles maps the box's own corner centre + ax + ay + az to (1, 1, 1)
    cast = _casts([([1, 2, 3], [0, 0, -1], ([1, 0, 1], [0, 2, 0], [0.5, 0, 1]), INF)])[0]
    p = np.array([[1 + 1 + 0 + 0.5, 2 + 0 + 2 + 0, 3 + 1 + 0 + 1]], dtype=F)
    assert np.allclose(local_triangles(cast, 0.0, p, p, p)[0], 1.0) and np.allclose(local_triangles(cast, 2.0, p, p, p)[0, 0], [-1, 1, 5])


# eps = K * 2^-24 * extent / |shortest half-axis vector|, in the box's own coordinates.  The least K at which the fp32 restatement
# passes float64_check below on the CPU, found by bisecting its k_eps argument to 0.01 (the printed figures alone do not give it:
# the check a bound's worth of time before t moves with K): viking_room 3.86 (the reported triangle's distance from the box at the 10 % size), example_object3 2.23 (a triangle
# inside the deflated box a bound's worth of time before t, at the 10 % size).  DESIGN
# §33 has the table.  The test is pinned at four times the worst, the margin DESIGN §22 took for the same reason: grazing contacts
# lose the most.
K_EPS = 4 * 3.86


def missing_casts(casts, t, middle, radius, rng):
    """12 casts that have no time, made from the first 12 of `casts` (whose times are `t`): six turned so that they move at right
    angles to the line from their start to the scene's middle — they start farther from it than the scene's radius and their own
    reach together, so they never come nearer —, three stopped at half their time, three at T = t exactly (a contact at T is no
    candidate)"""
    out = casts[:12].copy()
    away = middle - out["centre"][:6].astype(np.float64)
    reach = np.linalg.norm(out["ax"][:6].astype(np.float64), axis=1) + np.linalg.norm(out["ay"][:6].astype(np.float64), axis=1) + \
        np.linalg.norm(out["az"][:6].astype(np.float64), axis=1)
    assert (np.linalg.norm(away, axis=1) > radius + reach).all()
    side = np.cross(away, rng.normal(size=(6, 3)))
    out["dir"][:6] = (side / np.linalg.norm(side, axis=1, keepdims=True)).astype(F)
    assert (t[6:12] > 0).all() and np.isfinite(t[6:12]).all()
    out["t_max"][6:9] = t[6:9] * F(0.5)
    out["t_max"][9:12] = t[9:12]
    return out


def float64_check(name, k_eps):
    """-> (casts with a time > 0, casts with none).  48 casts per size: 36 aimed at the surface (OBBs, AABBs and sheared boxes in turn,
    unit directions, open range) and missing_casts' 12.  For a cast with a time t: at t the box inflated by eps overlaps the reported
    triangle; for t > 0 the box deflated by eps overlaps no triangle a bound's worth of time earlier (eps * |shortest half-axis| /
    |dir|), nor at four times spread over [0, t).  A cast with no time: the deflated box overlaps nothing at four times spread over
    [0, T) and a bound's worth of time before T, or, for an open range, at six times along twice its way to the scene's middle."""
    a, b, c = positions(golden(name))
    ext = extent_of(a, b, c)
    pts = np.concatenate([a, b, c]).astype(np.float64)
    middle = pts.mean(axis=0)
    radius = float(np.linalg.norm(pts - middle, axis=1).max())
    contacts = missing = 0
    for j, size in enumerate(SIZES):
        rng = np.random.default_rng(300 + j)
        casts = aimed_casts(a, b, c, 36, rng, sizes=(size,), plain=True)
        t = BR.nearest(casts, a, b, c)[0]
        casts = np.concatenate([casts, missing_casts(casts, t, middle, radius, rng)])
        t, tri, axis = BR.nearest(casts, a, b, c)
        assert not np.isfinite(t[36:]).any(), (name, size, t[36:])
        worst_own = worst_early = 0.0
        for i, cast in enumerate(casts):
            shortest = min(float(np.linalg.norm(cast[k].astype(np.float64))) for k in ("ax", "ay", "az"))
            unit = 2.0 ** -24 * ext / shortest
            eps = k_eps * unit
            speed = float(np.linalg.norm(cast["dir"].astype(np.float64)))
            before = lambda time: [max(time - eps * shortest / speed, 0.0)] + [time * f for f in (0.0, 0.3, 0.6, 0.9)]
            if np.isfinite(t[i]):
                own = cube_distance(local_triangles(cast, float(t[i]), a[tri[i]:tri[i] + 1], b[tri[i]:tri[i] + 1], c[tri[i]:tri[i] + 1])[0])
                worst_own = max(worst_own, (own - 1.0) / unit)
                assert own <= 1.0 + eps, (name, size, i, "reported triangle not touched", (own - 1.0) / unit)
                times = before(float(t[i])) if t[i] > 0 else []
                contacts += t[i] > 0
            elif np.isfinite(cast["t_max"]):
                times = before(float(cast["t_max"]))
                missing += 1
            else:
                way = float(np.linalg.norm(cast["centre"].astype(np.float64) - middle)) / speed
                times = [way * f for f in np.linspace(0.0, 2.0, 6)]
                missing += 1
            for time in times:
                near = nearest_cube_distance(cast, time, a, b, c, 1.0)
                worst_early = max(worst_early, (1.0 - near) / unit)
                assert near >= 1.0 - eps, (name, size, i, time, "a triangle is inside the box before the reported time or T", (1.0 - near) / unit)
        hit = np.isfinite(t)
        print(f"{name}, half extent {size} * extent: {int(hit.sum())} with a time ({int((t == 0).sum())} at t = 0), {int((~hit).sum())} with none, "
              f"worst K: reported triangle {worst_own:.2f}, earlier overlap {worst_early:.2f}; axes {np.bincount(axis[hit], minlength=14).tolist()}")
    return contacts, missing


@pytest.mark.parametrize("name", ["viking_room", "example_object3"])
def test_reference_agrees_with_an_independent_float64_clip(name):
    contacts, missing = float64_check(name, K_EPS)
    assert contacts > 60 and missing >= 36


@pytest.mark.parametrize("name", ["viking_room", "cfg1_4096"])
def test_the_accept_rule_rejects_next_to_nothing_on_the_parity_inputs(name):
    """Of all (cast, triangle) pairs with a time in [0, T), at most 1 in 1 000 misses its grown box or has t < entry: the rule does
    not carry the parity tests.  Every pair of the first 300 parity casts is evaluated, with the Morton stage's boxes."""
    a, b, c = scene_positions(name)
    lo, hi = padded_boxes(a, b, c)
    casts = parity_casts(name, a, b, c)[:300]
    r = BR.reference(casts, a, b, c, lo, hi, casts_per_chunk=16, count_rule=True)
    print(f"{name}: {r.valid} pairs with a time, {r.rejected} rejected = {100.0 * r.rejected / max(r.valid, 1):.4f} %")
    assert r.valid > 1000 and r.rejected <= 0.001 * r.valid
    plain = BR.reference(casts, a, b, c, lo, hi)
    assert (words(plain.records) == words(r.records)).all() and (plain.flags == r.flags).all()


def test_shrunk_boxes_make_the_rule_reject():
    a, b, c = scene_positions("viking_room")
    lo, hi = padded_boxes(a, b, c)
    casts = parity_casts("viking_room", a, b, c)[:300]
    before = BR.reference(casts, a, b, c, lo, hi, casts_per_chunk=16, count_rule=True)
    picked = np.unique(before.records["tri"][before.flags == 1])[:40]
    centre, half = (lo[picked] + hi[picked]) * F(0.5), (hi[picked] - lo[picked]) * F(0.05)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[picked], hi2[picked] = centre - half, centre + half
    g = (np.abs(casts["ax"]) + np.abs(casts["ay"])) + np.abs(casts["az"])
    lo2[picked] += g.max()                                         # ... and moved off by more than any box reaches
    hi2[picked] += g.max()
    after = BR.reference(casts, a, b, c, lo2, hi2, casts_per_chunk=16, count_rule=True)
    print(f"shrunk boxes: rejected {before.rejected} -> {after.rejected}")
    assert after.valid == before.valid and after.rejected > before.rejected
    assert (words(after.records) != words(before.records)).any()


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Casts:
    """device buffers for one cast set and the two calls"""

    def __init__(self, ctx, drawer, casts):
        self.ctx, self.drawer, self.n = ctx, drawer, len(casts)
        self.casts = H().DataBuffer(ctx, self.n, L().BOX_RAY)
        self.casts.local[:] = casts
        self.casts.sync()
        self.hits = H().DataBuffer(ctx, self.n + 1, L().BOX_HIT)
        self.flags = H().DataBuffer(ctx, self.n + 1, np.uint32)

    def cast(self):
        self.hits.fill_u32(0x7FC00000)
        self.drawer.box_cast(self.casts, self.hits)
        got = self.hits.get_data().copy()
        assert (words(got[self.n:]) == 0x7FC00000).all()
        return got[: self.n]

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.box_cast_any(self.casts, self.flags)
        got = self.flags.get_data().copy()
        assert got[self.n] == 0xDEADBEEF
        return got[: self.n]

    def dispose(self):
        for b in (self.casts, self.hits, self.flags):
            b.dispose()


def assert_records(got, ref, what=""):
    bad = np.nonzero((words(got).reshape(-1, 4) != words(ref.records).reshape(-1, 4)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], ref.records[bad[:3]])


def both(ctx, drawer, casts, ref, what):
    q = Casts(ctx, drawer, casts)
    try:
        got, flags = q.cast(), q.any()
    finally:
        q.dispose()
    assert_records(got, ref, what)
    assert (flags == ref.flags).all(), (what, np.nonzero(flags != ref.flags)[0][:10])
    return got, flags


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_the_cached_scenes():
    """The parity scenes stay on the device for the tests of this file only.  Device memory a test file keeps for the rest of the
    session moves every later hipMalloc: tests/test_sort_pairs_sharded.py's retry passes a capacity larger than one of its output
    buffers, and whether the library's overlap check then trips depends on what lies next to that buffer."""
    yield
    for case in _CASES.values():
        case[3].on_destroy()
    _CASES.clear()


def parity_case(ctx, name):
    """(positions, casts, reference, drawer): the reference is computed once per scene with the library's boxes; one context keeps
    one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _CASES:
        a, b, c = scene_positions(name)
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        lo, hi = library_boxes(d)
        casts = parity_casts(name, a, b, c)
        _CASES[name] = ((a, b, c), casts, BR.reference(casts, a, b, c, lo, hi), d)
    _CASES[name][3].build_fast_scene()
    return _CASES[name]


SCENES = ["viking_room", "example_object3", "cfg1_4096", "grid_80x80"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_b1_records_and_flags_equal_the_brute_force_word_for_word(ctx, name):
    _, casts, ref, d = parity_case(ctx, name)
    got, flags = both(ctx, d, casts, ref, name)
    act = BR.active(casts)
    hit = ref.flags == 1
    by = np.bincount(ref.records["axis"][hit], minlength=14)
    print(f"{name}: {len(casts)} casts, {int(act.sum())} active, {int(hit.sum())} touch, {int((ref.records['t'][hit] == 0).sum())} at "
          f"t = 0, {int((ref.ties > 1).sum())} ties, by axis {by.tolist()}")
    assert hit.sum() > 300 and (hit & (ref.records["t"] == 0)).sum() > 20 and (act & ~hit).sum() > 30 and (~act).sum() > 70
    assert by[0] > 10 and by[1:4].sum() > 10 and by[4:13].sum() > 10 and by[13] == (hit & (ref.records["t"] == 0)).sum()
    assert (words(got[~act]).reshape(-1, 4) == MISS_WORDS).all() and (flags[~act] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", [BIG, SKEW], ids=["big", "skew"])
def test_b2_the_known_answers_and_every_inactive_form_on_the_device(ctx, scene):
    a, b, c = scene
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    casts, expected = _known(scene)
    ref = BR.reference(casts, a, b, c, *library_boxes(d))
    got, flags = both(ctx, d, casts, ref, "known answers")
    assert _triples(got) == expected and flags.tolist() == [int(e[0] < L().MAX_FLOAT) for e in expected]
    dead = inactive_forms()
    got, flags = both(ctx, d, dead, BR.reference(dead, a, b, c, *library_boxes(d)), "inactive forms")
    assert (words(got).reshape(-1, 4) == MISS_WORDS).all() and (flags == 0).all()
    d.on_destroy()


def pair_casts(count, seed=3):
    a, b, c = BIG
    rng = np.random.default_rng(seed)
    casts = aimed_casts(a[:1], b[:1], c[:1], count, rng)
    scale = rng.choice(np.array([0.3, 1.0, 10.0], dtype=F), count)[:, None]
    for k in ("ax", "ay", "az"):
        casts[k] = casts[k] * scale
    return casts


@pytest.mark.gpu
def test_b3_two_triangles_and_small_counts(ctx):
    a, b, c = BIG
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    lo, hi = library_boxes(d)
    for count in (1, 2, 63, 64, 65):
        casts = pair_casts(count, seed=count)
        casts[0] = _casts([([2, 2, 5], [0, 0, -1], ([0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]), INF)])[0]       # the first cast is a live one
        ref = BR.reference(casts, a, b, c, lo, hi)
        got, _ = both(ctx, d, casts, ref, count)
        assert got["t"][0] == F(4.5) and got["tri"][0] == 0 and got["axis"][0] == 0
    # runs of 64 or more inactive casts between active ones
    casts = pair_casts(400, seed=9)
    casts["t_max"][50:130] = 0.0
    casts["ax"][200:270, 0] = np.nan
    ref = BR.reference(casts, a, b, c, lo, hi)
    act = BR.active(casts)
    assert not act[50:130].any() and not act[200:270].any() and ref.flags[:50].sum() > 5 and ref.flags[270:].sum() > 5
    got, _ = both(ctx, d, casts, ref, "inactive runs")
    assert (words(got[~act]).reshape(-1, 4) == MISS_WORDS).all()
    d.on_destroy()


@pytest.mark.gpu
def test_b4_a_contact_on_a_shared_edge_goes_to_the_lower_index(ctx):
    casts = _casts(SHARED_CASTS)
    for order in ((0, 1), (1, 0)):
        a, b, c = (np.array([SHARED[o][k] for o in order], dtype=F) for k in range(3))
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        ref = BR.reference(casts, a, b, c, *library_boxes(d))
        assert ref.ties.tolist() == [2, 0, 2] and ref.records["tri"].tolist() == [0, 0, 0] and ref.records["t"].tolist()[::2] == [4.0, 4.0]
        _, flags = both(ctx, d, casts, ref, "shared edge")
        assert flags.tolist() == [1, 0, 1]
        d.on_destroy()


@pytest.mark.gpu
def test_b5_order_independence_under_a_shuffle_of_the_triangles(ctx):
    (a, b, c), casts, ref, d = parity_case(ctx, "cfg1_4096")
    perm = np.random.default_rng(8).permutation(len(a))                          # new index j holds old triangle perm[j]
    d2 = H().RaytracingMeshDrawer(ctx, pack(a[perm], b[perm], c[perm])).awake()
    q = Casts(ctx, d2, casts)
    got, flags = q.cast(), q.any()
    q.dispose()
    d2.on_destroy()
    assert (words(got["t"]) == words(ref.records["t"])).all() and (flags == ref.flags).all()
    unique = (ref.flags == 1) & (ref.ties == 1)
    assert unique.sum() > 300 and (perm[got["tri"][unique]] == ref.records["tri"][unique]).all()
    assert (got["axis"][unique] == ref.records["axis"][unique]).all()             # the same triangle, the same axis


@pytest.mark.gpu
def test_b6_device_stack_and_a_box_beyond_the_scene(ctx):
    (a, b, c), casts, ref, d = parity_case(ctx, "viking_room")
    h, lib = ctx.handle, N().lib
    ext = extent_of(a, b, c)
    centre = np.concatenate([a, b, c]).mean(axis=0)
    rng = np.random.default_rng(1)
    ax, ay, az = random_boxes(70, np.full(70, 3.0 * ext), rng)
    big = BR.make_casts(np.tile(centre, (70, 1)).astype(F), rng.normal(size=(70, 3)).astype(F), ax.astype(F), ay.astype(F), az.astype(F))
    rb = BR.reference(big, a, b, c, *library_boxes(d))
    try:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))                       # all but one entry in device memory
        both(ctx, d, casts, ref, "stack split 1")
        got, flags = both(ctx, d, big, rb, "a box beyond the scene, stack split 1")
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert (got["t"] == 0).all() and (got["tri"] == 0).all() and (got["axis"] == START).all() and (flags == 1).all()
    both(ctx, d, big, rb, "a box beyond the scene")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_b7_lane_refill_under_a_wave_cap(ctx, waves):
    """1 500 casts on 1, 2, 3 or 7 waves: runs of 215 .. 1 500 casts, every lane refilled many times"""
    _, casts, ref, d = parity_case(ctx, "viking_room")
    assert len(casts) == 1500
    h, lib = ctx.handle, N().lib
    try:
        N().check(h, lib.lbvh_debug_ray_waves(h, waves))
        both(ctx, d, casts, ref, f"{waves} waves")
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))


def _counted(ctx, stats, call):
    stats.fill_u32(0)
    N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    try:
        got = call()
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    s = stats.get_data()[0]
    return got, (int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"]))


@pytest.mark.gpu
def test_b8_statistics_count_the_active_casts_and_the_entry_contract(ctx):
    """what a row of tests/test_query_entry_contract.py holds for the other families: two calls give the same words, the counting
    instantiation gives the plain one's words and counts, the plain one leaves a poisoned statistics block alone, and the flag form
    never takes more node steps or triangle lines than the record form"""
    _, casts, ref, d = parity_case(ctx, "viking_room")
    q = Casts(ctx, d, casts)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    try:
        stats.fill_u32(0x7FC0DEAD)
        first, again = q.cast(), q.cast()
        assert (words(first) == words(again)).all() and (q.any() == q.any()).all()
        assert (words(stats.get_data()) == 0x7FC0DEAD).all()
        per = {}
        for name, call in (("cast", q.cast), ("any", q.any)):
            got, per[name] = _counted(ctx, stats, call)
            assert (words(got) == words(ref.records if name == "cast" else ref.flags)).all()          # the counting kernels: same answers
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
        stats.dispose()
        q.dispose()
    print("casts, node lines, triangle lines:", per)
    n_active = int(BR.active(casts).sum())
    assert per["cast"][0] == n_active and per["any"][0] == n_active
    assert per["any"][1] <= per["cast"][1] and per["any"][2] <= per["cast"][2] and per["cast"][1] >= n_active and per["cast"][2] > 0


@pytest.mark.gpu
def test_b9_errors_the_stale_scene_the_stack_limit_and_the_live_path_list(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        casts = aimed_casts(a, b, c, 600, np.random.default_rng(2))
        ref = BR.reference(casts, a, b, c, *library_boxes(d))
        assert 100 < ref.flags.sum() < 600
        q = Casts(c2, d, casts)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(casts)
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        # what lbvh_trace_rays answers before any cast: the live-path list it leaves behind is dropped by the casts below
        st = np.zeros(n, dtype=L().PATH_STATE)
        st["origin"], st["dir"], st["alive"] = casts["centre"], np.where(np.isfinite(casts["dir"]), casts["dir"], 1.0), 1
        st["origin"][~np.isfinite(st["origin"])] = 0.0
        st["alive"][7::9] = 0
        states = H().DataBuffer(c2, n, L().PATH_STATE)
        states.local[:] = st
        states.sync()
        path_hits = H().DataBuffer(c2, n, L().HIT)

        def trace_rays():
            path_hits.fill_u32(0x7FC0DEAD)
            N().check(h, lib.lbvh_trace_rays(h, states.device, n, 0.0, C.byref(s), path_hits.device))
            return words(path_hits.get_data()).copy()

        def untouched():
            return (words(q.hits.get_data()) == 0x7FC00000).all() and (q.flags.get_data() == 0xDEADBEEF).all()

        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        assert lib.lbvh_box_cast(h, q.casts.device, n, C.byref(s), q.hits.device) == -2
        assert untouched()
        expected_path = trace_rays()
        assert_records(q.cast(), ref, "after the failed reservation")
        assert (trace_rays() == expected_path).all()                                  # the list was dropped and made again
        assert (q.any() == ref.flags).all()
        assert (trace_rays() == expected_path).all()
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        for fn, who, out, off in ((lib.lbvh_box_cast, b"lbvh_box_cast: ", q.hits, 8), (lib.lbvh_box_cast_any, b"lbvh_box_cast_any: ", q.flags, 2)):
            bad = who + b"invalid argument: "
            misaligned = bad + b"((uintptr_t)d_casts & 15) == 0 && ((uintptr_t)d_out & (ANY ? 3 : 15)) == 0"
            for args in ((None, n, C.byref(s), out.device), (q.casts.device, n, None, out.device), (q.casts.device, n, C.byref(s), None)):
                assert fn(h, *args) == -1
                assert lib.lbvh_last_error(h) == bad + b"d_casts != nullptr && h_scene != nullptr && d_out != nullptr"
            assert fn(h, p(q.casts, 4), 10, C.byref(s), out.device) == -1
            assert lib.lbvh_last_error(h) == misaligned
            assert fn(h, q.casts.device, 10, C.byref(s), p(out, off)) == -1
            assert lib.lbvh_last_error(h) == misaligned
            assert fn(h, q.casts.device, 1 << 32, C.byref(s), out.device) == -1
            assert lib.lbvh_last_error(h) == bad + b"count <= 0xFFFFFFFFull"
            assert fn(None, q.casts.device, 10, C.byref(s), out.device) == -1
            assert fn(h, q.casts.device, 0, C.byref(s), out.device) == 0              # count == 0: a no-op
        assert untouched()
        # aligned sub-ranges are accepted: casts 1 .. 10 into records from record 1
        assert lib.lbvh_box_cast(h, p(q.casts, 80), 10, C.byref(s), p(q.hits, 16)) == 0
        assert (words(q.hits.get_data()[1:11]) == words(ref.records[1:11])).all()
        # a stale scene: triangles uploaded without a rebuild; the message names the entry point
        d.container.triangle_data.sync()
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        assert lib.lbvh_box_cast(h, q.casts.device, n, C.byref(s), q.hits.device) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_box_cast: ") and b"stale" in msg, msg
        assert lib.lbvh_box_cast_any(h, q.casts.device, n, C.byref(s), q.flags.device) == -1
        assert lib.lbvh_last_error(h).startswith(b"lbvh_box_cast_any: ")
        assert untouched()
        d.rebuild(fast=True)
        # the stack limit: a reported error (LBVH_ERR_HIP at the next sync), never a silently wrong record
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        q.drawer.box_cast(q.casts, q.hits)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_records(q.cast(), ref, "after the stack limit")
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_b10_path_tracer_frame_undisturbed_by_a_cast_between_bounces(ctx):
    """the casts drop the live-path list: the next lbvh_path_bounce scans again and the frame is the one without them"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    a, b, c = positions(tris)
    big = aimed_casts(a, b, c, 4 * 160 * 96, np.random.default_rng(12), sizes=(0.005,))      # 4x the frame: the scratch grows in mid-frame
    q = Casts(ctx, pt.drawer, big)
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def cast():
        pt.drawer.box_cast(q.casts, q.hits)
        pt.drawer.box_cast_any(q.casts, q.flags)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    cast()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        cast()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    cast()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    f = q.flags.get_data()[: q.n]
    assert 0 < f.sum() < q.n and ((q.hits.get_data()[: q.n]["t"] < L().MAX_FLOAT) == (f == 1)).all()
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), (7, 0.5, 1.25)])
def test_b11_cpp_host_driver_boxcast_matches_the_python_host(ctx, args):
    """`lbvh_driver boxcast` on the driver's own random mesh (default and given seed, half extent, t_max) against the Python host on
    the same triangles and the same casts"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 6000
    res = json.loads(subprocess.run([exe, "boxcast"] + [str(x) for x in args], check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(4096)
    casts = BR.driver_casts(lo, hi, count, *args)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Casts(ctx, d, casts)
    got, flags = q.cast(), q.any()
    q.dispose()
    d.on_destroy()
    assert res["triangles"] == len(tris) and res["casts"] == count and F(res["half_extent"]) == F(args[1] if args else 1.5)
    assert res["touching"] == int((got["t"] < L().MAX_FLOAT).sum()) == res["flagged"] == int(flags.sum())
    assert res["at_start"] == int((got["t"] == 0).sum())
    assert res["by_axis"] == np.bincount(got["axis"][got["t"] < L().MAX_FLOAT], minlength=14).tolist()
    assert res["word_sum"] == int(words(got).astype(np.uint64).sum())
    assert [r[1] for r in res["records"]] == got["tri"][:3].tolist() and [r[2] for r in res["records"]] == got["axis"][:3].tolist()
    assert [words(np.array(r[0], dtype=F))[0] for r in res["records"]] == words(got["t"][:3]).tolist()
    assert 0 < res["touching"] < count
