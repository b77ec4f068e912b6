"""lbvh_capsule_cast / lbvh_capsule_cast_any: first contact of a moving capsule with the mesh, over the four-wide derived traversal
scene.  The expectation is tests/capsule_reference.py: the header's definition in numpy float32 through the sphere cast's own
restatement, brute force over every (cast, triangle) pair with the boxes the library produced.  Every GPU comparison is word for
word on uint32 views, no tolerance."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import capsule_reference as CR
import ray_reference as RR
import sweep_reference as S
import triangle_query_reference as TQ
from query_support import driver_mesh, golden, H, L, library_boxes, N, pack, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
RADII = (0.005, 0.02, 0.1)                  # of the scene's extent: test_sphere_cast.py's
LENGTHS = (0.0, 2.0, 8.0)                   # |axis| in radii
MISS_WORDS = words(np.array([CR.MISS]))


def extent_of(a, b, c):
    pts = np.concatenate([a, b, c])
    return float((pts.max(axis=0) - pts.min(axis=0)).max())


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_the_struct_and_both_prototypes_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    m = re.search(r"typedef struct lbvh_capsule_ray \{(.*?)\} lbvh_capsule_ray;", h, re.S)
    assert m and re.findall(r"(?:float|uint32_t)\s+(\w+)", m.group(1)) == ["origin", "radius", "dir", "t_max", "axis", "_pad"]
    for fn, out in (("lbvh_capsule_cast", r"lbvh_hit\* d_hits"), ("lbvh_capsule_cast_any", r"uint32_t\* d_flags")):
        assert re.search(r"lbvh_status " + fn + r"\(lbvh_context\* ctx, const lbvh_capsule_ray\* d_casts, size_t count, "
                         r"const lbvh_scene\* h_scene,\s+" + out + r"\);", h), fn
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_capsule_cast" in bounce and "lbvh_capsule_cast_any" in bounce


def test_layout_signatures_csharp_and_cpp_host():
    lay, nat = L(), N()
    assert lay.CAPSULE_RAY.itemsize == 48
    assert [lay.CAPSULE_RAY.fields[k][1] for k in ("origin", "radius", "dir", "t_max", "axis", "_pad")] == [0, 12, 16, 28, 32, 44]
    assert lay.CAPSULE_RAY is CR.CAPSULE_RAY
    for fn in ("lbvh_capsule_cast", "lbvh_capsule_cast_any"):
        res, args = nat.SIGNATURES[fn]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
        assert getattr(nat.lib, fn).argtypes is not None
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public struct CapsuleRay \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["originX", "originY", "originZ", "radius", "dirX", "dirY", "dirZ", "tMax",
                                                                 "axisX", "axisY", "axisZ", "pad"]
    for fn in ("lbvh_capsule_cast", "lbvh_capsule_cast_any"):
        assert re.search(r"public static extern int " + fn + r"\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+\);", cs)
    cc = open(os.path.join(ROOT, "bindings", "csharp", "CapsuleCasts.cs")).read()
    assert "lbvh_capsule_cast(" in cc and "lbvh_capsule_cast_any(" in cc and "unsafe" not in cc and "stride != 48" in cc
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void CapsuleCast(" in hpp and "void CapsuleCastAny(" in hpp
    assert hasattr(H().RaytracingMeshDrawer, "capsule_cast") and hasattr(H().RaytracingMeshDrawer, "capsule_cast_any")


# ---- CPU: known answers of the restatement, exact in fp32 ---------------------------------------------------------------

BIG = (np.array([[0, 0, 0], [500, 500, 500]], dtype=F), np.array([[8, 0, 0], [501, 500, 500]], dtype=F),
       np.array([[0, 8, 0], [500, 501, 500]], dtype=F))        # one big triangle in z = 0 and a far dummy (scenes need n >= 2)


def _casts(origin, direction, radius, axis, t_max=INF):
    rows = lambda x: np.asarray(x, dtype=F).reshape(-1, 3)
    return CR.make_casts(rows(origin), rows(direction), radius, rows(axis), t_max)


def _one(origin, direction, radius, axis, t_max=INF, tri=BIG):
    a, b, c = tri
    return CR.reference(_casts(origin, direction, radius, axis, t_max), a, b, c, *padded_boxes(a, b, c))


def _record(r, k=0):
    return float(r.records["t"][k]), int(r.records["tri"][k]), float(r.records["u"][k]), float(r.records["v"][k]), int(r.which[k]), float(r.s[k])


def test_known_answers_on_one_triangle():
    # upright, dropped on the face from height 5 with r = 1: the end at the origin arrives first, s = 0; the mirrored capsule (origin
    # at the top, the axis pointing down) touches with its other end, s = 1, through the shifted copy of the triangle
    r = _one([[2, 2, 5], [2, 2, 8]], [[0, 0, -1]] * 2, F(1.0), [[0, 0, 3], [0, 0, -3]])
    assert _record(r, 0) == (4.0, 0, 0.25, 0.25, 0, 0.0) and _record(r, 1) == (4.0, 0, 0.25, 0.25, 1, 1.0) and r.flags.tolist() == [1, 1]
    # lying parallel to the face: the triangle and its shifted copy are met at the same time, the first one keeps it
    r = _one([[2, 2, 5]], [[0, 0, -1]], F(1.0), [[2, 0, 0]])
    assert _record(r) == (4.0, 0, 0.25, 0.25, 0, 0.0)
    # upright beside the triangle, the axis crossed over the line of edge ab (from z = -0.75 to 0.75), moving onto the edge: the
    # cylinder meets the edge at t = 4 with the middle of the axis, a contact on the side over ab; each end sphere alone is later
    cast = dict(origin=[[2, -5, -0.75]], direction=[[0, 1, 0]], radius=F(1.0), axis=[[0, 0, 1.5]])
    r = _one(**cast)
    assert _record(r) == (4.0, 0, 0.25, 0.0, 2, 0.5)
    a, b, c = BIG
    for end in ([[2, -5, -0.75]], [[2, -5, 0.75]]):
        alone = S.reference(CR.as_spheres(_casts(end, cast["direction"], F(1.0), [[0, 0, 0]])), a, b, c, *padded_boxes(a, b, c))
        assert alone.flags[0] == 1 and 4.3 < alone.records["t"][0] < 4.4
    # the same over edge ca near a, a contact in the half of that side next to the edge a - a': derived triangle 7, (A', C', A)
    r = _one([[-5, 1, -0.75]], [[1, 0, 0]], F(1.0), [[0, 0, 1.5]])
    assert _record(r) == (4.0, 0, 0.0, 0.125, 7, 0.5)
    # and with the axis pointing the other way: the other triangle of the side over ab, s = 1 - v'
    r = _one([[6, -5, 0.75]], [[0, 1, 0]], F(1.0), [[0, 0, -1.5]])
    assert _record(r)[:4] == (4.0, 0, 0.75, 0.0) and _record(r)[4] in (2, 3) and _record(r)[5] == 0.5
    # the axis through the face at the start, ends and edges farther than r: t = +0, s = t_p = 3 / 8, whatever the direction
    r = _one([[2, 2, -3]] * 2, [[1, 0, 0], [0, 0, 1]], F(1.0), [[0, 0, 8]] * 2)
    assert _record(r, 0) == (0.0, 0, 0.25, 0.25, CR.PIERCE, 0.375) == _record(r, 1) and not np.signbit(r.records["t"]).any()
    # ... and neither end sphere overlaps there, nor does a row of five spheres along the axis
    row = np.array([[2, 2, -3 + 2 * k] for k in range(5)], dtype=F)
    spheres = S.reference(CR.as_spheres(_casts(row, [[1, 0, 0]] * 5, F(0.9), [[0, 0, 0]] * 5, F(0.5))), a, b, c, *padded_boxes(a, b, c))
    assert (spheres.flags == 0).all()
    # moving away, and t_max just short of the contact / just past it (the bound is strict)
    r = _one([[2, 2, 5]] * 4, [[0, 0, 1]] + [[0, 0, -1]] * 3, F(1.0), [[0, 0, 3]] * 4,
             np.array([np.inf, np.nextafter(F(4), F(0)), 4.0, np.nextafter(F(4), INF)], dtype=F))
    assert r.flags.tolist() == [0, 0, 0, 1] and (words(r.records[:3]).reshape(-1, 4) == MISS_WORDS).all()


def test_axis_zero_is_the_sphere_cast():
    origin = [[2, 2, 5], [4, -5, 0], [-3, -4, 0], [2, 2, 0.5], [-5, 2, 0.999], [2, 2, 5]]
    direction = [[0, 0, -1], [0, 1, 0], [0.6, 0.8, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]]
    a, b, c = BIG
    casts = _casts(origin, direction, F(1.0), np.zeros((6, 3)))
    r = CR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    sph = S.reference(CR.as_spheres(casts), a, b, c, *padded_boxes(a, b, c))
    assert r.flags.tolist() == [1, 1, 1, 1, 1, 0] and (words(r.records) == words(sph.records)).all() and (r.flags == sph.flags).all()
    assert (r.which == 0).all()


def test_every_inactive_form_is_a_miss_record():
    o, d, h = [2, 2, 5], [0, 0, -1], [0, 0, 3]
    forms = [(o, d, 0.0, INF, h), (o, d, -1.0, INF, h), (o, d, np.nan, INF, h), (o, d, np.inf, INF, h), (o, d, 1.0, 0.0, h),
             (o, d, 1.0, -1.0, h), (o, d, 1.0, np.nan, h), ([np.nan, 2, 5], d, 1.0, INF, h), (o, [0, np.inf, -1], 1.0, INF, h),
             (o, [0, np.nan, -1], 1.0, INF, h), (o, [0, 0, 0], 1.0, INF, h), (o, [0, 0, -1e-30], 1.0, INF, h),
             (o, d, 1.0, INF, [0, np.inf, 3]), (o, d, 1.0, INF, [-np.inf, 0, 0]), (o, d, 1.0, INF, [0, 0, np.nan])]
    casts = CR.make_casts(np.array([f[0] for f in forms], dtype=F), np.array([f[1] for f in forms], dtype=F),
                          np.array([f[2] for f in forms], dtype=F), np.array([f[4] for f in forms], dtype=F),
                          np.array([f[3] for f in forms], dtype=F))
    assert not CR.active(casts).any()
    a, b, c = BIG
    r = CR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert (r.flags == 0).all() and (words(r.records).reshape(-1, 4) == MISS_WORDS).all()
    assert CR.active(_casts([o, o], [d, d], F(1.0), [h, [0, 0, 0]])).all()


# ---- cast sets ----------------------------------------------------------------------------------------------------------

def aimed_casts(a, b, c, count, rng, radii=RADII, lengths=LENGTHS, plain=False):
    """Capsules that start outside the mesh's box and aim at points of its surface.  The radii in turn and, every third cast, the
    next axis length (in radii); the axis in a random direction, in the plane of the aimed-at face, or parallel to dir, a third
    each.  plain: unit directions, t_max = +inf and active casts only (the float64 comparison).  Otherwise a mix as
    test_sphere_cast.py's: 15 % axis-aligned directions, 40 % non-unit, half with a finite t_max around the contact, 10 % starting
    on a surface (in overlap, or pierced by it), and inactive forms — scattered ones and one run of 70 in a row."""
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
    reach = 1.25 * np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)) + 0.2 * ext
    radius = (np.array(radii)[np.arange(count) % len(radii)] * ext).astype(F)
    length = np.array(lengths)[(np.arange(count) // len(radii)) % len(lengths)] * radius
    kind = rng.integers(0, 3, count)
    h = rng.normal(size=(count, 3))
    in_plane = (b[k] - a[k]) * rng.normal(size=(count, 1)) + (c[k] - a[k]) * rng.normal(size=(count, 1))
    h[kind == 1] = in_plane[kind == 1]
    h[kind == 2] = d[kind == 2] * rng.choice([-1.0, 1.0], (kind == 2).sum())[:, None]
    norm = np.linalg.norm(h, axis=1, keepdims=True)
    h = np.where(norm > 0, h / np.where(norm > 0, norm, 1.0), 0.0) * length[:, None]
    origin = target - d * reach - h * rng.random((count, 1))           # some point of the axis is aimed at the target
    t_max = np.full(count, INF, dtype=F)
    if not plain:
        scale = np.where(rng.random(count) < 0.4, rng.uniform(0.25, 4.0, count), 1.0)
        d = d * scale[:, None]
        finite = rng.random(count) < 0.5
        t_max[finite] = (reach / scale * rng.uniform(0.6, 1.3, count))[finite]
        inside = rng.random(count) < 0.1
        origin[inside] = (target - h * rng.random((count, 1)))[inside] + rng.normal(size=(inside.sum(), 3)) * (0.4 * radius[inside])[:, None]
    casts = CR.make_casts(origin.astype(F), d.astype(F), radius, h.astype(F), t_max)
    if not plain:
        dead = rng.random(count) < 0.05
        dead[count // 2: count // 2 + 70] = True
        form = rng.integers(0, 6, count)
        casts["radius"][dead & (form == 0)] = 0.0
        casts["radius"][dead & (form == 1)] = np.nan
        casts["t_max"][dead & (form == 2)] = -1.0
        casts["dir"][dead & (form == 3)] = 0.0
        casts["origin"][dead & (form == 4), 1] = np.nan
        casts["axis"][dead & (form == 5), 2] = np.inf
    return casts


def scene_positions(name):
    if name == "cfg1_4096":
        pos = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["positions"]
        return tuple(np.ascontiguousarray(pos[:, k], dtype=F) for k in range(3))
    if name == "grid_80x80":
        return positions(scenes.grid_scene())
    return positions(golden(name))


COUNTS = {"viking_room": 1500, "example_object3": 1000, "cfg1_4096": 1500, "grid_80x80": 1000}


def parity_casts(name, a, b, c):
    return aimed_casts(a, b, c, COUNTS[name], np.random.default_rng(11 + len(a)))


# ---- CPU: the restatement against an independent float64 evaluation -----------------------------------------------------------
# The distance between a segment and a triangle, written from the geometry and sharing nothing with the definition: the least of
# both ends to the triangle (projection on the plane, or the nearest edge), the segment to the three edges (clamped closest points
# of two segments), and 0 where the segment goes through the face.

def _point_segment(p, q0, q1):
    e = q1 - q0
    ee = np.einsum("...k,...k->...", e, e)
    s = np.clip(np.einsum("...k,...k->...", p - q0, e) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
    return np.linalg.norm(p - (q0 + e * s[..., None]), axis=-1)


def _point_triangle(p, a, b, c):
    n = np.cross(b - a, c - a)
    nn = np.einsum("...k,...k->...", n, n)
    with np.errstate(all="ignore"):
        height = np.einsum("...k,...k->...", p - a, n) / np.sqrt(nn)
        foot = p - n * (np.einsum("...k,...k->...", p - a, n) / nn)[..., None]
        inside = True
        for q0, q1 in ((a, b), (b, c), (c, a)):
            inside = inside & (np.einsum("...k,...k->...", np.cross(q1 - q0, foot - q0), n) >= 0)
    edges = np.minimum(np.minimum(_point_segment(p, a, b), _point_segment(p, b, c)), _point_segment(p, c, a))
    return np.where(inside & (nn > 0), np.abs(height), edges)


def _segment_segment(p0, p1, q0, q1):
    """Ericson 5.1.9, vectorised; degenerate segments fall back on the end points, which the callers cover anyway"""
    d1, d2, r = p1 - p0, q1 - q0, p0 - q0
    dot = lambda x, y: np.einsum("...k,...k->...", x, y)
    aa, ee, f, bb, cc = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, d2), dot(d1, r)
    den = aa * ee - bb * bb
    with np.errstate(all="ignore"):
        s = np.where(den > 0, np.clip((bb * f - cc * ee) / den, 0.0, 1.0), 0.0)
        t = np.where(ee > 0, (bb * s + f) / ee, 0.0)
        s = np.where(t < 0, np.clip(np.where(aa > 0, -cc / aa, 0.0), 0.0, 1.0), np.where(t > 1, np.clip(np.where(aa > 0, (bb - cc) / aa, 0.0), 0.0, 1.0), s))
        t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm((p0 + d1 * s[..., None]) - (q0 + d2 * t[..., None]), axis=-1)


def segment_triangle_distance(p0, p1, a, b, c):
    """float64, the arrays broadcast over their leading axes"""
    p0, p1, a, b, c = (np.asarray(x, dtype=np.float64) for x in (p0, p1, a, b, c))
    dist = np.minimum(_point_triangle(p0, a, b, c), _point_triangle(p1, a, b, c))
    for q0, q1 in ((a, b), (b, c), (c, a)):
        dist = np.minimum(dist, _segment_segment(p0, p1, q0, q1))
    n = np.cross(b - a, c - a)
    s0, s1 = np.einsum("...k,...k->...", p0 - a, n), np.einsum("...k,...k->...", p1 - a, n)
    with np.errstate(all="ignore"):
        x = p0 + (p1 - p0) * (s0 / (s0 - s1))[..., None]
        through = (s0 * s1 <= 0) & (s0 != s1)
        for q0, q1 in ((a, b), (b, c), (c, a)):
            through = through & (np.einsum("...k,...k->...", np.cross(q1 - q0, x - q0), n) >= 0)
    return np.where(through, 0.0, dist)


def test_the_independent_distance_knows_its_own_answers():
    a, b, c = (np.array(v, dtype=float) for v in ([0, 0, 0], [8, 0, 0], [0, 8, 0]))
    d = lambda p0, p1: float(segment_triangle_distance(np.array(p0, dtype=float), np.array(p1, dtype=float), a, b, c))
    assert d([2, 2, 3], [2, 2, 5]) == 3.0 and d([2, 2, -3], [2, 2, 5]) == 0.0 and d([2, -5, -1], [2, -5, 1]) == 5.0
    assert abs(d([-1, -1, 2], [9, 9, 2]) - 2.0) < 1e-12 and abs(d([-3, -4, 0], [-3, -4, 7]) - 5.0) < 1e-12
    assert abs(d([10, 10, 0], [10, 10, 1]) - np.sqrt(72.0)) < 1e-12


K_BOUND = 4 * 20384.0                       # test_sphere_cast.py's bound, unchanged: in units of 2^-24 * extent (/ |dir| for a time)


@pytest.mark.parametrize("name", ["viking_room", "example_object3"])
def test_reference_agrees_with_an_independent_float64_distance(name):
    """For every cast of 36 per radius (three axis lengths, unit directions) with a time t > 0, in float64 on the same fp32 inputs:
    at c(t) the reported triangle is r away from the axis and no triangle is nearer than r, within K * 2^-24 * extent — the bound
    of test_sphere_cast.py's float64 test, which carries over: a derived triangle's vertices cost one more rounding of a coordinate
    (2^-24 * extent each) against the thousands of units the grazing quadratics lose —; a time K * 2^-24 * extent / |dir| earlier
    and at four times spread over [0, t) no triangle is nearer than r within the same bound, so t is the FIRST contact (a hole in
    the derived surface would show here); and a cast with no time below T has no triangle nearer than r - bound at 6 times along
    its way, as far as its way was sampled.  A cast with t = 0 has a triangle within r + bound at the start."""
    a, b, c = positions(golden(name))
    ext = extent_of(a, b, c)
    tol = K_BOUND * 2.0 ** -24 * ext
    a64, b64, c64 = (x.astype(np.float64)[None] for x in (a, b, c))
    checked = sides = 0
    for j, radius in enumerate(RADII):
        casts = aimed_casts(a, b, c, 36, np.random.default_rng(200 + j), radii=(radius,), plain=True)
        t, tri, which, _ = CR.nearest(casts, a, b, c)
        o, d, h = (casts[k].astype(np.float64) for k in ("origin", "dir", "axis"))
        rr = casts["radius"].astype(np.float64)
        speed = np.linalg.norm(d, axis=1)

        def nearest_at(sel, time):
            p0 = o[sel] + d[sel] * time[:, None]
            return segment_triangle_distance(p0[:, None, :], (p0 + h[sel])[:, None, :], a64, b64, c64)

        hit = np.isfinite(t) & (t > 0)
        assert hit.sum() > 18
        t64 = t[hit].astype(np.float64)
        dist = nearest_at(hit, t64)
        own = dist[np.arange(hit.sum()), tri[hit]]
        worst_own, worst_near = np.abs(own - rr[hit]).max() / tol * K_BOUND, (rr[hit] - dist.min(axis=1)).max() / tol * K_BOUND
        print(f"{name}, r = {radius} * extent: {int(hit.sum())} contacts, worst |dist(axis, reported) - r| = {worst_own:.1f}, worst r - nearest "
              f"= {worst_near:.1f} (units of 2^-24 * extent); by derived triangle {np.bincount(which[hit], minlength=9).tolist()}")
        assert (np.abs(own - rr[hit]) <= tol).all()
        assert (dist.min(axis=1) >= rr[hit] - tol).all()
        for frac in (None, 0.0, 0.3, 0.6, 0.9):
            before = np.maximum(t64 - tol / speed[hit], 0.0) if frac is None else t64 * frac
            assert (nearest_at(hit, before).min(axis=1) >= rr[hit] - tol).all(), frac
        zero = np.isfinite(t) & (t == 0)
        if zero.any():
            assert (nearest_at(zero, np.zeros(zero.sum())).min(axis=1) <= rr[zero] + tol).all()
        miss = ~np.isfinite(t)
        for frac in np.linspace(0.0, 2.0, 6):
            if miss.any():
                reach = np.linalg.norm(o[miss] - np.concatenate([a, b, c]).mean(axis=0), axis=1) / speed[miss]
                assert (nearest_at(miss, reach * frac).min(axis=1) >= rr[miss] - tol).all()
        checked, sides = checked + int(hit.sum()), sides + int((which[hit] >= 2).sum())
    assert checked > 70 and sides > 8


@pytest.mark.parametrize("name", ["viking_room", "cfg1_4096"])
def test_the_accept_rule_rejects_next_to_nothing_on_the_parity_inputs(name):
    """Of all (cast, triangle) pairs with a time in [0, T), the share that misses its grown box or has t < entry is at most 1 %
    (test_sphere_cast.py's cap): the rule does not carry the parity tests.  Every pair of the first 300 parity casts is evaluated,
    with the Morton stage's boxes."""
    a, b, c = scene_positions(name)
    lo, hi = padded_boxes(a, b, c)
    casts = parity_casts(name, a, b, c)[:300]
    r = CR.reference(casts, a, b, c, lo, hi, casts_per_chunk=16, count_rule=True)
    print(f"{name}: {r.valid} pairs with a time, {r.rejected} rejected = {100.0 * r.rejected / max(r.valid, 1):.3f} %")
    assert r.valid > 1000 and r.rejected <= 0.01 * r.valid
    plain = CR.reference(casts, a, b, c, lo, hi)
    assert (words(plain.records) == words(r.records)).all() and (plain.flags == r.flags).all()


def test_shrunk_boxes_make_the_rule_reject():
    a, b, c = scene_positions("viking_room")
    lo, hi = padded_boxes(a, b, c)
    casts = parity_casts("viking_room", a, b, c)[:300]
    before = CR.reference(casts, a, b, c, lo, hi, casts_per_chunk=16, count_rule=True)
    picked = np.unique(before.records["tri"][before.flags == 1])[:40]
    centre, half = (lo[picked] + hi[picked]) * F(0.5), (hi[picked] - lo[picked]) * F(0.05)
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[picked], hi2[picked] = centre - half, centre + half
    after = CR.reference(casts, a, b, c, lo2, hi2, casts_per_chunk=16, count_rule=True)
    print(f"shrunk boxes: rejected {before.rejected} -> {after.rejected}")
    assert after.valid == before.valid and after.rejected > before.rejected
    assert (words(after.records) != words(before.records)).any()


def test_the_pierce_and_its_parameter_are_one_test():
    """triangle_query_reference.pierce gives no t; ray_reference.ray_triangle is the same arithmetic: pass iff 0 <= t <= 1"""
    a, b, c = scene_positions("cfg1_4096")
    rng = np.random.default_rng(4)
    k = rng.integers(0, len(a), 20000)
    w = rng.dirichlet((1, 1, 1), len(k))
    h = (rng.normal(size=(len(k), 3)) * 3.0).astype(F)
    o = (a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:] - h * rng.uniform(-0.5, 1.5, (len(k), 1))).astype(F)      # half go through
    t = RR.ray_triangle(o, h, a[k], (b - a)[k], (c - a)[k])[0]
    passes = TQ.pierce(o, h, a[k], (b - a)[k], (c - a)[k])
    with np.errstate(invalid="ignore"):
        assert passes.sum() > 5000 and (~passes).sum() > 5000 and (passes == ((F(0) <= t) & (t <= F(1)))).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Casts:
    """device buffers for one cast set and the two calls"""

    def __init__(self, ctx, drawer, casts):
        self.ctx, self.drawer, self.n = ctx, drawer, len(casts)
        self.casts = H().DataBuffer(ctx, self.n, L().CAPSULE_RAY)
        self.casts.local[:] = casts
        self.casts.sync()
        self.hits = H().DataBuffer(ctx, self.n + 1, L().HIT)
        self.flags = H().DataBuffer(ctx, self.n + 1, np.uint32)

    def cast(self):
        self.hits.fill_u32(0x7FC00000)
        self.drawer.capsule_cast(self.casts, self.hits)
        got = self.hits.get_data().copy()
        assert (words(got[self.n:]) == 0x7FC00000).all()
        return got[: self.n]

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.capsule_cast_any(self.casts, self.flags)
        got = self.flags.get_data().copy()
        assert got[self.n] == 0xDEADBEEF
        return got[: self.n]

    def dispose(self):
        for b in (self.casts, self.hits, self.flags):
            b.dispose()


def assert_records(got, ref, what=""):
    bad = np.nonzero((words(got).reshape(-1, 4) != words(ref.records).reshape(-1, 4)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], ref.records[bad[:3]], ref.which[bad[:10]])


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


def parity_case(ctx, name):
    """(positions, casts, reference, drawer): the reference is computed once per scene with the library's boxes; one context keeps
    one derived traversal scene, so the scene is derived again for the test that asks"""
    if name not in _CASES:
        a, b, c = scene_positions(name)
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        lo, hi = library_boxes(d)
        casts = parity_casts(name, a, b, c)
        _CASES[name] = ((a, b, c), casts, CR.reference(casts, a, b, c, lo, hi), d)
    _CASES[name][3].build_fast_scene()
    return _CASES[name]


SCENES = ["viking_room", "example_object3", "cfg1_4096", "grid_80x80"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_c1_records_and_flags_equal_the_brute_force_word_for_word(ctx, name):
    _, casts, ref, d = parity_case(ctx, name)
    got, flags = both(ctx, d, casts, ref, name)
    act = CR.active(casts)
    hit = ref.flags == 1
    by = np.bincount(ref.which[hit], minlength=9)
    print(f"{name}: {len(casts)} casts, {int(act.sum())} active, {int(hit.sum())} touch, {int((ref.records['t'][hit] == 0).sum())} at "
          f"t = 0, {int((ref.ties > 1).sum())} ties, by derived triangle {by.tolist()}")
    assert hit.sum() > 300 and (hit & (ref.records["t"] == 0)).sum() > 20 and (act & ~hit).sum() > 30 and (~act).sum() > 70
    assert by[0] > 50 and by[1] > 20 and by[2:8].sum() > 50
    assert (words(got[~act]).reshape(-1, 4) == MISS_WORDS).all() and (flags[~act] == 0).all()


@pytest.mark.gpu
def test_c2_the_known_answers_on_the_device(ctx):
    a, b, c = BIG
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    casts = _casts([[2, 2, 5], [2, 2, 8], [2, 2, 5], [2, -5, -0.75], [-5, 1, -0.75], [6, -5, 0.75], [2, 2, -3], [2, 2, 5]],
                   [[0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 1, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]], F(1.0),
                   [[0, 0, 3], [0, 0, -3], [2, 0, 0], [0, 0, 1.5], [0, 0, 1.5], [0, 0, -1.5], [0, 0, 8], [0, 0, 3]])
    ref = CR.reference(casts, a, b, c, *library_boxes(d))
    got, flags = both(ctx, d, casts, ref, "known answers")
    assert got["t"].tolist() == [4, 4, 4, 4, 4, 4, 0, S.MAX_FLOAT] and flags.tolist() == [1] * 7 + [0]
    assert got["u"].tolist() == [0.25, 0.25, 0.25, 0.25, 0, 0.75, 0.25, 0] and got["v"].tolist() == [0.25, 0.25, 0.25, 0, 0.125, 0, 0.25, 0]
    assert ref.which.tolist()[:5] == [0, 1, 0, 2, 7] and ref.which[6] == CR.PIERCE
    d.on_destroy()


def pair_casts(count, seed=3):
    a, b, c = BIG
    rng = np.random.default_rng(seed)
    casts = aimed_casts(a[:1], b[:1], c[:1], count, rng)
    casts["radius"] = rng.choice(np.array([0.05, 0.5, 2.0], dtype=F), count)
    return casts


@pytest.mark.gpu
def test_c3_two_triangles_and_small_counts(ctx):
    a, b, c = BIG
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    lo, hi = library_boxes(d)
    for count in (1, 63, 64, 65):
        casts = pair_casts(count, seed=count)
        casts["radius"][0], casts["t_max"][0], casts["axis"][0] = F(0.5), INF, (0, 0, 2)       # the first cast is a live one
        casts["origin"][0], casts["dir"][0] = (2, 2, 5), (0, 0, -1)
        ref = CR.reference(casts, a, b, c, lo, hi)
        got, _ = both(ctx, d, casts, ref, count)
        assert got["t"][0] == F(4.5) and got["tri"][0] == 0
    # runs of 64 or more inactive casts between active ones
    casts = pair_casts(400, seed=9)
    casts["radius"][50:130] = 0.0
    casts["axis"][200:270, 0] = np.nan
    ref = CR.reference(casts, a, b, c, lo, hi)
    act = CR.active(casts)
    assert not act[50:130].any() and not act[200:270].any() and ref.flags[:50].sum() > 5 and ref.flags[270:].sum() > 5
    got, _ = both(ctx, d, casts, ref, "inactive runs")
    assert (words(got[~act]).reshape(-1, 4) == MISS_WORDS).all()
    d.on_destroy()


@pytest.mark.gpu
def test_c4_a_contact_on_a_shared_edge_goes_to_the_lower_index(ctx):
    """two coplanar triangles sharing the edge (4, 0, 0) - (0, 4, 0), an upright capsule dropped on the middle of that edge: both
    have t = 4 exactly, index 0 wins in either order"""
    t0 = ([0, 0, 0], [4, 0, 0], [0, 4, 0])
    t1 = ([4, 0, 0], [4, 4, 0], [0, 4, 0])
    casts = _casts([[2, 2, 5]] * 3, [[0, 0, -1]] * 3, F(1.0), [[0, 0, 2]] * 3, np.array([np.inf, 4.0, 4.5], dtype=F))
    for order in ((t0, t1), (t1, t0)):
        a, b, c = (np.array([t[k] for t in order], dtype=F) for k in range(3))
        d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
        ref = CR.reference(casts, a, b, c, *library_boxes(d))
        assert ref.ties.tolist() == [2, 0, 2] and ref.records["tri"].tolist() == [0, 0, 0] and ref.records["t"].tolist()[::2] == [4.0, 4.0]
        _, flags = both(ctx, d, casts, ref, "shared edge")
        assert flags.tolist() == [1, 0, 1]
        d.on_destroy()


@pytest.mark.gpu
def test_c5_order_independence_under_a_shuffle_of_the_triangles(ctx):
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
    for k in ("u", "v"):                                                         # the same triangle, the same contact point
        assert (words(got[k][unique]) == words(ref.records[k][unique])).all()


@pytest.mark.gpu
def test_c6_device_stack_and_a_capsule_beyond_the_scene(ctx):
    (a, b, c), casts, ref, d = parity_case(ctx, "viking_room")
    h, lib = ctx.handle, N().lib
    ext = extent_of(a, b, c)
    centre = np.concatenate([a, b, c]).mean(axis=0)
    rng = np.random.default_rng(1)
    big = CR.make_casts(np.tile(centre, (70, 1)).astype(F), rng.normal(size=(70, 3)).astype(F), F(3.0 * ext),
                        (rng.normal(size=(70, 3)) * 3.0 * ext).astype(F))
    rb = CR.reference(big, a, b, c, *library_boxes(d))
    try:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))                       # all but one entry in device memory
        both(ctx, d, casts, ref, "stack split 1")
        got, flags = both(ctx, d, big, rb, "a radius and an axis beyond the scene, stack split 1")
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert (got["t"] == 0).all() and (got["tri"] == 0).all() and (flags == 1).all()
    both(ctx, d, big, rb, "a radius and an axis beyond the scene")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_c7_lane_refill_under_a_wave_cap(ctx, waves):
    """1 500 casts on 1, 2, 3 or 7 waves: runs of 215 .. 1 500 casts, every lane refilled many times"""
    _, casts, ref, d = parity_case(ctx, "viking_room")
    assert len(casts) == 1500
    h, lib = ctx.handle, N().lib
    try:
        N().check(h, lib.lbvh_debug_ray_waves(h, waves))
        both(ctx, d, casts, ref, f"{waves} waves")
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))


@pytest.mark.gpu
def test_c8_statistics_count_the_active_casts(ctx):
    _, casts, ref, d = parity_case(ctx, "viking_room")
    q = Casts(ctx, d, casts)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    per = {}
    try:
        for name, call in (("cast", q.cast), ("any", q.any)):
            stats.fill_u32(0)
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
            got = call()
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
            s = stats.get_data()[0]
            per[name] = (int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"]))
            assert (words(got) == words(ref.records if name == "cast" else ref.flags)).all()          # the counting kernels: same answers
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    print("casts, node lines, triangle lines:", per)
    n_active = int(CR.active(casts).sum())
    assert per["cast"][0] == n_active and per["any"][0] == n_active
    assert per["any"][1] <= per["cast"][1] and per["any"][2] <= per["cast"][2] and per["cast"][1] >= n_active
    stats.dispose()
    q.dispose()


@pytest.mark.gpu
def test_c9_errors_the_stale_scene_the_stack_limit_and_the_live_path_list(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        casts = aimed_casts(a, b, c, 600, np.random.default_rng(2))
        ref = CR.reference(casts, a, b, c, *library_boxes(d))
        assert 100 < ref.flags.sum() < 600
        q = Casts(c2, d, casts)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(casts)
        p = lambda buf, k: C.c_void_p(buf.device.value + k)
        # what lbvh_trace_rays answers before any cast: the live-path list it leaves behind is dropped by the casts below
        st = np.zeros(n, dtype=L().PATH_STATE)
        st["origin"], st["dir"], st["alive"] = casts["origin"], np.where(np.isfinite(casts["dir"]), casts["dir"], 1.0), 1
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
        assert lib.lbvh_capsule_cast(h, q.casts.device, n, C.byref(s), q.hits.device) == -2
        assert untouched()
        expected_path = trace_rays()
        assert_records(q.cast(), ref, "after the failed reservation")
        assert (trace_rays() == expected_path).all()                                  # the list was dropped and made again
        assert (q.any() == ref.flags).all()
        assert (trace_rays() == expected_path).all()
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        for fn, out, off in ((lib.lbvh_capsule_cast, q.hits, 8), (lib.lbvh_capsule_cast_any, q.flags, 2)):
            assert fn(h, None, n, C.byref(s), out.device) == -1
            assert fn(h, q.casts.device, n, None, out.device) == -1
            assert fn(h, q.casts.device, n, C.byref(s), None) == -1
            assert fn(h, p(q.casts, 4), 10, C.byref(s), out.device) == -1
            assert fn(h, q.casts.device, 10, C.byref(s), p(out, off)) == -1
            assert fn(h, q.casts.device, 1 << 32, C.byref(s), out.device) == -1
            assert fn(None, q.casts.device, 10, C.byref(s), out.device) == -1
            assert fn(h, q.casts.device, 0, C.byref(s), out.device) == 0              # count == 0: a no-op
        assert untouched()
        # aligned sub-ranges are accepted: casts 1 .. 10 into records from record 1
        assert lib.lbvh_capsule_cast(h, p(q.casts, 48), 10, C.byref(s), p(q.hits, 16)) == 0
        assert (words(q.hits.get_data()[1:11]) == words(ref.records[1:11])).all()
        # a stale scene: triangles uploaded without a rebuild; the message names the entry point
        d.container.triangle_data.sync()
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        assert lib.lbvh_capsule_cast(h, q.casts.device, n, C.byref(s), q.hits.device) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_capsule_cast: ") and b"stale" in msg, msg
        assert lib.lbvh_capsule_cast_any(h, q.casts.device, n, C.byref(s), q.flags.device) == -1
        assert lib.lbvh_last_error(h).startswith(b"lbvh_capsule_cast_any: ")
        assert untouched()
        d.rebuild(fast=True)
        # the stack limit: a reported error (LBVH_ERR_HIP at the next sync), never a silently wrong record
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        q.drawer.capsule_cast(q.casts, q.hits)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_records(q.cast(), ref, "after the stack limit")
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_c10_path_tracer_frame_undisturbed_by_a_cast_between_bounces(ctx):
    """the casts drop the live-path list: the next lbvh_path_bounce scans again and the frame is the one without them"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    a, b, c = positions(tris)
    big = aimed_casts(a, b, c, 4 * 160 * 96, np.random.default_rng(12), radii=(0.005,))      # 4x the frame: the scratch grows in mid-frame
    q = Casts(ctx, pt.drawer, big)
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def cast():
        pt.drawer.capsule_cast(q.casts, q.hits)
        pt.drawer.capsule_cast_any(q.casts, q.flags)

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
    assert 0 < f.sum() < q.n and ((q.hits.get_data()[: q.n]["t"] < S.MAX_FLOAT) == (f == 1)).all()
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), (7, 0.5, 12.0)])
def test_c11_cpp_host_driver_capsule_matches_the_python_host(ctx, args):
    """`lbvh_driver capsule` on the driver's own random mesh (default and given seed, radius, height) against the Python host on the
    same triangles and the same casts"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 6000
    res = json.loads(subprocess.run([exe, "capsule", str(count)] + [str(x) for x in args], check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(4096)
    casts = CR.driver_casts(lo, hi, count, *args)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Casts(ctx, d, casts)
    got, flags = q.cast(), q.any()
    q.dispose()
    d.on_destroy()
    assert res["triangles"] == len(tris) and res["casts"] == count and F(res["radius"]) == casts["radius"][0]
    assert res["touching"] == int((got["t"] < S.MAX_FLOAT).sum()) == res["flagged"] == int(flags.sum())
    assert res["at_start"] == int((got["t"] == 0).sum())
    assert res["word_sum"] == int(words(got).astype(np.uint64).sum())
    assert [r[1] for r in res["records"]] == got["tri"][:3].tolist()
    assert [words(np.array(r[0], dtype=F))[0] for r in res["records"]] == words(got["t"][:3]).tolist()
    assert 0 < res["touching"] < count
