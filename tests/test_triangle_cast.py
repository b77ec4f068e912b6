"""lbvh_triangle_cast / lbvh_triangle_cast_any: where a moving triangle first hits the mesh, over the four-wide derived traversal
scene.  The expectation is tests/triangle_cast_reference.py: the header's definition in numpy float32, brute force over every
(cast, triangle) pair with the boxes the library produced.  Every GPU comparison is word for word on uint32 views, no tolerance.
The restatement itself is checked against float64 geometry that shares no line with it."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hostile_scenes as HS
import ray_reference as RR
import triangle_cast_reference as TR
import triangle_query_reference as TQ
from query_support import driver_mesh, H, L, library_boxes, make_rays, N, pack, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
SIZES = (0.005, 0.02, 0.1)                  # edge lengths of the query triangles, of the scene's extent
MISS_WORDS = words(np.array([TR.MISS]))
START = 16                                  # LBVH_TRI_CAST_START


def extent_of(a, b, c):
    pts = np.concatenate([a, b, c])
    return float((pts.max(axis=0) - pts.min(axis=0)).max())


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def test_header_declares_both_structs_and_both_prototypes_and_keeps_the_abi_version():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    m = re.search(r"typedef struct lbvh_tri_ray \{(.*?)\} lbvh_tri_ray;", h, re.S)
    assert m and re.findall(r"(?:float|uint32_t)\s+(\w+)", m.group(1)) == ["a", "skip", "b", "t_max", "c", "_pad0", "dir", "_pad1"]
    m = re.search(r"typedef struct lbvh_tri_cast_hit \{(.*?)\} lbvh_tri_cast_hit;", h, re.S)
    assert m and re.findall(r"(?:float|uint32_t)\s+(\w+)", m.group(1)) == ["t", "tri", "feature", "w"]
    for fn, out in (("lbvh_triangle_cast", r"lbvh_tri_cast_hit\* d_hits"), ("lbvh_triangle_cast_any", r"uint32_t\* d_flags")):
        assert re.search(r"lbvh_status " + fn + r"\(lbvh_context\* ctx, const lbvh_tri_ray\* d_casts, size_t count, "
                         r"const lbvh_scene\* h_scene,\s+" + out + r"\);", h), fn
    assert re.search(r"#define LBVH_ABI_VERSION 11\b", h)                  # purely additive
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_triangle_cast," in bounce and "lbvh_triangle_cast_any" in bounce
    assert "pierce_quad" in h and "lbvh_triangle_cast_all) is out of scope" in h


def test_layout_signatures_csharp_and_cpp_host():
    lay, nat = L(), N()
    assert lay.TRI_RAY.itemsize == 64 and lay.TRI_CAST_HIT.itemsize == 16 and lay.TRI_CAST_START == START
    assert [lay.TRI_RAY.fields[k][1] for k in ("a", "skip", "b", "t_max", "c", "_pad0", "dir", "_pad1")] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert [lay.TRI_CAST_HIT.fields[k][1] for k in ("t", "tri", "feature", "w")] == [0, 4, 8, 12]
    assert lay.TRI_RAY is TR.TRI_RAY
    for fn in ("lbvh_triangle_cast", "lbvh_triangle_cast_any"):
        res, args = nat.SIGNATURES[fn]
        assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
        assert getattr(nat.lib, fn).argtypes is not None
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    m = re.search(r"public struct TriRay \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["aX", "aY", "aZ", "skip", "bX", "bY", "bZ", "tMax", "cX", "cY", "cZ", "pad0",
                                                                 "dirX", "dirY", "dirZ", "pad1"]
    m = re.search(r"public struct TriCastHit \{(.*?)\}", cs, re.S)
    assert m and re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == ["t", "tri", "feature", "w"]
    for fn in ("lbvh_triangle_cast", "lbvh_triangle_cast_any"):
        assert re.search(r"public static extern int " + fn + r"\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+\);", cs)
    cc = open(os.path.join(ROOT, "bindings", "csharp", "TriangleCasts.cs")).read()
    assert "lbvh_triangle_cast(" in cc and "lbvh_triangle_cast_any(" in cc and "unsafe" not in cc and "stride != 64" in cc
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void TriangleCast(" in hpp and "void TriangleCastAny(" in hpp
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, k) for k in ("triangle_cast", "triangle_cast_any", "mesh_sweep"))
    assert all(hasattr(H(), k) for k in ("tri_casts", "tri_casts_from_mesh", "triangle_cast_contact"))
    assert "tricast_main" in open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()


def test_builders():
    q = H().tri_casts([0, 0, 1], [[1, 0, 1], [2, 0, 1]], [0, 1, 1], [0, 0, -1], t_max=3.0)
    assert q.dtype == L().TRI_RAY and q.shape == (2,) and q["b"].tolist() == [[1, 0, 1], [2, 0, 1]] and (q["skip"] == L().NULL).all()
    assert (q["t_max"] == 3).all() and q["dir"].tolist() == [[0, 0, -1]] * 2
    tris = scenes.random_triangles(5, seed=3)
    m = H().tri_casts_from_mesh(tris, [1, 2, 3], skip_self=True)
    assert m["skip"].tolist() == [0, 1, 2, 3, 4] and (m["c"] == tris["c"][:, :3]).all() and np.isinf(m["t_max"]).all()
    assert (H().tri_casts_from_mesh(positions(tris), [1, 2, 3])["skip"] == L().NULL).all()


# ---- CPU: known answers of the restatement, exact in fp32 ---------------------------------------------------------------

BIG = (np.array([[0, 0, 0], [500, 500, 500]], dtype=F), np.array([[8, 0, 0], [501, 500, 500]], dtype=F),
       np.array([[0, 8, 0], [500, 501, 500]], dtype=F))        # one big triangle in z = 0 and a far dummy (scenes need n >= 2)
TILT = (np.array([[0, 0, 0], [500, 500, 500]], dtype=F), np.array([[8, 0, 0], [501, 500, 500]], dtype=F),
        np.array([[4, 4, 3], [500, 501, 500]], dtype=F))       # tilted: the top vertex c = v0 + e2 is alone at z = 3
T_EDGE = F(6)
EDGE_NORMAL = [0.0, -1 / 5 ** 0.5, 2 / 5 ** 0.5]      # at right angles to both edges (0, 4, 2) and (8, 0, 0), against dir = -z
# (scene, a, b, c, dir, t_max, skip, expected (t, feature, w) or None for the miss record, contact point, normal)
KNOWN = [
    # one lowest vertex, dropped from height 5: that vertex onto the face
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], INF, TR.NULL, (5.0, 0, 0.0), [2, 2, 0], [0, 0, 1]),
    (BIG, [3, 2, 6], [2, 2, 5], [2, 3, 6], [0, 0, -1], INF, TR.NULL, (5.0, 1, 0.0), [2, 2, 0], [0, 0, 1]),
    (BIG, [3, 2, 6], [2, 3, 6], [2, 2, 5], [0, 0, -2], INF, TR.NULL, (2.5, 2, 0.0), [2, 2, 0], [0, 0, 1]),
    # the query edge ab crosses over the line of the scene edge ab (y = 0) at x = 3, 6 above it; its ends miss the face (a) or come
    # later (b): moving edge 0 against scene edge 0 at 3 / 8 of it
    (BIG, [3, -2, 5], [3, 2, 7], [3, 0, 12], [0, 0, -1], INF, TR.NULL, (6.0, 6, 0.375), [3, 0, 0], EDGE_NORMAL),
    # the same edge as the query's bc and ca: moving edges 1 and 2
    (BIG, [3, 0, 12], [3, -2, 5], [3, 2, 7], [0, 0, -1], INF, TR.NULL, (6.0, 9, 0.375), [3, 0, 0], EDGE_NORMAL),
    (BIG, [3, 2, 7], [3, 0, 12], [3, -2, 5], [0, 0, -1], INF, TR.NULL, (6.0, 12, 0.375), [3, 0, 0], EDGE_NORMAL),
    # a large horizontal triangle lowered onto the tilted triangle: the scene's top vertex v0 + e2 onto the moving face
    (TILT, [-20, -20, 8], [30, -20, 8], [-20, 30, 8], [0, 0, -1], INF, TR.NULL, (5.0, 5, 0.0), [4, 4, 3], [0, 0, 1]),
    # piercing the face at the start, whatever the direction
    (BIG, [2, 2, -1], [2, 2, 1], [3, 2, 1], [1, 0, 0], INF, TR.NULL, (0.0, START | 0, 0.0), None, None),
    (BIG, [2, 2, -1], [2, 2, 1], [3, 2, 1], [0, 0, 1], INF, TR.NULL, (0.0, START | 0, 0.0), None, None),
    (BIG, [2, 2, -1], [2, 2, 1], [3, 2, 1], [0, -3, -1], F(1e-30), TR.NULL, (0.0, START | 0, 0.0), None, None),
    # moving away
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, 1], INF, TR.NULL, None, None, None),
    # the strict bound: t_max just below the contact time, at it, just above it
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], np.nextafter(F(5), F(0)), TR.NULL, None, None, None),
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], F(5), TR.NULL, None, None, None),
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], np.nextafter(F(5), INF), TR.NULL, (5.0, 0, 0.0), [2, 2, 0], [0, 0, 1]),
    # skip equal to the only candidate
    (BIG, [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], INF, 0, None, None, None),
]


def _casts(rows):
    """rows of (a, b, c, dir, t_max, skip)"""
    col = lambda k: np.array([r[k] for r in rows], dtype=F).reshape(-1, 3)
    return TR.make_casts(col(0), col(1), col(2), col(3), np.array([r[4] for r in rows], dtype=F), np.array([r[5] for r in rows], dtype=np.uint32))


def _known(scene):
    rows = [k for k in KNOWN if k[0] is scene]
    expected = [(float(L().MAX_FLOAT), 0, 0, 0.0) if k[7] is None else (k[7][0], 0, k[7][1], k[7][2]) for k in rows]
    return _casts([k[1:7] for k in rows]), expected, rows


def _tuples(records):
    return [(float(r["t"]), int(r["tri"]), int(r["feature"]), float(r["w"])) for r in records]


def _check_contacts(casts, records, scene, rows):
    point, normal = H().triangle_cast_contact(casts, records, scene)
    for i, k in enumerate(rows):
        if k[8] is None:
            assert np.isnan(point[i]).all() and np.isnan(normal[i]).all()
        else:
            assert point[i].tolist() == k[8] and np.allclose(normal[i], k[9], rtol=0, atol=1e-15), (i, point[i], normal[i])


@pytest.mark.parametrize("scene", [BIG, TILT], ids=["big", "tilt"])
def test_known_answers_on_one_triangle(scene):
    casts, expected, rows = _known(scene)
    a, b, c = scene
    r = TR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert _tuples(r.records) == expected
    assert r.flags.tolist() == [int(e[0] < L().MAX_FLOAT) for e in expected]
    assert not np.signbit(r.records["t"]).any() and not np.signbit(r.records["w"]).any()
    _check_contacts(casts, r.records, scene, rows)


def inactive_forms():
    a, b, c, d = [2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1]
    nan, inf = np.nan, np.inf
    rows = [(a, b, c, d, t, TR.NULL) for t in (0.0, -1.0, nan, -inf)]
    for bad in (nan, inf, -inf):
        for v in range(3):
            for k in range(3):
                tri = [list(a), list(b), list(c)]
                tri[v][k] = bad
                rows.append((tri[0], tri[1], tri[2], d, INF, TR.NULL))
        for k in range(3):
            dd = list(d)
            dd[k] = bad
            rows.append((a, b, c, dd, INF, TR.NULL))
    rows += [(a, b, c, [0, 0, 0], INF, TR.NULL), (a, b, c, [0, 0, -1e-30], INF, TR.NULL)]       # dot(dir, dir) = 0 (underflow)
    return _casts(rows)


def test_every_inactive_form_is_a_miss_record():
    casts = inactive_forms()
    assert len(casts) == 4 + 3 * 12 + 2 and not TR.active(casts).any()
    a, b, c = BIG
    r = TR.reference(casts, a, b, c, *padded_boxes(a, b, c))
    assert (r.flags == 0).all() and (words(r.records).reshape(-1, 4) == MISS_WORDS).all()
    live = _casts([([2, 2, 5], [3, 2, 6], [2, 3, 6], [0, 0, -1], 1e-30, TR.NULL), ([2, 2, 5], [2, 2, 5], [2, 2, 5], [0, 0, -1e-10], INF, 7)])
    assert TR.active(live).all()


def test_three_rays_from_the_vertices_miss_the_edge_contact():
    """the workaround is wrong: the edge-over-edge case answered by lbvh_trace_closest's restatement from the three vertices gives a
    strictly later time"""
    a, b, c = BIG
    lo, hi = padded_boxes(a, b, c)
    row = KNOWN[3]
    cast = _casts([row[1:7]])
    assert TR.reference(cast, a, b, c, lo, hi).records["t"][0] == T_EDGE
    rays = make_rays(np.array(row[1:4], dtype=F), np.array([row[4]] * 3, dtype=F), F(0), INF)
    t = RR.reference(rays, a, b, c, lo, hi).records["t"]
    assert t.tolist() == [float(L().MAX_FLOAT), 7.0, 12.0] and t.min() > T_EDGE


# ---- cast sets ----------------------------------------------------------------------------------------------------------

def soup64():
    return positions(scenes.random_triangles(64, seed=21, extent=10.0, edge=4.0))


def mean_edge(a, b, c):
    return float(np.mean([np.linalg.norm(b - a, axis=1), np.linalg.norm(c - b, axis=1), np.linalg.norm(a - c, axis=1)]))


def aimed_casts(a, b, c, count, rng, edges, plain=False):
    """Triangles that start outside the mesh's box and aim at points of its surface; `edges` = the lengths of b - a and c - a in
    turn (random directions).  plain: unit directions, t_max = +inf, no skip, active casts only (the float64 comparison).
    Otherwise: 15 % axis-aligned directions, 40 % non-unit, half with a finite t_max around the contact, 10 % starting on the
    surface (intersecting at the start), 20 % with skip = the triangle aimed at (as in a self-pass), and inactive forms."""
    pts = np.concatenate([a, b, c])
    k = rng.integers(0, len(a), count)
    w = rng.dirichlet((1, 1, 1), count)
    target = a[k] * w[:, :1] + b[k] * w[:, 1:2] + c[k] * w[:, 2:]
    d = rng.normal(size=(count, 3))
    if not plain:
        along = rng.random(count) < 0.15
        d[along] = np.eye(3)[rng.integers(0, 3, along.sum())] * rng.choice([-1.0, 1.0], along.sum())[:, None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    size = np.asarray(edges, dtype=float)[np.arange(count) % len(edges)]
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    h1 = unit(rng.normal(size=(count, 3))) * (size * rng.uniform(0.7, 1.0, count))[:, None]
    h2 = unit(rng.normal(size=(count, 3))) * (size * rng.uniform(0.7, 1.0, count))[:, None]
    reach = 1.25 * np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)) + 2.0 * size.max()
    centre = target - d * reach
    t_max = np.full(count, INF, dtype=F)
    skip = np.full(count, TR.NULL, dtype=np.uint32)
    if not plain:
        scale = np.where(rng.random(count) < 0.4, rng.uniform(0.25, 4.0, count), 1.0)
        d = d * scale[:, None]
        finite = rng.random(count) < 0.5
        t_max[finite] = (reach / scale * rng.uniform(0.6, 1.3, count))[finite]
        inside = rng.random(count) < 0.1
        centre[inside] = target[inside]
        own = rng.random(count) < 0.2
        skip[own] = k[own]
    qa = centre - (h1 + h2) / 3.0
    casts = TR.make_casts(qa.astype(F), (qa + h1).astype(F), (qa + h2).astype(F), d.astype(F), t_max, skip)
    if not plain:
        dead = rng.random(count) < 0.08
        form = rng.integers(0, 6, count)
        casts["t_max"][dead & (form == 0)] = 0.0
        casts["t_max"][dead & (form == 1)] = np.nan
        casts["dir"][dead & (form == 2)] = 0.0
        casts["a"][dead & (form == 3), 1] = np.nan
        casts["c"][dead & (form == 4), 2] = np.inf
        casts["dir"][dead & (form == 5), 0] = -np.inf
    return casts


def scene_positions(name):
    if name == "big":
        return BIG
    if name == "soup64":
        return soup64()
    if name == "grid_80x80":
        return positions(scenes.grid_scene())
    if name == "driver":
        pos = driver_mesh(4096)[1]
        return tuple(np.ascontiguousarray(pos[:, k], dtype=F) for k in range(3))
    return positions(HS.scene(name))


def parity_casts(name, a, b, c, count=130):
    ext = extent_of(a[:1], b[:1], c[:1]) if name == "big" else extent_of(a, b, c)
    x = (a[:1], b[:1], c[:1]) if name == "big" else (a, b, c)
    return aimed_casts(*x, count, np.random.default_rng(17 + len(a) + count), [s * ext for s in SIZES])


# ---- CPU: the restatement against float64 geometry that shares no code with it ---------------------------------------------

def _tri_tri_touch(p, q):
    """float64, signed volumes only: p (3, 3) against q (m, 3, 3) -> bool (m,): some edge of one crosses the other (closed)"""
    vol = lambda a, b, c, d: np.einsum("...i,...i", np.cross(b - a, c - a), d - a)
    out = np.zeros(len(q), dtype=bool)
    p = np.broadcast_to(p, q.shape)
    for s, t in ((p, q), (q, p)):
        for i in range(3):
            x, y = s[:, i], s[:, (i + 1) % 3]
            d1, d2 = vol(t[:, 0], t[:, 1], t[:, 2], x), vol(t[:, 0], t[:, 1], t[:, 2], y)
            s0, s1, s2 = vol(x, y, t[:, 0], t[:, 1]), vol(x, y, t[:, 1], t[:, 2]), vol(x, y, t[:, 2], t[:, 0])
            inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
            out |= (d1 * d2 <= 0) & ((d1 != 0) | (d2 != 0)) & inside
    return out


def test_the_independent_geometry_knows_its_own_answers():
    q = np.array([[[0, 0, 0], [8, 0, 0], [0, 8, 0]]], dtype=float)
    at = lambda z: np.array([[2, 2, z], [3, 2, z + 1], [2, 3, z + 1]], dtype=float)
    assert not _tri_tri_touch(at(1e-9), q)[0] and _tri_tri_touch(at(-1e-9), q)[0] and not _tri_tri_touch(at(-2), q)[0]
    edge = lambda z: np.array([[3, -2, z - 1], [3, 2, z + 1], [3, 0, z + 6]], dtype=float)
    assert not _tri_tri_touch(edge(1e-9), q)[0] and _tri_tri_touch(edge(-1e-9), q)[0]


K_BOUND = 20.0


def float64_check(name, count=2000):
    """The restatement's records against float64 geometry, per record with a time t > 0 (the winning feature's own solve, and a
    feature-free triangle-triangle test against the whole mesh just before and just after t).

    The bound, in time: K * 2^-24 * scale / (conditioning * |D|) with, for the winning test pierce(P, D; V, E1, E2),
    conditioning = |det| / (|D| |E1| |E2|) and scale = |P - V| + t |D|.  K from pierce's operations, each rounding 2^-24 relative:
    the numerator dot(E2, cross(P - V, E1)) carries 1 (the subtraction) + 3 (a cross component: two products, one difference) + 3
    (the dot: three products, two sums) = 7 roundings of size |P - V| |E1| |E2|; det = dot(E1, cross(D, E2)) carries 3 + 3 = 6 of size
    |D| |E1| |E2|, which enter t = numerator / det multiplied by t; 1 / det and the last product 2 more; E1 and E2 are themselves
    fp32 differences of the vertices the float64 side starts from, each one rounding in the numerator and in det: 4.  7 + 6 + 2 +
    4 = 19, taken as K = 20.  Nothing here was fitted to an output.
    Left out: records whose winning test has |det| < 1e-3 |D| |E1| |E2| (the issue's allowance); the cap of 2 % is asserted.
    Counted on the CPU: grid_80x80 0 of 2 000 records with a time left out (0 %), worst |t64 - t| 0.047 of the bound; soup64 0 of
    2 000 (0 %), worst 0.106 of the bound."""
    a, b, c = scene_positions(name)
    me = mean_edge(a, b, c)
    rng = np.random.default_rng(500 + len(a))
    casts = aimed_casts(a, b, c, count, rng, rng.uniform(0.5 * me, 2.0 * me, 97), plain=True)
    lo, hi = padded_boxes(a, b, c)
    ref = TR.reference(casts, a, b, c, lo, hi)
    e1, e2 = b - a, c - a
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    scene = np.stack([f8(a), f8(b), f8(c)], axis=1)
    blo, bhi = scene.min(axis=1), scene.max(axis=1)
    timed = np.nonzero((ref.flags == 1) & (ref.records["t"] > 0))[0]
    tri = ref.records["tri"][timed].astype(np.int64)
    _, feat, _, det, scale3 = TR.pair_time(casts["a"][timed], casts["b"][timed], casts["c"][timed], casts["dir"][timed], a[tri], e1[tri], e2[tri],
                                           np.zeros(len(timed), dtype=bool), with_det=True)
    assert (feat == ref.records["feature"][timed]).all()
    left_out = checked = 0
    worst = 0.0
    by_kind = [0, 0, 0]
    for n, i in enumerate(timed):
        cond = abs(det[n]) / scale3[n]
        if cond < 1e-3:
            left_out += 1
            continue
        q = casts[i]
        t, w, f = float(ref.records["t"][i]), float(ref.records["w"][i]), int(feat[n])
        qa, qb, qc, d = f8(q["a"]), f8(q["b"]), f8(q["c"]), f8(q["dir"])
        sv = scene[tri[n]]
        speed = np.linalg.norm(d)
        moving = np.stack([qa, qb, qc])
        if f < 6:                                                    # a vertex onto a face: the plane, then barycentrics from areas
            x, dd, face = (moving[f], d, sv) if f < 3 else (sv[f - 3], -d, moving)
            nrm = np.cross(face[1] - face[0], face[2] - face[0])
            t64 = np.dot(face[0] - x, nrm) / np.dot(dd, nrm)
            p = x + dd * t64
            areas = np.array([np.dot(np.cross(face[(j + 1) % 3] - p, face[(j + 2) % 3] - p), nrm) for j in range(3)]) / np.dot(nrm, nrm)
            reach = np.linalg.norm(x - face[0]) + t * speed
            # a point off by the bound (as a distance) moves a barycentric by at most that over the face's least altitude
            longest = max(np.linalg.norm(face[(j + 1) % 3] - face[j]) for j in range(3))
            inside = areas.min() >= -(K_BOUND * 2.0 ** -24 * reach / cond) * longest / np.linalg.norm(nrm)
            off = 0.0
        else:                                                        # an edge onto an edge: P + E s + d t = Q + F u
            m, e = (f - 6) // 3, (f - 6) % 3
            pp, ee = moving[m], moving[(m + 1) % 3] - moving[m]
            qq, ff = (sv[0], sv[1] - sv[0]) if e == 0 else (sv[0], sv[2] - sv[0]) if e == 1 else (sv[1], sv[2] - sv[1])
            s64, t64, u64 = np.linalg.solve(np.stack([ee, d, -ff], axis=1), qq - pp)
            reach = np.linalg.norm(pp - qq) + t * speed
            slack = K_BOUND * 2.0 ** -24 * reach / cond
            inside = -slack / np.linalg.norm(ee) <= s64 <= 1 + slack / np.linalg.norm(ee) and -slack / np.linalg.norm(ff) <= u64 <= 1 + slack / np.linalg.norm(ff)
            off = abs(u64 - w) * np.linalg.norm(ff)
        bound = K_BOUND * 2.0 ** -24 * reach / (cond * speed)
        worst = max(worst, abs(t64 - t) / bound, off / (bound * speed))
        assert inside, (name, i, f, "the winning feature's point is outside its triangle or edge")
        assert abs(t64 - t) <= bound and off <= bound * speed, (name, i, f, t, t64, abs(t64 - t) / bound, off / (bound * speed))
        # feature-free: apart just before, touching just after, in float64
        delta = 2.0 * bound
        for time, want in ((t - delta, False), (t + delta, True)):
            now = moving + d * time
            near = ((blo <= now.max(axis=0) + 1e-9) & (bhi >= now.min(axis=0) - 1e-9)).all(axis=1)
            near[tri[n]] = True
            idx = np.nonzero(near)[0]
            touch = _tri_tri_touch(now, scene[idx])
            if want:
                assert touch.any(), (name, i, f, "touching nothing just after t")     # the mesh, not the reported triangle: by then
                #                                                                        the contact may have slid onto a neighbour
            else:
                assert not touch.any(), (name, i, f, "touching", idx[touch], "just before t")
        checked += 1
        by_kind[0 if f < 3 else 1 if f < 6 else 2] += 1
    # casts with no time: apart from everything at six times along their way
    for i in np.nonzero(ref.flags == 0)[0][:100]:
        q = casts[i]
        moving, d = np.stack([f8(q["a"]), f8(q["b"]), f8(q["c"])]), f8(q["dir"])
        way = 2.0 * np.linalg.norm(scene.reshape(-1, 3).mean(axis=0) - moving[0]) / np.linalg.norm(d)
        for time in np.linspace(0.0, way, 6):
            now = moving + d * time
            near = ((blo <= now.max(axis=0)) & (bhi >= now.min(axis=0))).all(axis=1)
            assert not _tri_tri_touch(now, scene[near]).any(), (name, i, time, "a cast with no time touches")
    print(f"{name}: {count} casts, {len(timed)} with a time > 0, {checked} checked (vertex/face {by_kind[0]}, face/vertex {by_kind[1]}, "
          f"edge/edge {by_kind[2]}), {left_out} left out = {100.0 * left_out / max(len(timed), 1):.2f} %, worst share of the bound {worst:.3f}")
    return len(timed), checked, left_out, by_kind


@pytest.mark.parametrize("name", ["grid_80x80", "soup64"])
def test_reference_agrees_with_independent_float64_geometry(name):
    timed, checked, left_out, by_kind = float64_check(name)
    assert timed > 1000 and left_out <= 0.02 * timed and checked == timed - left_out
    assert by_kind[0] > 100 and (name == "grid_80x80" or (by_kind[1] > 20 and by_kind[2] > 100))


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Casts:
    """device buffers for one cast set and the two calls"""

    def __init__(self, ctx, drawer, casts):
        self.ctx, self.drawer, self.n = ctx, drawer, len(casts)
        self.casts = H().DataBuffer(ctx, self.n, L().TRI_RAY)
        self.casts.local[:] = casts
        self.casts.sync()
        self.hits = H().DataBuffer(ctx, self.n + 1, L().TRI_CAST_HIT)
        self.flags = H().DataBuffer(ctx, self.n + 1, np.uint32)

    def cast(self):
        self.hits.fill_u32(0x7FC00000)
        self.drawer.triangle_cast(self.casts, self.hits)
        got = self.hits.get_data().copy()
        assert (words(got[self.n:]) == 0x7FC00000).all()
        return got[: self.n]

    def any(self):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.triangle_cast_any(self.casts, self.flags)
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


def scene_case(ctx, name, count=130):
    """-> (positions, casts, reference with the library's boxes, drawer); the caller destroys the drawer"""
    a, b, c = scene_positions(name)
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    casts = parity_casts(name, a, b, c, count)
    return (a, b, c), casts, TR.reference(casts, a, b, c, *library_boxes(d)), d


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big", "soup64", "grid_80x80", "driver"])
def test_t1_records_and_flags_equal_the_brute_force_word_for_word(ctx, name):
    """130 casts per call: three waves, the last partial; sizes of 0.5 / 2 / 10 % of the extent, inactive forms and `skip` mixed in"""
    _, casts, ref, d = scene_case(ctx, name)
    try:
        got, flags = both(ctx, d, casts, ref, name)
    finally:
        d.on_destroy()
    act = TR.active(casts)
    hit = ref.flags == 1
    by = np.bincount(ref.records["feature"][hit], minlength=22)
    print(f"{name}: {len(casts)} casts, {int(act.sum())} active, {int(hit.sum())} touch, {int((casts['skip'] != TR.NULL).sum())} with skip, by feature {by.tolist()}")
    assert len(casts) == 130 and 0 < (~act).sum() and (casts["skip"][act] != TR.NULL).any()
    assert (words(got[~act]).reshape(-1, 4) == MISS_WORDS).all() and (flags[~act] == 0).all()
    assert hit.sum() > (5 if name == "driver" else 40) and set(np.nonzero(by)[0]) <= set(range(15)) | set(range(16, 22))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", [BIG, TILT], ids=["big", "tilt"])
def test_t2_the_known_answers_and_every_inactive_form_on_the_device(ctx, scene):
    a, b, c = scene
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    try:
        casts, expected, rows = _known(scene)
        got, flags = both(ctx, d, casts, TR.reference(casts, a, b, c, *library_boxes(d)), "known answers")
        assert _tuples(got) == expected and flags.tolist() == [int(e[0] < L().MAX_FLOAT) for e in expected]
        assert not np.signbit(got["t"]).any()
        _check_contacts(casts, got, scene, rows)
        dead = inactive_forms()
        got, flags = both(ctx, d, dead, TR.reference(dead, a, b, c, *library_boxes(d)), "inactive forms")
        assert (words(got).reshape(-1, 4) == MISS_WORDS).all() and (flags == 0).all()
    finally:
        d.on_destroy()


@pytest.mark.gpu
def test_t3_relations_between_the_calls(ctx):
    """On soup64 with 130 casts and no `skip`: _any == (record != miss); two calls write the same bytes; the record's t is never
    above the least lbvh_trace_closest time from the three vertices along dir; a cast whose start triangle lbvh_triangle_intersects_any
    flags has t == +0; feature is in 0 - 14 or 16 - 21.  The start relation can fail in the definition itself (a start overlap whose
    vertex a is an ulp outside the grown box is no candidate): the restatement is asserted to have no such cast in this set."""
    a, b, c = scene_positions("soup64")
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    lo, hi = library_boxes(d)
    casts = parity_casts("soup64", a, b, c)
    casts["skip"] = TR.NULL
    ref = TR.reference(casts, a, b, c, lo, hi)
    act = TR.active(casts)
    starts = TQ.reference(TQ.make_queries(casts["a"], casts["b"], casts["c"]), a, b, c, lo, hi).flags
    assert (starts[act] == 1).sum() > 3 and (ref.records["t"][act & (starts == 1)] == 0).all()          # no exception in this set
    q = Casts(ctx, d, casts)
    n = len(casts)
    rays = H().DataBuffer(ctx, 3 * n, L().RAY)
    ray_hits = H().DataBuffer(ctx, 3 * n, L().HIT)
    tq = H().DataBuffer(ctx, n, L().TRI_QUERY)
    tflags = H().DataBuffer(ctx, n, np.uint32)
    try:
        first, again = q.cast(), q.cast()
        assert (words(first) == words(again)).all()
        flags = q.any()
        assert (flags == q.any()).all() and ((flags == 1) == (first["t"] < L().MAX_FLOAT)).all()
        assert_records(first, ref, "relations")
        for v, key in enumerate("abc"):
            rays.local[v * n:(v + 1) * n] = make_rays(casts[key], casts["dir"], F(0), casts["t_max"])
        rays.local["dir"][~np.isfinite(rays.local["dir"])] = 1.0
        rays.local["origin"][~np.isfinite(rays.local["origin"])] = 0.0
        rays.sync()
        d.trace_closest(rays, ray_hits)
        rt = ray_hits.get_data()["t"].reshape(3, n).min(axis=0)
        assert (first["t"][act] <= rt[act]).all() and (rt[act] < L().MAX_FLOAT).sum() > 30
        tq.local[:] = TQ.make_queries(casts["a"], casts["b"], casts["c"])
        tq.sync()
        d.triangle_intersects_any(tq, tflags)
        on = (tflags.get_data() == 1) & act
        assert (on == ((starts == 1) & act)).all() and (words(first["t"][on]) == 0).all() and (first["feature"][on] >= START).all()
        f = first["feature"]
        assert (((f <= 14) | ((f >= 16) & (f <= 21)))).all()
    finally:
        for buf in (rays, ray_hits, tq, tflags):
            buf.dispose()
        q.dispose()
        d.on_destroy()


@pytest.fixture(scope="module")
def order_case():
    """1 500 casts on the grid, their reference computed once, on a context of its own"""
    c2 = H().Context(0)
    a, b, c = scene_positions("grid_80x80")
    d = H().RaytracingMeshDrawer(c2, pack(a, b, c)).awake()
    casts = parity_casts("grid_80x80", a, b, c, 1500)
    ref = TR.reference(casts, a, b, c, *library_boxes(d))
    yield c2, d, casts, ref
    d.on_destroy()
    c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 4, 16])
def test_t4_order_independence_under_the_stack_split(order_case, split):
    c2, d, casts, ref = order_case
    h, lib = c2.handle, N().lib
    try:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
        both(c2, d, casts, ref, f"stack split {split}")
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t5_lane_refill_under_a_wave_cap(order_case, waves):
    """1 500 casts on 1, 2, 3 or 7 waves: runs of 215 .. 1 500 casts, about 23 refills per lane on one wave"""
    c2, d, casts, ref = order_case
    assert len(casts) == 1500 and ref.flags.sum() > 500
    h, lib = c2.handle, N().lib
    try:
        N().check(h, lib.lbvh_debug_ray_waves(h, waves))
        both(c2, d, casts, ref, f"{waves} waves")
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))


@pytest.mark.gpu
def test_t6_statistics(order_case):
    c2, d, casts, ref = order_case
    q = Casts(c2, d, casts)
    stats = H().DataBuffer(c2, 1, L().RAY_STATS)
    per = {}
    try:
        for name, call in (("cast", q.cast), ("any", q.any)):
            stats.fill_u32(0)
            N().check(c2.handle, N().lib.lbvh_ray_stats_target(c2.handle, stats.device))
            try:
                got = call()
            finally:
                N().check(c2.handle, N().lib.lbvh_ray_stats_target(c2.handle, None))
            s = stats.get_data()[0]
            per[name] = (int(s["rays"]), int(s["node_fetches"]), int(s["triangle_tests"]))
            assert (words(got) == words(ref.records if name == "cast" else ref.flags)).all()      # the counting kernels: same answers
    finally:
        stats.dispose()
        q.dispose()
    print("casts, node lines, triangle lines:", per)
    n_active = int(TR.active(casts).sum())
    assert per["cast"][0] == n_active == per["any"][0] and per["cast"][2] > 0 and per["any"][2] > 0 and per["cast"][1] >= n_active
    assert per["any"][1] <= per["cast"][1] and per["any"][2] <= per["cast"][2]


@pytest.mark.gpu
def test_t7_errors_the_stale_scene_and_the_stack_limit(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        ext = extent_of(a, b, c)
        casts = aimed_casts(a, b, c, 600, np.random.default_rng(2), [s * ext for s in SIZES])
        ref = TR.reference(casts, a, b, c, *library_boxes(d))
        assert 100 < ref.flags.sum() < 600
        q = Casts(c2, d, casts)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(casts)
        p = lambda buf, k: C.c_void_p(buf.device.value + k)

        def untouched():
            return (words(q.hits.get_data()) == 0x7FC00000).all() and (q.flags.get_data() == 0xDEADBEEF).all()

        assert_records(q.cast(), ref, "before the rejections")
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        for fn, who, out, off in ((lib.lbvh_triangle_cast, b"lbvh_triangle_cast: ", q.hits, 8), (lib.lbvh_triangle_cast_any, b"lbvh_triangle_cast_any: ", q.flags, 2)):
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
        assert lib.lbvh_triangle_cast(h, p(q.casts, 64), 10, C.byref(s), p(q.hits, 16)) == 0
        assert (words(q.hits.get_data()[1:11]) == words(ref.records[1:11])).all()
        # a stale scene: triangles uploaded without a rebuild; the message names the entry point
        d.container.triangle_data.sync()
        q.hits.fill_u32(0x7FC00000)
        q.flags.fill_u32(0xDEADBEEF)
        assert lib.lbvh_triangle_cast(h, q.casts.device, n, C.byref(s), q.hits.device) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_triangle_cast: ") and b"stale" in msg, msg
        assert lib.lbvh_triangle_cast_any(h, q.casts.device, n, C.byref(s), q.flags.device) == -1
        assert lib.lbvh_last_error(h).startswith(b"lbvh_triangle_cast_any: ")
        assert untouched()
        d.rebuild(fast=True)
        # the stack limit: the library's own status word, reported at the next sync, never a silently wrong record
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        q.drawer.triangle_cast(q.casts, q.hits)
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_records(q.cast(), ref, "after the stack limit")
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_t8_hostile_scenes_word_for_word(ctx, name):
    _, casts, ref, d = scene_case(ctx, name)
    try:
        both(ctx, d, casts, ref, name)
    finally:
        d.on_destroy()
    assert ref.flags.sum() > 10, name


@pytest.mark.gpu
def test_t9_mesh_sweep_is_the_least_record_over_the_moving_mesh(ctx):
    a, b, c = scene_positions("soup64")
    d = H().RaytracingMeshDrawer(ctx, pack(a, b, c)).awake()
    try:
        lo, hi = library_boxes(d)
        other = tuple(x[:40] + np.array([0, 0, 40], dtype=F) for x in scene_positions("soup64"))     # a copy of 40 triangles, lifted
        for direction, t_max in (([0, 0, -1], np.inf), ([0.1, 0, -1], 25.0), ([0, 0, 1], np.inf)):
            ref = TR.reference(H().tri_casts_from_mesh(other, direction, t_max), a, b, c, lo, hi)
            record, index = d.mesh_sweep(other, direction, t_max)
            k = int(np.argmin(ref.records["t"]))
            if ref.flags.any():
                assert index == k and (words(np.array([record])) == words(ref.records[k:k + 1])).all()
            else:
                assert index == -1 and (words(np.array([record])) == MISS_WORDS).all()
        assert TR.reference(H().tri_casts_from_mesh(other, [0, 0, -1]), a, b, c, lo, hi).flags.any()
    finally:
        d.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), (700, 7, 1.25)])
def test_t10_cpp_host_driver_tricast_matches_the_python_host(ctx, args):
    """`lbvh_driver tricast` on the driver's own random mesh (default and given count, seed, t_max) against the Python host on the
    same triangles and the same casts"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    res = json.loads(subprocess.run([exe, "tricast"] + [str(x) for x in args], check=True, capture_output=True, text=True).stdout)
    count = args[0] if args else 6000
    tris, _, lo, hi = driver_mesh(4096)
    casts = TR.driver_casts(lo, hi, count, *args[1:])
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    q = Casts(ctx, d, casts)
    got, flags = q.cast(), q.any()
    q.dispose()
    d.on_destroy()
    hit = got["t"] < L().MAX_FLOAT
    assert res["triangles"] == len(tris) and res["casts"] == count and F(res["t_max"]) == F(args[2] if args else 2.0)
    assert res["touching"] == int(hit.sum()) == res["flagged"] == int(flags.sum())
    assert res["at_start"] == int((hit & (got["feature"] >= START)).sum())
    assert res["by_feature"] == np.bincount(got["feature"][hit], minlength=22).tolist()
    assert res["word_sum"] == int(words(got).astype(np.uint64).sum())
    assert [r[1] for r in res["records"]] == got["tri"][:3].tolist() and [r[2] for r in res["records"]] == got["feature"][:3].tolist()
    assert [words(np.array(r[0], dtype=F))[0] for r in res["records"]] == words(got["t"][:3]).tolist()
    assert 0 < res["touching"] < count
