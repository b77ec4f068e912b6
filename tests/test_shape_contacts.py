"""lbvh_capsule_contacts / lbvh_capsule_deepest: how deep a capsule is in each triangle it touches and which way out, as a CSR list
of 32-byte records and as the deepest record per shape, over the four-wide derived traversal scene.  The expectation is
tests/contact_reference.py: the header's definition in numpy float32 on the candidate set of tests/shape_overlap_reference.py — no
tree.  The order inside a segment is not part of the contract, so every list is compared word for word AFTER a host sort of each
segment by `tri`.
  CPU  the surface in every host; hand-made pairs with answers derivable on paper; the reference's list against
       shape_overlap_reference's; the reference against float64 geometry that shares no line with it; the parity sets are not vacuous
  T1   parity of both calls on grid_80x80 and cfg1_4096        T2  the relations to lbvh_capsule_overlaps on the device
  T3   shape counts around a wave; wave caps (the lane refill)  T4  inactive shapes
  T5   count-only and overflow                                  T6  count == 0, every rejection, a stale scene, the live-path list
  T7   a small LDS stack; statistics                            T8  host.push_out on a floor and a wall
  T9   lbvh_driver contacts: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import contact_reference as K
import point_reference as P
import shape_overlap_reference as S
from query_support import driver_mesh, H, L, library_boxes, N, pack, padded_boxes, positions, words
from test_shape_overlaps import extent_of, K_EPS, parity_shapes, PARITY, scene, spoiled
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNT = 2000
NAMES = ("lbvh_capsule_contacts", "lbvh_capsule_deepest")
NULL = 0xFFFFFFFF


def rw(records):
    """layouts.CONTACT records -> (rows, 8) words"""
    return words(records).reshape(-1, 8)


def contact_shapes(a, b, c, count=COUNT, seed=17):
    """test_shape_overlaps.parity_shapes("capsule") — sizes of 0.5 .. 5 % of the extent about points of the surface, 45 % of them moved
    off by 2.5 .. 8 sizes, every eighth a needle through the surface — with, of every 16 shapes, one whose axis is 0 (a sphere) and
    one ten extents away from the mesh, and of every 500 one lying parallel to a face above it at 0.2 .. 0.9 of its radius."""
    q = parity_shapes("capsule", a, b, c, count=count, seed=seed)[0]
    rng = np.random.default_rng(seed + 1000 + len(a))
    i = np.arange(len(q))
    q["axis"][i % 16 == 5] = 0
    flat = np.nonzero(i % 500 == 9)[0]
    k = rng.integers(0, len(a), len(flat))
    e1, e2 = (b - a)[k].astype(np.float64), (c - a)[k].astype(np.float64)
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    length = np.linalg.norm(q["axis"][flat].astype(np.float64), axis=1)
    h = e1 / np.linalg.norm(e1, axis=1, keepdims=True) * length[:, None]
    mid = a[k] + 0.3 * e1 + 0.3 * e2 + n * (q["radius"][flat].astype(np.float64) * rng.uniform(0.2, 0.9, len(flat)))[:, None]
    q["axis"][flat] = h.astype(F)
    q["origin"][flat] = (mid - 0.5 * h).astype(F)
    q["origin"][i % 16 == 13] += F(10 * extent_of(a, b, c))
    return q


_CPU = {}


def cpu_case(name):
    """(a, b, c, box_lo, box_hi, shapes, contact reference with the CPU tests' padded boxes), once per scene"""
    if name not in _CPU:
        a, b, c = positions(scene(name))
        lo, hi = padded_boxes(a, b, c)
        q = contact_shapes(a, b, c)
        _CPU[name] = (a, b, c, lo, hi, q, K.reference(q, a, b, c, lo, hi))
    return _CPU[name]


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------------

def test_header_declares_the_record_and_the_two_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"typedef struct lbvh_contact \{\s+float\s+depth;[^}]*?uint32_t tri;[^}]*?float\s+u, v;[^}]*?float\s+normal\[3\];[^}]*?float\s+s;[^}]*?\} lbvh_contact;", h)
    assert re.search(r"lbvh_status lbvh_capsule_contacts\(lbvh_context\* ctx, const lbvh_capsule\* d_shapes, size_t count, const lbvh_scene\* h_scene,"
                     r"\s+uint64_t\* d_offsets, lbvh_contact\* d_contacts, uint64_t capacity\);", h)
    assert re.search(r"lbvh_status lbvh_capsule_deepest\(lbvh_context\* ctx, const lbvh_capsule\* d_shapes, size_t count, const lbvh_scene\* h_scene,"
                     r"\s+lbvh_contact\* d_out\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert all(n in bounce for n in NAMES)
    text = h[h.index("Capsule contacts: HOW DEEP"):h.index("lbvh_status lbvh_capsule_contacts(")]
    for must in ("Pierce first", "strictly", "NOT clamped", "Face contact", "NOT PART OF THE CONTRACT", "the lower original triangle index",
                 "Nothing can be pruned beyond rule 1", "monotone in the box", "d_offsets[0] included", "Out of scope: box and sheared-box contacts",
                 "lbvh_sort_hit_segments is for 16-byte records", "one huge"):
        assert must in text, must
    overlaps = h[h.index("Shape overlaps: WHICH"):h.index("lbvh_status lbvh_capsule_overlaps(")]
    assert "lbvh_capsule_contacts / lbvh_capsule_deepest" in overlaps and "the\n * box's penetration depth or direction" in overlaps


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_capsule_contacts"]
    assert res is C.c_int32 and len(args) == 7 and args[2] is C.c_size_t and args[6] is C.c_uint64
    res, args = nat.SIGNATURES["lbvh_capsule_deepest"]
    assert res is C.c_int32 and len(args) == 5 and args[2] is C.c_size_t
    assert all(hasattr(nat.lib, n) for n in NAMES)
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.CONTACT.itemsize == 32
    assert [lay.CONTACT.fields[f][1] for f in ("depth", "tri", "u", "v", "normal", "s")] == [0, 4, 8, 12, 16, 28]
    assert rw(np.array([K.NONE])).tolist() == [[0, NULL, 0, 0, 0, 0, 0, 0]]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_capsule_contacts\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+,"
                     r"\s+IntPtr \w+,\s+ulong capacity\);", cs)
    assert re.search(r"public static extern int lbvh_capsule_deepest\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene,\s+IntPtr \w+\);", cs)
    assert "public struct Contact " in cs
    sc = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "ShapeContacts.cs")).read())
    assert all(n in sc for n in NAMES) and "unsafe" not in sc
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert all(f"void {m}(" in hpp for m in ("CapsuleContacts", "CapsuleDeepest"))
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"contacts", contacts_main}' in drv and "lbvh_driver contacts <n_shapes> [seed]" in drv
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("capsule_contacts", "capsule_deepest", "contacts")) and callable(H().push_out)


# ---- CPU: the restatement on pairs with answers derivable on paper -----------------------------------------------------------

TRI = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]


def one_contact(origin, axis, radius, tri=TRI):
    """-> the one record (or None) of one capsule and one scene triangle, with `which`"""
    t = np.array(tri, dtype=F)
    a, b, c = t[None, 0], t[None, 1], t[None, 2]
    shape = S.make_capsules(np.array([origin], dtype=F), np.array([axis], dtype=F), F(radius))
    r = K.reference(shape, a, b, c, *padded_boxes(a, b, c))
    assert int(r.offsets[1]) in (0, 1)
    if int(r.offsets[1]) == 0:
        assert words(r.deepest).tolist() == words(np.array([K.NONE])).tolist()
        return None, None
    assert words(r.deepest).tolist() == words(r.contacts).tolist()
    return r.contacts[0], int(r.which[0])


def test_reference_a_capsule_lying_flat_above_the_face():
    # parallel to the face at the height z < r: every point of the axis is equally near; the order rule takes j = 0, so s = 0
    for z in (0.25, 0.4375):
        k, which = one_contact((1, 1, z), (1, 0.5, 0), 0.5)
        assert which == 0 and k["s"] == 0 and k["normal"].tolist() == [0, 0, 1] and k["depth"] == F(0.5) - F(z)
        assert (k["u"], k["v"]) == (0.25, 0.25)
        k, _ = one_contact((1, 1, -z), (1, 0.5, 0), 0.5)
        assert k["normal"].tolist() == [0, 0, -1] and k["depth"] == F(0.5) - F(z)
    assert one_contact((1, 1, 0.5001), (1, 0.5, 0), 0.5)[0] is None


def test_reference_a_capsule_across_an_edge_from_outside():
    # a vertical axis 0.25 outside the edge y = 0 (z from -1 to 1): the interior of the axis against the interior of the edge — a side
    # of the prism, j = 2 or 3 — at s = 0.5; the way out is -y
    k, which = one_contact((2, -0.25, -1), (0, 0, 2), 0.5)
    assert which in (2, 3) and k["s"] == 0.5 and k["normal"].tolist() == [0, -1, 0] and k["depth"] == 0.25
    assert (k["u"], k["v"]) == (0.5, 0)
    # outside the edge x = 0 (the side C-A: j = 6 or 7), the axis pointing down
    k, which = one_contact((-0.125, 1, 3), (0, 0, -4), 0.5)
    assert which in (6, 7) and k["s"] == 0.75 and k["normal"].tolist() == [-1, 0, 0] and k["depth"] == 0.375
    assert (k["u"], k["v"]) == (0, 0.25)


def test_reference_a_capsule_end_on_at_a_vertex():
    # the axis points away from the vertex (0, 0, 0) along (-3, -4, 0) / 5, the near end 0.25 away; either end first
    k, which = one_contact((-0.15, -0.2, 0), (-3, -4, 0), 0.5)
    assert k["s"] == 0 and (k["u"], k["v"]) == (0, 0) and abs(float(k["depth"]) - 0.25) < 1e-6
    assert np.allclose(k["normal"], (-0.6, -0.8, 0), atol=1e-6)
    k, which = one_contact((-3.15, -4.2, 0), (3, 4, 0), 0.5)
    assert k["s"] == 1 and which == 1 and (k["u"], k["v"]) == (0, 0) and abs(float(k["depth"]) - 0.25) < 1e-6
    assert np.allclose(k["normal"], (-0.6, -0.8, 0), atol=1e-6)


def test_reference_an_axis_that_pierces_the_face():
    # through the face at (1, 1), both ends farther than r from it: z from -1 to 3.  The middle of the axis is above, so the normal
    # is +z and the push brings the lower end to the height r: depth = r + 1; s = t_p = 0.25
    k, which = one_contact((1, 1, -1), (0, 0, 4), 0.5)
    assert which == K.PIERCE and k["s"] == 0.25 and k["normal"].tolist() == [0, 0, 1] and k["depth"] == 1.5 and (k["u"], k["v"]) == (0.25, 0.25)
    # the same axis turned round: the same contact, s = 0.75
    k, which = one_contact((1, 1, 3), (0, 0, -4), 0.5)
    assert which == K.PIERCE and k["s"] == 0.75 and k["normal"].tolist() == [0, 0, 1] and k["depth"] == 1.5
    # the middle below: the way out is -z, past the upper end at the height 1
    k, which = one_contact((1, 1, -3), (0, 0, 4), 0.5)
    assert which == K.PIERCE and k["s"] == 0.75 and k["normal"].tolist() == [0, 0, -1] and k["depth"] == 1.5
    # an end ON the face (dist2 == 0 without a pierce that passes is the same face contact): the axis lies in z >= 0
    k, _ = one_contact((1, 1, 0), (0, 0, 2), 0.5)
    assert k["normal"].tolist() == [0, 0, 1] and k["depth"] == 0.5 and k["s"] == 0


def test_reference_a_degenerate_triangle_has_the_zero_normal():
    # three points on a line: N = 0.  The axis ends on the segment itself (dist2 == 0): the face contact with len == 0
    k, _ = one_contact((1, 0, 0), (0, 0, 2), 0.5, tri=[(0, 0, 0), (2, 0, 0), (4, 0, 0)])
    assert k["normal"].tolist() == [0, 0, 0] and k["depth"] == 0.5
    # beside it, the contact is an ordinary one: the residual decides
    k, _ = one_contact((1, 0.25, 0), (0, 0, 2), 0.5, tri=[(0, 0, 0), (2, 0, 0), (4, 0, 0)])
    assert k["normal"].tolist() == [0, 1, 0] and k["depth"] == 0.25


def test_reference_axis_zero_is_the_point_query():
    rng = np.random.default_rng(3)
    t = np.array(TRI, dtype=F)
    for p in rng.uniform(-1, 5, (40, 3)).astype(F) * np.array([1, 1, 0.1], dtype=F):
        d2, u, v = P.point_triangle(p[None], t[None, 0], (t[1] - t[0])[None], (t[2] - t[0])[None])
        k, which = one_contact(p, (0, 0, 0), 3.0)
        # (a derived triangle j >= 1, formed again from a + e, may win by a rounding and give another s: x = o + 0 * s is o all the same)
        assert which != K.PIERCE and 0 <= k["s"] <= 1 and (words(k["u"]), words(k["v"])) == (words(u[0]), words(v[0]))
        assert k["depth"] == F(3.0) - np.sqrt(d2[0])


# ---- CPU: the reference's list is shape_overlap_reference's -------------------------------------------------------------------

def test_the_list_is_the_overlap_list_word_for_word():
    for name in PARITY:
        a, b, c, lo, hi, q, r = cpu_case(name)
        so = S.reference(q, a, b, c, lo, hi)
        assert (r.offsets == so.offsets).all() and (r.contacts["tri"] == so.tris).all() and r.pairs == so.pairs
        assert ((r.deepest["tri"] != NULL) == (so.flags == 1)).all()
        assert (r.which[so.pierce_only] == K.PIERCE).all()


def test_the_parity_sets_are_not_vacuous():
    for name in PARITY:
        a, b, c, lo, hi, q, r = cpu_case(name)
        n = np.diff(r.offsets).astype(np.int64)
        by_j = np.bincount(r.which, minlength=9)
        print(f"{name}: {len(r.contacts)} contacts of {r.pairs} rule-1 pairs, winning j {by_j[:8].tolist()}, pierce {int(by_j[8])}, face contacts "
              f"{int(r.face.sum())}, shapes with three or more {int((n >= 3).sum())}, depth < 0: {int((r.contacts['depth'] < 0).sum())}")
        assert len(q) == COUNT and len(r.contacts) >= 1000
        assert (by_j[:8] > 0).all() and by_j[8] >= 20 and (n >= 3).sum() >= 20
        assert (q["axis"] == 0).all(axis=1).sum() == COUNT // 16 and (~np.isnan(r.contacts["depth"])).all()
        assert (n[(q["axis"] == 0).all(axis=1)] > 0).any() and (n[(np.arange(COUNT) % 500 == 9) & (np.arange(COUNT) % 16 != 13)] > 0).all() and (n[np.arange(COUNT) % 16 == 13] == 0).all()


# ---- CPU: the reference against float64 geometry that shares no line with it ---------------------------------------------------

def nearest_on_triangle64(p, a, b, c):
    """rows, float64 -> (distance, the nearest point of the triangle): the foot of the perpendicular where it is inside, else the
    nearest point of the three edges"""
    n = np.cross(b - a, c - a)
    foot = p - n * (((p - a) * n).sum(axis=1) / (n * n).sum(axis=1))[:, None]
    inside = np.ones(len(p), dtype=bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, foot - u) * n).sum(axis=1) >= 0
    best, at = np.where(inside, np.linalg.norm(p - foot, axis=1), np.inf), foot.copy()
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        y = u + e * np.clip(((p - u) * e).sum(axis=1) / (e * e).sum(axis=1), 0.0, 1.0)[:, None]
        d = np.linalg.norm(p - y, axis=1)
        at = np.where((d < best)[:, None], y, at)
        best = np.minimum(best, d)
    return best, at


def nearest_of_segments64(p, d, q, e):
    """rows of segments [p, p + d] (d may be 0) and [q, q + e], float64 -> (distance, point of the first, point of the second): the
    lines' solution clamped to the first segment, projected on the second and clamped, projected back and clamped"""
    r = p - q
    dd, ee, de, dr, er = (d * d).sum(axis=1), (e * e).sum(axis=1), (d * e).sum(axis=1), (d * r).sum(axis=1), (e * r).sum(axis=1)
    den = dd * ee - de * de
    ok = den > 1e-30 * np.maximum(dd * ee, 1e-300)
    s = np.clip(np.where(ok, (de * er - dr * ee) / np.where(ok, den, 1.0), 0.0), 0.0, 1.0)
    t = np.clip((de * s + er) / ee, 0.0, 1.0)
    s = np.where(dd > 0, np.clip((de * t - dr) / np.where(dd > 0, dd, 1.0), 0.0, 1.0), 0.0)
    x, y = p + d * s[:, None], q + e * t[:, None]
    return np.linalg.norm(x - y, axis=1), x, y


def nearest_pair64(o, h, a, b, c):
    """rows, float64 -> (dist, x on the axis, y on the triangle, crosses, other): the least over the two ends against the triangle and
    the axis against the three edges, 0 at the crossing point where the axis goes through the triangle.  other = the distance and the
    points of every candidate, for the caller's test of whether the pair is determined."""
    cands = []
    for end in (o, o + h):
        d, y = nearest_on_triangle64(end, a, b, c)
        cands.append((d, end, y))
    for u, v in ((a, b), (b, c), (c, a)):
        cands.append(nearest_of_segments64(o, h, u, v - u))
    dist = np.stack([k[0] for k in cands])
    best = dist.argmin(axis=0)
    rows = np.arange(len(o))
    x, y = np.stack([k[1] for k in cands])[best, rows], np.stack([k[2] for k in cands])[best, rows]
    n = np.cross(b - a, c - a)
    s0, s1 = ((o - a) * n).sum(axis=1), ((o + h - a) * n).sum(axis=1)
    crosses = (s0 * s1 <= 0) & (s0 != s1)
    at = o + h * np.where(crosses, s0 / np.where(crosses, s0 - s1, 1.0), 0.0)[:, None]
    for u, v in ((a, b), (b, c), (c, a)):
        crosses &= (np.cross(v - u, at - u) * n).sum(axis=1) >= 0
    x, y = np.where(crosses[:, None], at, x), np.where(crosses[:, None], at, y)
    return np.where(crosses, 0.0, dist.min(axis=0)), x, y, crosses, cands


def test_the_float64_helpers_know_their_own_answers():
    tri = [np.array([x], dtype=np.float64) for x in TRI]
    at = lambda *p: np.array([p], dtype=np.float64)
    d, x, y, crosses, _ = nearest_pair64(at(1, 1, 1), at(0, 0, 6), *tri)
    assert abs(d[0] - 1) < 1e-12 and np.allclose(x, [[1, 1, 1]]) and np.allclose(y, [[1, 1, 0]]) and not crosses[0]
    d, x, y, crosses, _ = nearest_pair64(at(1, 1, -3), at(0, 0, 4), *tri)
    assert d[0] == 0 and crosses[0] and np.allclose(x, [[1, 1, 0]]) and np.allclose(y, [[1, 1, 0]])
    d, x, y, crosses, _ = nearest_pair64(at(3, 3, -1), at(0, 0, 2), *tri)               # skew to the hypotenuse
    assert abs(d[0] - np.sqrt(2)) < 1e-12 and np.allclose(x, [[3, 3, 0]]) and np.allclose(y, [[2, 2, 0]])
    d, x, y, crosses, _ = nearest_pair64(at(-0.3, -0.4, 0), at(-3, -4, 0), *tri)
    assert abs(d[0] - 0.5) < 1e-12 and np.allclose(y, [[0, 0, 0]])
    d, x, y, crosses, _ = nearest_pair64(at(1, 1, 0.25), at(0, 0, 0), *tri)              # a point
    assert abs(d[0] - 0.25) < 1e-12 and np.allclose(y, [[1, 1, 0]])


def test_reference_agrees_with_an_independent_float64_evaluation():
    """Every contact of the parity sets against float64 geometry (DESIGN section 35 has the derivation).  With band = K_EPS * 2^-24 *
    extent, section 34's bound of a static test on these operations:
      depth    |depth - (r - dist64)| <= band; where the axis crosses the triangle, |depth - (r + the nearer end's height)| <= band
      points   |x(s) - x64| <= band and |y(u, v) - y64| <= band for (x64, y64) the nearest points of a float64 feature pair — an end
               against the triangle, the axis against an edge — whose distance is within the band of the least: near a vertex two
               such pairs lie within the band in distance (the distance is flat to second order about its minimum) and either is
               the answer
      normal   |normal - (x64 - y64) / d64| <= band / d64 + 4 * 2^-24 for that pair: the residual, in error by at most the band, is
               divided by its length; the square root and the division round once each, on a vector of unit length.  Where the axis
               crosses: the plane's unit normal on the side of the middle of the axis, within 8 * 2^-24 (the cross product's terms);
               either side where the middle is within the band of the plane (the needles of the parity sets)
    The depth is asked of every contact that fp32 and float64 both call a crossing or both do not.  Left out of the normal and point
    comparison, at most 1 % of the contacts: dist64 below the band (no direction); an axis parallel within the band to the face or to
    an edge (|axis . n| or |axis x e| below the band: a continuum of nearest pairs, of which the five feature pairs name only the
    ends); a crossing that the two decide differently (within the band of an edge).
    Measured, seed 17: grid_80x80 17 116 contacts, 55 left out (0.321 %), depth error <= 0.024 band, point error <= 0.69 band;
    cfg1_4096 1 239 contacts, 2 left out (0.161 %), point error <= 0.72 band."""
    eps = 2.0 ** -24
    for name in PARITY:
        a, b, c, lo, hi, q, r = cpu_case(name)
        band = K_EPS * eps * extent_of(a, b, c)
        seg = np.repeat(np.arange(COUNT), np.diff(r.offsets).astype(np.int64))
        tri = r.contacts["tri"].astype(np.int64)
        o, h, rad = (q[f][seg].astype(np.float64) for f in ("origin", "axis", "radius"))
        a64, b64, c64 = (x[tri].astype(np.float64) for x in (a, b, c))
        e1, e2 = (b - a)[tri].astype(np.float64), (c - a)[tri].astype(np.float64)        # the fp32 differences of the triangle line
        dist, x64, y64, crosses, cands = nearest_pair64(o, h, a64, b64, c64)
        depth, normal = r.contacts["depth"].astype(np.float64), r.contacts["normal"].astype(np.float64)
        x = o + h * r.contacts["s"].astype(np.float64)[:, None]
        y = a64 + e1 * r.contacts["u"].astype(np.float64)[:, None] + e2 * r.contacts["v"].astype(np.float64)[:, None]
        n = np.cross(b64 - a64, c64 - a64)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        g0, g1 = ((o - a64) * n).sum(axis=1), ((o + h - a64) * n).sum(axis=1)
        # the depth
        want = np.where(crosses, rad + np.minimum(np.abs(g0), np.abs(g1)), rad - dist)
        undecided = crosses != (r.which == K.PIERCE)
        err = np.abs(depth - want)
        assert (err[~undecided] <= band).all(), (name, np.nonzero(~undecided & (err > band))[0][:5], err.max(), band)
        # what is left out
        parallel = np.abs((h * n).sum(axis=1)) < band
        for u, v in ((a64, b64), (b64, c64), (c64, a64)):
            parallel |= np.linalg.norm(np.cross(h, (v - u) / np.linalg.norm(v - u, axis=1, keepdims=True)), axis=1) < band
        parallel &= np.linalg.norm(h, axis=1) > 0
        left_out = ((dist < band) & ~crosses) | parallel | undecided
        keep = ~left_out
        print(f"{name}: {len(seg)} contacts, {int(crosses.sum())} cross, left out {int(left_out.sum())} ({100.0 * left_out.mean():.3f} %): "
              f"{int(((dist < band) & ~crosses).sum())} below the band, {int(parallel.sum())} parallel, {int(undecided.sum())} crossings decided "
              f"differently; depth error <= {err[~undecided].max() / band:.3f} band")
        assert left_out.mean() <= 0.01
        # the points and the normal, against the best-matching feature pair within the band of the least distance
        side = np.where(g0 + g1 >= 0, 1.0, -1.0)[:, None]
        ep = np.maximum(np.linalg.norm(x - x64, axis=1), np.linalg.norm(y - y64, axis=1))
        en = np.linalg.norm(normal - np.where(crosses[:, None], side * n, (x64 - y64) / np.where(dist > 0, dist, 1.0)[:, None]), axis=1)
        # (the middle of a needle lies on the surface: within the band of the plane either side is the answer, and the depth is the same)
        en = np.where(crosses & (np.abs(g0 + g1) < 2 * band), np.minimum(en, np.linalg.norm(normal + side * n, axis=1)), en)
        bound = np.where(crosses, 8 * eps, band / np.where(dist > 0, dist, 1.0) + 4 * eps)
        for d_k, x_k, y_k in cands:
            ep_k = np.maximum(np.linalg.norm(x - x_k, axis=1), np.linalg.norm(y - y_k, axis=1))
            better = (d_k < dist + band) & ~crosses & (d_k > 0) & (ep_k < ep)
            safe = np.where(d_k > 0, d_k, 1.0)
            ep = np.where(better, ep_k, ep)
            en = np.where(better, np.linalg.norm(normal - (x_k - y_k) / safe[:, None], axis=1), en)
            bound = np.where(better, band / safe + 4 * eps, bound)
        assert (ep[keep] <= band).all(), (name, np.nonzero(keep & (ep > band))[0][:5], ep[keep].max() / band)
        assert (en[keep] <= bound[keep]).all(), (name, np.nonzero(keep & (en > bound))[0][:5], (en[keep] / bound[keep]).max())
        flat = (r.contacts["normal"] == 0).all(axis=1)
        assert not flat.any() and (np.abs(np.linalg.norm(normal, axis=1) - 1) <= 4 * eps).all()
        print(f"{name}: point error <= {ep[keep].max() / band:.3f} band, normal error <= {(en[keep] / bound[keep]).max():.3f} of its bound")


def test_driver_generator_is_deterministic_and_inside_the_box():
    lo, hi = np.array([-1, -2, -3], dtype=F), np.array([4, 5, 6], dtype=F)
    caps, caps2 = K.driver_capsules(lo, hi, 50, seed=5), K.driver_capsules(lo, hi, 50, seed=5)
    assert (words(caps) == words(caps2)).all() and (caps["origin"] >= lo).all() and (caps["origin"] <= hi).all()
    assert (np.abs(caps["axis"]) <= 6).all() and (caps["radius"] == 3).all() and S.active(caps).all()
    assert (words(caps) != words(K.driver_capsules(lo, hi, 50, seed=6))).any()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

class Caps:
    """device buffers of one capsule set; contacts() / deepest() = one call each on caller-owned buffers"""

    def __init__(self, ctx, drawer, shapes):
        self.ctx, self.drawer, self.count = ctx, drawer, len(shapes)
        self.shapes = H().DataBuffer(ctx, max(len(shapes), 1), L().CAPSULE)
        self.shapes.local[:len(shapes)] = shapes
        self.shapes.sync()
        self.offsets = H().DataBuffer(ctx, len(shapes) + 1, np.uint64)
        self.out = H().DataBuffer(ctx, max(len(shapes), 1), L().CONTACT)

    def run(self, contacts=None, capacity=None):
        """offsets (host copy) after one lbvh_capsule_contacts; contacts: a CONTACT DataBuffer or None, capacity defaults to its size"""
        self.offsets.fill_u32(0xDEADBEEF)
        s = self.drawer.container.scene()
        cap = 0 if contacts is None else (contacts.size if capacity is None else capacity)
        N().check(self.ctx.handle, N().lib.lbvh_capsule_contacts(self.ctx.handle, self.shapes.device, self.count, C.byref(s), self.offsets.device,
                                                                 contacts.device if contacts is not None else None, cap))
        return self.offsets.get_data().copy()

    def lists(self):
        """(offsets, records with every segment sorted by tri) through the count -> allocate -> fill convenience"""
        off, recs = self.drawer.contacts(self.shapes)
        return off, K.sort_segments(off, recs)

    def deepest(self):
        self.out.fill_u32(0xDEADBEEF)
        self.drawer.capsule_deepest(self.shapes, self.out)
        return self.out.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.shapes, self.offsets, self.out):
            b.dispose()


def assert_equal_contacts(got, ref, what=""):
    (go, gc), ro, rc = got, ref.offsets, ref.contacts
    assert (go[:len(ro)] == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gc) == len(rc) == int(ro[-1]), what
    bad = np.nonzero((rw(gc) != rw(rc)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], gc[bad[:5]], rc[bad[:5]])


def assert_equal_deepest(got, ref, what=""):
    bad = np.nonzero((rw(got) != rw(ref.deepest)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], ref.deepest[bad[:5]])


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


def gpu_case(ctx, name):
    """(a, b, c, lo, hi, shapes, reference with the library's boxes, drawer): the reference once per scene"""
    a, b, c, lo, hi, d = gpu_scene(ctx, name)
    if ("ref", name) not in _GPU:
        q = contact_shapes(a, b, c)
        _GPU["ref", name] = (q, K.reference(q, a, b, c, lo, hi))
    return (a, b, c, lo, hi) + _GPU["ref", name] + (d,)


def overlap_lists(ctx, d, q):
    """(offsets, tris sorted inside every segment, flags) of lbvh_capsule_overlaps / _any on the device buffers of a Caps"""
    off, tris = d.touching(q.shapes, device_sort=True)
    flags = H().DataBuffer(ctx, max(q.count, 1), np.uint32)
    d.capsule_overlaps_any(q.shapes, flags)
    f = flags.get_data()[:q.count].copy()
    flags.dispose()
    return off, tris, f


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, name)
    assert len(ref.contacts) >= 1000
    q = Caps(ctx, d, shapes)
    assert_equal_contacts(q.lists(), ref)
    assert_equal_deepest(q.deepest(), ref)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_t2_relations_to_the_overlaps_on_the_device(ctx, name):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, name)
    q = Caps(ctx, d, shapes)
    total = int(ref.offsets[-1])
    buf = H().DataBuffer(ctx, total, L().CONTACT)
    runs = []
    for _ in range(2):
        buf.fill_u32(0xABABABAB)
        off = q.run(buf)
        runs.append((off, words(buf.get_data()).copy(), words(q.deepest()).copy()))
    assert all((x == y).all() for x, y in zip(runs[0], runs[1]))                  # two calls write the same bytes
    off, recs, deep = runs[0][0], buf.get_data().copy(), q.deepest()
    o_off, o_tris, o_flags = overlap_lists(ctx, d, q)
    assert off.tobytes() == o_off.tobytes()
    assert (K.sort_segments(off, recs)["tri"] == o_tris).all()
    assert ((deep["tri"] != NULL) == (o_flags == 1)).all()
    assert (words(deep) == words(K.deepest_of(off, recs))).all()                  # the maximum of its own segment under the order
    for k in np.nonzero(np.diff(off))[0][:200]:
        seg = recs[int(off[k]):int(off[k + 1])]
        assert deep["depth"][k] == seg["depth"].max() and deep["tri"][k] == seg["tri"][seg["depth"] == seg["depth"].max()].min()
    buf.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_t3_shape_counts_around_a_wave(ctx, count):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "grid_80x80")
    first = int(np.nonzero(np.diff(ref.offsets))[0][0])                # (the single shape is one that touches)
    sub = shapes[first:first + count]
    r = K.reference(sub, a, b, c, lo, hi)
    assert int(r.offsets[-1]) > 0
    q = Caps(ctx, d, sub)
    assert_equal_contacts(q.lists(), r, count)
    assert_equal_deepest(q.deepest(), r, count)
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_t3_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 shapes on 1, 2, 3 or 7 waves: runs of 1 500 .. 215, every lane refilled many times"""
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "grid_80x80")
    if "caps" not in _GPU:
        sub = shapes[:1500].copy()
        sub["origin"][100:235, 0] = np.nan                              # a block of inactive shapes inside a run
        _GPU["caps"] = (sub, K.reference(sub, a, b, c, lo, hi))
    sub, r = _GPU["caps"]
    q = Caps(ctx, d, sub)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        got, deep = q.lists(), q.deepest()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_equal_contacts(got, r, waves)
    assert_equal_deepest(deep, r, waves)
    q.dispose()


@pytest.mark.gpu
def test_t4_inactive_shapes_among_active_ones(ctx):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "grid_80x80")
    sub, places = spoiled("capsule", shapes[:700])
    act = S.active(sub)
    assert (~act).sum() == len(places) and not act[places].any()
    r = K.reference(sub, a, b, c, lo, hi)
    q = Caps(ctx, d, sub)
    off, recs = q.lists()
    deep = q.deepest()
    assert_equal_contacts((off, recs), r)
    assert_equal_deepest(deep, r)
    assert (np.diff(off)[~act] == 0).all() and (rw(deep[~act]) == rw(np.array([K.NONE]))).all()
    # the neighbours are what they were in the full set
    full = np.diff(ref.offsets)[:700]
    assert (np.diff(off)[act] == full[act]).all() and np.diff(off)[act].sum() > 0
    assert (words(deep[act]) == words(ref.deepest[:700][act])).all()
    q.dispose()
    # an inactive shape is never walked: the set of only them fetches no node
    idle = Caps(ctx, d, sub[~act])
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    stats.fill_u32(0)
    N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    try:
        off, deep = idle.run(None), idle.deepest()
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
    st = stats.get_data()[0]
    assert (off == 0).all() and (rw(deep) == rw(np.array([K.NONE]))).all()
    assert (st["rays"], st["node_fetches"], st["triangle_tests"]) == (0, 0, 0)
    stats.dispose()
    idle.dispose()


@pytest.mark.gpu
def test_t5_count_only_and_overflow(ctx):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "cfg1_4096")
    total, guard = int(ref.offsets[-1]), 512
    q = Caps(ctx, d, shapes)
    assert (q.run(None) == ref.offsets).all()                            # capacity == 0, d_contacts == NULL
    buf = H().DataBuffer(ctx, total + guard, L().CONTACT)
    inside = [int(ref.offsets[k]) + 1 for k in np.nonzero(np.diff(ref.offsets) >= 3)[0][[2, -2]]]      # capacities that cut a segment
    for cap in [0, 1, total - 1] + inside:
        buf.fill_u32(0xABABABAB)
        off = q.run(buf, capacity=cap)                                   # (capacity 0 with a buffer: still count-only)
        got = buf.get_data().copy()
        assert (off == ref.offsets).all() and int(off[-1]) == total      # d_offsets[count] is the need
        assert (words(got[cap:]) == 0xABABABAB).all(), cap               # nothing at the capacity or beyond
        fits = np.nonzero(ref.offsets[1:] <= cap)[0]
        assert len(fits) < COUNT
        last = int(ref.offsets[fits[-1] + 1]) if len(fits) else 0
        part = K.sort_segments(ref.offsets[:(fits[-1] + 2) if len(fits) else 1], got[:last])
        assert (words(part) == words(ref.contacts[:last])).all(), cap
    assert all(ref.offsets[np.searchsorted(ref.offsets, cap, side="right") - 1] < cap < total for cap in inside)
    buf.dispose()
    q.dispose()


@pytest.mark.gpu
def test_t6_count_zero_rejections_a_stale_scene_and_the_live_path_list():
    """the rows test_shape_overlaps.py has for the overlaps, for these two: on a context of its own"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        centre = a[rng.integers(0, 64, 130)] + rng.normal(size=(130, 3)).astype(F) * F(2)
        shapes = S.make_capsules(centre, rng.normal(size=(130, 3)).astype(F), F(0.7))
        ref = K.reference(shapes, a, b, c, lo, hi)
        assert 0 < (ref.deepest["tri"] != NULL).sum() < 130
        q = Caps(ctx, d, shapes)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, L().CONTACT)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        both, one = lib.lbvh_capsule_contacts, lib.lbvh_capsule_deepest
        dq, do, dd, dl = q.shapes.device, q.offsets.device, q.out.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, q.out, lst)
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
        assert both(h, dq, 0, C.byref(s), do, dl, 64) == 0 and one(h, dq, 0, C.byref(s), dd) == 0     # count == 0: a no-op
        for args in ((None, 10, C.byref(s), do, None, 0), (dq, 10, None, do, None, 0), (dq, 10, C.byref(s), None, None, 0),
                     (dq, 10, C.byref(s), do, None, 5), (at(q.shapes, 4), 10, C.byref(s), do, None, 0),
                     (dq, 10, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, C.byref(s), do, at(lst, 8), 8),
                     (dq, 10, C.byref(s), do, at(lst, 4), 8), (dq, 1 << 32, C.byref(s), do, None, 0)):
            assert both(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_capsule_contacts: invalid argument")
        for args in ((None, 10, C.byref(s), dd), (dq, 10, None, dd), (dq, 10, C.byref(s), None), (at(q.shapes, 8), 10, C.byref(s), dd),
                     (dq, 10, C.byref(s), at(q.out, 8)), (dq, 1 << 32, C.byref(s), dd)):
            assert one(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_capsule_deepest: invalid argument")
        assert both(None, dq, 10, C.byref(s), do, None, 0) == -1 and one(None, dq, 10, C.byref(s), dd) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        for fn, args, name in ((both, (do, None, 0), b"lbvh_capsule_contacts"), (one, (dd,), b"lbvh_capsule_deepest")):
            assert fn(h, dq, 130, C.byref(s), *args) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        assert (trace_rays() == expected_path).all()
        # aligned sub-ranges are fine
        assert both(h, at(q.shapes, 32), 10, C.byref(s), at(q.offsets, 8), at(lst, 32), 8) == 0
        assert one(h, at(q.shapes, 32), 10, C.byref(s), at(q.out, 32)) == 0
        for form in (q.lists, q.deepest):
            # each call drops the live-ray list the trace before it left: lbvh_trace_rays makes its own again
            assert (trace_rays() == expected_path).all()
            form()
        assert (trace_rays() == expected_path).all()
        assert_equal_contacts(q.lists(), ref)
        assert_equal_deepest(q.deepest(), ref)
        for buf in (lst, states, path_hits):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_t7_a_small_lds_stack_and_the_statistics(ctx):
    a, b, c, lo, hi, shapes, ref, d = gpu_case(ctx, "grid_80x80")
    q = Caps(ctx, d, shapes)
    h, lib = ctx.handle, N().lib
    # a small LDS part exercises the device-memory part of the stack: the same answers
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        got, deep = q.lists(), q.deepest()
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert_equal_contacts(got, ref, "stack split 1")
    assert_equal_deepest(deep, ref, "stack split 1")
    # statistics: the full form reports the count walk's plus the fill walk's; the counting instantiations write the same words
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    big = H().DataBuffer(ctx, max(int(ref.offsets[-1]), 1), L().CONTACT)
    seen = []
    try:
        for form in ("count", "full", "deepest"):
            stats.fill_u32(0)
            N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
            if form == "deepest":
                assert_equal_deepest(q.deepest(), ref, "counting")
            else:
                off = q.run(big if form == "full" else None)
                assert (off == ref.offsets).all()
                if form == "full":
                    assert_equal_contacts((off, K.sort_segments(off, big.get_data().copy())), ref, "counting")
            N().check(h, lib.lbvh_ray_stats_target(h, None))
            st = stats.get_data()[0]
            seen.append((int(st["rays"]), int(st["node_fetches"]), int(st["triangle_tests"])))
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
    print("shapes, node fetches, triangle lines: count-only %s, full %s, deepest %s" % tuple(seen))
    active = int(S.active(shapes).sum())
    assert seen[0][0] == active and seen[1] == tuple(2 * x for x in seen[0]) and seen[2] == seen[0]
    assert seen[0][2] == ref.pairs                                   # one triangle line per pair that passes rule 1
    for buf in (stats, big):
        buf.dispose()
    q.dispose()


def push_out_child():
    """test_t8's body, in a process of its own that imported torch first (see there); prints one JSON line"""
    w = 20.0
    quad = lambda p0, p1, p2, p3: [(p0, p1, p2), (p0, p2, p3)]
    floor = quad((-w, -w, 0), (w, -w, 0), (w, w, 0), (-w, w, 0))
    wall = quad((0, -w, -w), (0, w, -w), (0, w, w), (0, -w, w))
    pos = np.array(floor + wall, dtype=F)
    tris = pack(pos[:, 0], pos[:, 1], pos[:, 2])
    rng = np.random.default_rng(11)
    n, r = 64, 0.5
    sink_z, sink_x = rng.uniform(0.05, 0.45, n), rng.uniform(0.05, 0.45, n)
    kind = np.arange(n) % 3                                             # 0: the floor, 1: the wall, 2: both
    origin = np.stack([np.where(kind == 0, 5.0, r - sink_x), rng.uniform(-8, 8, n), np.where(kind == 1, 5.0, r - sink_z)], axis=1)
    axis = np.stack([rng.uniform(0, 0.5, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 2, n)], axis=1)
    shapes = H().capsule_shapes(origin, axis, r)
    with H().Context(0) as ctx:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        d.build_fast_scene()
        q = Caps(ctx, d, shapes)
        before = q.deepest()
        moved, depths = H().push_out(d, q.shapes, 1e-3, iterations=4)
        flags = H().DataBuffer(ctx, n, np.uint32)
        flags.fill_u32(0xDEADBEEF)
        d.capsule_overlaps_any(q.shapes, flags)
        after = q.shapes.get_data()["origin"].astype(np.float64)
        print(json.dumps({"before_in_range": bool(((before["depth"] > 0) & (before["depth"] < r)).all()), "same_buffer": moved is q.shapes,
                          "depths": depths.tolist(), "flags": flags.get_data().tolist(),
                          "out_of_both": bool(((after[:, 0] > r) & (after[:, 2] > r)).all()),
                          "sideways": float(max(np.abs(after[:, 1] - origin[:, 1].astype(F)).max(), np.abs(after[kind == 0, 0] - 5.0).max(),
                                                np.abs(after[kind == 1, 2] - 5.0).max()))}))
        flags.dispose()
        q.dispose()
        d.on_destroy()


@pytest.mark.gpu
def test_t8_push_out_of_a_floor_and_a_wall():
    """A floor z = 0 of two large triangles sharing a diagonal, a wall x = 0 of two, and 64 capsules of radius 0.5 sunk by less than
    the radius into the floor, the wall or both (the axis points up and away from the wall, so its origin is the nearest point to
    both).  Each push moves a capsule by depth + skin along one of two orthogonal normals, which leaves it farther than the radius from
    that plane and changes nothing about the other: two iterations suffice, four is the margin.
    push_out computes with torch on the device.  Where torch brings a HIP runtime of its own, a process has to load torch before the
    library for the two to share one runtime; this process loaded the library long ago, so the body runs in a child that imports
    torch first."""
    code = "import torch, sys; torch.cuda.init(); sys.path.insert(0, %r); import test_shape_contacts as T; T.push_out_child()" % os.path.join(ROOT, "tests")
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["before_in_range"] and res["same_buffer"]
    assert len(res["depths"]) == 64 and all(x <= 0 for x in res["depths"])
    assert res["flags"] == [0] * 64
    # along the planes a push moves a capsule only by the rounding of the contact point on triangles 40 across (2^-24 * 40 * K_EPS is
    # 4 * 10^-5) times at most 4 pushes of less than one radius each
    assert res["out_of_both"] and res["sideways"] <= 1e-4


@pytest.mark.gpu
def test_t9_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver contacts 2000 11`: CapsuleContacts and CapsuleDeepest of lbvh_host.hpp on the driver's own mesh and capsules, against
    the brute force on the Python mirrors of its generators and the boxes the library makes for that mesh"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "contacts", str(count), "11"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    boxes = library_boxes(d)
    d.on_destroy()
    r = K.reference(K.driver_capsules(lo, hi, count, seed=11), a, b, c, *boxes)
    n = np.diff(r.offsets).astype(np.int64)
    weigh = lambda recs: (rw(recs).astype(np.uint64) * np.arange(1, 9, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    assert int(r.offsets[-1]) > 100
    assert (res["triangles"], res["shapes"], res["total"], res["non_empty"]) == (4096, count, int(r.offsets[-1]), int((n > 0).sum()))
    assert res["touching"] == int((r.deepest["tri"] != NULL).sum())
    assert res["word_sum"] == int(weigh(r.contacts).sum(dtype=np.uint64))
    assert res["deepest_sum"] == int((weigh(r.deepest) * np.arange(1, count + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    first = np.nonzero(n)[0][:3]
    assert res["deepest"] == [[int(k)] + rw(r.deepest[k:k + 1])[0].tolist() for k in first]
