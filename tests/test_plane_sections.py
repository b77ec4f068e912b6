"""lbvh_plane_sections: the contour where a plane cuts the mesh, one 32-byte record per cut triangle, every plane spread over the device
in the frame of lbvh_region_overlaps_large (include/lbvh.h).  The expectation is the numpy restatement of
tests/plane_section_reference.py, word for word (every NaN folded to one pattern: only planes with an infinite word produce them).
  CPU  the surface in every host; the restatement against float64 (K = 64, |cos| >= 2^-5, at most 1 % of the ends left out — the figures
       are printed); host.stitch_sections on the restatement's records: closed, consistently oriented loops on a sphere and a torus
  L1   parity on grid_80x80, example_object3, cfg1_4096, an icosphere, a torus and scenes of 2 and 5 triangles under forced task caps
       4, 5, 8, 64, 4 096 and the default, on the special planes and 1, 2, 63, 64, 65 and 1 500 random ones
  L2   the record invariants on the device output       L3  two calls write the same bytes       L4  the CSR contract
  L5   the candidates lie in lbvh_region_overlaps_large's TOUCHING list of the slab regions; triangle_tests equals its total
  L6   wave caps, the stack split, the stack limit       L7  rejections, a stale scene, a failed allocation, count == 0, the live-path
       list, the ABI version       L8  lbvh_driver sections 200 7
A scene of ONE triangle cannot be built (lbvh_build_tree and lbvh_refit require two), so there is no GPU case for it: the restatement
alone is checked on it."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import plane_section_reference as PS
import test_region_queries as Q
from query_support import driver_mesh, H, L, library_boxes, N, pack, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CAPS = [4, 5, 8, 64, 4096, 0]                         # 0: the host's choice
COUNTS = [1, 2, 63, 64, 65, 1500]
SCENES = ["grid_80x80", "example_object3", "cfg1_4096", "icosphere", "torus", "two", "five"]
POISON = 0x7FC0DEAD


# ---- scenes -------------------------------------------------------------------------------------------------------------------------

def icosphere(level=3, radius=3.0):
    """a closed icosphere wound outwards: 20 * 4^level triangles (1 280), the vertices shared bit for bit between neighbours"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for i, j, k in f:
            a, b, c = m(i, j), m(j, k), m(k, i)
            out += [(i, a, c), (j, b, a), (k, c, b), (a, b, c)]
        f = out
    p = (np.array(v) * radius + np.array([0.3, -0.2, 0.1])).astype(F)
    f = np.array(f)
    return pack(p[f[:, 0]], p[f[:, 1]], p[f[:, 2]])


def torus(nu=24, nv=16, big=3.0, small=1.0):
    """a closed torus wound outwards: 2 * nu * nv triangles (768)"""
    u, w = np.meshgrid(np.arange(nu) * 2.0 * np.pi / nu, np.arange(nv) * 2.0 * np.pi / nv, indexing="ij")
    p = np.stack([(big + small * np.cos(w)) * np.cos(u), (big + small * np.cos(w)) * np.sin(u), small * np.sin(w)], axis=-1).astype(F)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    p00, p10, p01, p11 = p[i, j].reshape(-1, 3), p[i1, j].reshape(-1, 3), p[i, j1].reshape(-1, 3), p[i1, j1].reshape(-1, 3)
    return pack(np.concatenate([p00, p00]), np.concatenate([p10, p11]), np.concatenate([p11, p01]))


def scene(name):
    if name == "icosphere":
        return icosphere()
    if name == "torus":
        return torus()
    if name in ("one", "two", "five"):
        # seed 8: the float64 check's 1 % condition allows ONE end of a set of about 110 to lie on an edge with |cos| < 2^-5, and the
        # axis-aligned stacks hit an edge three times over; with this seed no edge of the five triangles is that close to an axis plane
        return scenes.random_triangles(n=5, seed=8, extent=5.0, edge=4.0)[:{"one": 1, "two": 2, "five": 5}[name]].copy()
    return Q.scene(name)


# ---- plane sets -----------------------------------------------------------------------------------------------------------------------

def fp32_through(n, p):
    """d with pv(p) == 0 exactly: d = -((nx * px + ny * py) + nz * pz) in fp32"""
    n, p = np.asarray(n, dtype=F), np.asarray(p, dtype=F)
    return -((n[..., 0] * p[..., 0] + n[..., 1] * p[..., 1]) + n[..., 2] * p[..., 2])


def random_planes(a, b, c, count, seed=42):
    """random orientations through random points of the scene's extent.  (Seed 42, not 41: a prefix of 63 planes has about 110 ends
    on the one-triangle scene, where the float64 check's 1 % condition allows one end under the cosine floor; 41 drew two.)"""
    rng = np.random.default_rng(seed + len(a))
    pts = np.concatenate([a, b, c])
    n = rng.normal(size=(count, 3))
    n *= rng.uniform(0.25, 4.0, (count, 1)) / np.linalg.norm(n, axis=1, keepdims=True)
    return H().planes(n, rng.uniform(pts.min(axis=0), pts.max(axis=0), (count, 3)))


def special_planes(a, b, c):
    """axis-aligned stacks whose normals have zero and -0 components; planes exactly through vertices (s == 0), axis-aligned ones through
    whole rows of them on the grid; planes that miss the mesh; on the grid the plane that contains every face; n = 0 with d = 0, 1,
    -1; NaN, +inf and -inf in each position"""
    rng = np.random.default_rng(43 + len(a))
    pts = np.concatenate([a, b, c])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (lo + hi) / F(2.0), float((hi - lo).max())
    n, d = [], []
    for axis in range(3):
        for sign, zeros in ((1.0, (0.0, -0.0)), (-1.0, (-0.0, 0.0)), (1.0, (-0.0, -0.0))):
            for level in np.linspace(lo[axis], hi[axis], 7)[1:-1]:
                normal = np.insert(np.array(zeros), axis, sign)
                n.append(normal)
                d.append(-sign * level)
    k = rng.integers(0, len(a), 12)
    for i, tri in enumerate(k):                                      # through stored vertices: axis-aligned (rows of the grid) and tilted
        v = (a, b, c)[i % 3][tri]
        normal = np.eye(3)[i % 3] if i < 6 else rng.normal(size=3)
        n.append(normal)
        d.append(fp32_through(normal, v))
    for i in range(4):                                               # they miss the mesh
        normal = rng.normal(size=3)
        n.append(normal)
        d.append(-(normal * (hi + (2.0 + i) * ext)).sum() if i % 2 else 4.0 * ext * np.linalg.norm(normal) + abs((normal * mid).sum()))
    if (pts[:, 2] == 0).all():                                       # the grid: the plane of a face as its edges give it, and z = 0 itself
        face = np.cross(b[0] - a[0], c[0] - a[0]).astype(F)          # (elsewhere a face's plane meets its own triangle in rounding noise
        n.append(face)                                               # only: two ends at |cos| ~ 0, which a scene of one triangle cannot
        d.append(fp32_through(face, a[0]))                           # keep under the float64 check's 1 % condition)
    n.append(np.array([0.0, 0.0, 1.0]))
    d.append(-0.0)
    for dd in (0.0, 1.0, -1.0):
        n.append(np.zeros(3))
        d.append(dd)
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(4):
            row = np.append(rng.normal(size=3), -(rng.normal(size=3) * mid).sum())
            row[:3] = rng.normal(size=3)
            row[3] = -(row[:3] * mid).sum()
            row[pos] = bad
            n.append(row[:3])
            d.append(row[3])
    return PS.make_planes(np.array(n, dtype=F), np.array(d, dtype=F))


_CPU = {}


def cpu_case(name, lo=None, hi=None):
    """(a, b, c, [(label, planes, reference Result)]): the special set and the prefixes of 1 500 random planes; the restatement runs
    once per scene (and once more with the library's boxes for the GPU tests, which are the same floats)"""
    key = (name, lo is not None)
    if key not in _CPU:
        a, b, c = positions(scene(name))
        if lo is None:
            lo, hi = padded_boxes(a, b, c)
        special, rnd = special_planes(a, b, c), random_planes(a, b, c, max(COUNTS))
        sets = [("special", special, PS.reference(special, a, b, c, lo, hi))]
        full = PS.reference(rnd, a, b, c, lo, hi)
        for count in COUNTS:
            last = int(full.offsets[count])
            sets.append((f"random{count}", rnd[:count], PS.Result(full.offsets[:count + 1].copy(), full.records[:last], full.rows[:last])))
        _CPU[key] = (a, b, c, lo, hi, sets)
    return _CPU[key]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_in_every_host():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"#define LBVH_PLANE_SECTIONS_MAX_COUNT\s+65536\b", h) and re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    assert "typedef struct lbvh_plane { float n[3]; float d; } lbvh_plane;" in h
    assert re.search(r"typedef struct lbvh_plane_segment \{\s+float p0\[3\]; uint32_t tri;[^\n]*\n\s+float p1\[3\]; uint32_t edges;[^\n]*\n\} lbvh_plane_segment;", h)
    assert re.search(r"lbvh_status lbvh_plane_sections\(lbvh_context\* ctx, const lbvh_plane\* d_planes, size_t count, const lbvh_scene\* h_scene,\s+"
                     r"uint64_t\* d_offsets, lbvh_plane_segment\* d_segments, uint64_t capacity\);", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_plane_sections" in bounce
    text = h[h.index("Plane sections: WHERE does a plane cut the mesh"):h.index("#define LBVH_PLANE_SECTIONS_MAX_COUNT")]
    for must in ("P >= 0 && N <= 0", "t = sp / (sp - sm)", "X = Vp + (Vm - Vp) * t", "bits 16 .. 18", "STITCHING", "is NOT promised",
                 "counts as the positive side", "NOT PART OF THE CONTRACT", "write the same bytes", "no kernel waits for another workgroup",
                 "count > LBVH_PLANE_SECTIONS_MAX_COUNT", "LBVH_ERR_OUT_OF_MEMORY", "triangle_tests the triangle lines read", "an _any form",
                 "coplanar faces", "Out of scope"):
        assert must in text, must
    nat = N()
    res, args = nat.SIGNATURES["lbvh_plane_sections"]
    assert res is C.c_int32 and args == nat.SIGNATURES["lbvh_triangle_intersection_segments"][1]
    assert callable(nat.lib.lbvh_plane_sections) and nat.PLANE_SECTIONS_MAX_COUNT == 65536 and nat.lib.lbvh_abi_version() == 11
    lay = L()
    assert lay.PLANE.itemsize == 16 and [lay.PLANE.fields[f][1] for f in ("n", "d")] == [0, 12]
    assert lay.PLANE_SEGMENT.itemsize == 32 and [lay.PLANE_SEGMENT.fields[f][1] for f in ("p0", "tri", "p1", "edges")] == [0, 12, 16, 28]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_plane_sections\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+,\s+IntPtr \w+,"
                     r"\s+ulong capacity\);", cs) and "public struct PlaneSegment" in cs and "public struct Plane " in cs
    ps = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "PlaneSections.cs")).read())
    assert "lbvh_plane_sections(" in ps and "public void Sections(" in ps
    assert "void PlaneSections(" in open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    drv = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver.cpp")).read()
    assert '{"sections", sections_main}' in drv
    for name in ("plane_sections", "cross_sections"):
        assert hasattr(H().RaytracingMeshDrawer, name)
    for name in ("planes", "section_edges", "stitch_sections"):
        assert callable(getattr(H(), name))
    for doc, must in (("README.md", "lbvh_plane_sections"), ("DESIGN.md", "## 41."), ("INTEGRATION.md", "stitch_sections")):
        assert must in open(os.path.join(ROOT, doc)).read(), doc


def test_host_planes_and_section_edges():
    p = H().planes([[0.0, 0.0, 2.0]], [[1.0, 2.0, 3.0], [0.0, 0.0, -1.0]])
    assert p.dtype == L().PLANE and (p["n"] == [0.0, 0.0, 2.0]).all() and p["d"].tolist() == [-6.0, 2.0]
    word = np.array([0b101 | (2 << 8) | (0 << 12) | (0b011 << 16)], dtype=np.uint32)
    crossing, k0, k1, sides = H().section_edges(word)
    assert crossing.tolist() == [[True, False, True]] and (k0[0], k1[0]) == (2, 0) and sides.tolist() == [[True, True, False]]


def check_records(rec):
    """the record invariants of the header"""
    crossing, k0, k1, sides = H().section_edges(rec)
    assert (crossing.sum(axis=1) == 2).all() and (k0 != k1).all() and (k0 < 3).all() and (k1 < 3).all()
    rows = np.arange(len(rec))
    assert crossing[rows, k0].all() and crossing[rows, k1].all()
    assert (sides.any(axis=1) & ~sides.all(axis=1)).all()
    assert (rec["edges"] & np.uint32(~(0x7 | (0x3 << 8) | (0x3 << 12) | (0x7 << 16)) & 0xFFFFFFFF) == 0).all()
    nxt = np.array([1, 2, 0])
    assert (sides[rows, k0] & ~sides[rows, nxt[k0]]).all() and (~sides[rows, k1] & sides[rows, nxt[k1]]).all()


@pytest.mark.parametrize("name", SCENES + ["one"])
def test_the_restatement_against_float64(name):
    """every end within K * 2^-24 * (|n| extent + |d|) / (|n| |cos|) of the float64 crossing of the original vertices; at most 1 % of
    the ends of any set left out; the sets are not vacuous"""
    a, b, c, lo, hi, sets = cpu_case(name)
    for label, planes, ref in sets:
        check_records(ref.records)
        assert len(ref.offsets) == len(planes) + 1 and int(ref.offsets[-1]) == len(ref.records)
        ratio, out = PS.float64_check(planes, a, b, c, ref)
        finite = np.isfinite(planes["n"]).all(axis=1) & np.isfinite(planes["d"])
        checked_out = out[finite[ref.rows]]
        share = checked_out.mean() if checked_out.size else 0.0
        print(name, label, "records", len(ref.records), "worst ratio %.3f" % (ratio.max() if ratio.size else 0.0), "left out %.4f" % share)
        assert share <= 0.01, (name, label, share)
        assert (ratio <= 1.0).all(), (name, label, ratio.max())
    by = {label: ref for label, planes, ref in sets}
    if len(a) >= 64:
        assert len(by["special"].records) > 50 and len(by["random1500"].records) > 1500
    if name == "grid_80x80":
        zero = by["special"].records
        assert ((zero["p0"] == zero["p1"]).all(axis=1)).sum() > 0                 # a vertex on the plane: zero-length records
    sizes = np.diff(by["special"].offsets).astype(np.int64)
    assert (sizes[-15:] == 0).sum() >= 7                                           # n = 0, NaN planes, d = +-inf: no candidates


def test_a_triangle_in_the_plane_is_not_reported_and_a_vertex_on_it_counts_as_positive():
    a, b, c = (np.array(x, dtype=F) for x in ([[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[1, 0, 0], [1, 0, -1], [1, 0, 1]], [[0, 1, 0], [0, 1, -1], [0, 1, 1]]))
    lo, hi = padded_boxes(a, b, c)
    ref = PS.reference(PS.make_planes(np.array([[0, 0, 1]], dtype=F), np.array([0], dtype=F)), a, b, c, lo, hi)
    assert ref.records["tri"].tolist() == [1]                        # coplanar: none; apex on the plane, rest below: a zero-length record;
    assert (ref.records["p0"] == 0).all() and (ref.records["p1"] == 0).all()       # apex on the plane, rest above: none
    assert H().section_edges(ref.records)[3].tolist() == [[True, False, False]]


@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_stitching_closes_every_contour_the_same_way_round(name):
    """generic planes on a closed, consistently wound mesh: every edge key occurs exactly twice, once as a p0-edge and once as a
    p1-edge; all chains close; on the sphere every loop of a plane turns the same way about n"""
    tris = scene(name)
    a, b, c, lo, hi, sets = cpu_case(name)
    planes, ref = next((p, r) for label, p, r in sets if label == "random65")
    raw = [[v[i].tobytes() for i in range(len(a))] for v in (a, b, c)]
    loops_seen = 0
    for k in range(len(planes)):
        rec = ref.records[int(ref.offsets[k]):int(ref.offsets[k + 1])]
        _, k0, k1, _ = H().section_edges(rec)
        keys = {}
        for r, e0, e1 in zip(rec, k0, k1):
            t = int(r["tri"])
            for kind, e in ((0, int(e0)), (1, int(e1))):
                u, v = raw[e][t], raw[(e + 1) % 3][t]
                keys.setdefault((min(u, v), max(u, v)), []).append(kind)
        assert all(sorted(v) == [0, 1] for v in keys.values()), (name, k)
        loops, chains = H().stitch_sections(rec, tris)
        assert not chains and sum(len(t) for _, t in loops) == len(rec), (name, k)
        assert len(loops) <= (1 if name == "icosphere" else 2)
        n = planes["n"][k].astype(np.float64)
        for pts, _ in loops:
            p = pts.astype(np.float64)
            turn = (np.cross(p, np.roll(p, -1, axis=0)).sum(axis=0) * n).sum()          # twice the signed area about n
            if name == "icosphere":
                assert turn > 0, (k, turn)          # outward winding, p0 on the edge leaving the positive side: counter-clockwise about n
            loops_seen += 1
    assert loops_seen >= 40


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

class Sections:
    """device buffers of one plane set; run() = one lbvh_plane_sections call on caller-owned buffers"""

    def __init__(self, ctx, drawer, planes):
        self.ctx, self.drawer, self.count = ctx, drawer, len(planes)
        self.planes = H().DataBuffer(ctx, max(len(planes), 1), L().PLANE)
        self.planes.local[:len(planes)] = planes
        self.planes.sync()
        self.offsets = H().DataBuffer(ctx, len(planes) + 1, np.uint64)

    def run(self, segments=None, capacity=None, poison=0xDEADBEEF, expect=0):
        self.offsets.fill_u32(poison)
        s = self.drawer.container.scene()
        cap = 0 if segments is None else (segments.size if capacity is None else capacity)
        rc = N().lib.lbvh_plane_sections(self.ctx.handle, self.planes.device, self.count, C.byref(s), self.offsets.device,
                                         segments.device if segments is not None else None, cap)
        assert rc == expect, (rc, N().lib.lbvh_last_error(self.ctx.handle))
        return self.offsets.get_data().copy()

    def lists(self):
        """(offsets, records ordered by tri inside every segment) through count -> allocate -> fill"""
        return self.drawer.cross_sections(self.planes)

    def dispose(self):
        for buf in (self.planes, self.offsets):
            buf.dispose()


class task_cap:
    """lbvh_debug_region_task_cap for a block of calls"""

    def __init__(self, ctx, cap):
        self.h, self.cap = ctx.handle, cap

    def __enter__(self):
        N().check(self.h, N().lib.lbvh_debug_region_task_cap(self.h, self.cap))

    def __exit__(self, *exc):
        N().check(self.h, N().lib.lbvh_debug_region_task_cap(self.h, 0))


def assert_same_records(got, ref, what=""):
    (go, gr), (ro, rr) = got, (ref.offsets, ref.records)
    assert len(go) == len(ro) and (go == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gr) == len(rr) == int(ro[-1]), (what, len(gr), len(rr))
    bad = np.nonzero((PS.record_words(gr) != PS.record_words(rr)).any(axis=1))[0]
    assert len(bad) == 0, (what, bad[:10], gr[bad[:3]], rr[bad[:3]])


_GPU = {}


def gpu_case(ctx, name):
    """(drawer, a, b, c, lo, hi, sets) with the library's boxes; a context keeps one derived traversal scene, so it is derived again
    for the test that asks"""
    if name not in _GPU:
        d = H().RaytracingMeshDrawer(ctx, scene(name)).awake()
        _GPU[name] = (d,) + cpu_case(name, *library_boxes(d))
    _GPU[name][0].build_fast_scene()
    return _GPU[name]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", SCENES)
def test_l1_parity_with_the_restatement(ctx, name, cap):
    d, a, b, c, lo, hi, sets = gpu_case(ctx, name)
    with task_cap(ctx, cap):
        for label, planes, ref in sets:
            q = Sections(ctx, d, planes)
            got = q.lists()
            assert_same_records(got, ref, (name, cap, label))
            check_records(got[1])                                        # L2
            assert (q.run() == ref.offsets).all()                        # the count-only form
            q.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 8])
def test_l3_two_calls_write_the_same_bytes(ctx, cap):
    d, a, b, c, lo, hi, sets = gpu_case(ctx, "example_object3")
    label, planes, ref = sets[-1]
    q = Sections(ctx, d, planes)
    total = int(ref.offsets[-1])
    bufs = [H().DataBuffer(ctx, total, L().PLANE_SEGMENT) for _ in range(2)]
    with task_cap(ctx, cap):
        for buf in bufs:
            buf.fill_u32(POISON)
            assert (q.run(buf) == ref.offsets).all()
    first, second = (buf.get_data().copy() for buf in bufs)
    assert (words(first) == words(second)).all()
    assert_same_records((ref.offsets, PS.sort_segments(ref.offsets, first)), ref)
    for buf in bufs:
        buf.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4, 4096])
def test_l4_the_csr_contract(ctx, cap):
    """cap 4 096: a task of these planes holds a few triangles, so a capacity inside a segment falls between two tasks of one plane;
    cap 4: at most four tasks per plane, so it falls inside a task"""
    d, a, b, c, lo, hi, sets = gpu_case(ctx, "cfg1_4096")
    label, planes, ref = sets[-1]
    assert label == "random1500"
    q = Sections(ctx, d, planes)
    ro, rr = ref.offsets, ref.records
    total, guard = int(ro[-1]), 512
    n = np.diff(ro).astype(np.int64)
    with task_cap(ctx, cap):
        assert (q.run(None) == ro).all()                                 # capacity == 0, d_segments == NULL
        cut = int(np.nonzero((n >= 8) & (ro[:-1] > total // 3))[0][0])
        buf = H().DataBuffer(ctx, total + guard, L().PLANE_SEGMENT)
        for capacity in (int(ro[cut]) + 1, int(ro[cut]) + int(n[cut]) // 2, int(ro[cut + 1]) - 1, int(ro[cut]), total - 1, 1):
            buf.fill_u32(0xABABABAB)
            off = q.run(buf, capacity=capacity)
            got = buf.get_data().copy()
            assert (off == ro).all() and int(off[-1]) == total           # d_offsets[count] still says what was needed
            assert (words(got[capacity:]) == 0xABABABAB).all()           # nothing at the capacity or beyond
            fits = int(np.nonzero(ro <= capacity)[0][-1])                # the segments before this offset fit
            last = int(ro[fits])
            assert (words(PS.sort_segments(ro[:fits + 1], got[:last])) == words(rr[:last])).all()
        buf.fill_u32(0xABABABAB)
        assert (q.run(buf, capacity=total) == ro).all()
        got = buf.get_data().copy()
        assert (words(got[total:]) == 0xABABABAB).all() and (words(PS.sort_segments(ro, got[:total])) == words(rr)).all()
        buf.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0
    q.dispose()


def slab_regions(planes):
    """{n, d}, {-n, -d}, 4 x {0, 0, 0, 1}: the triangles whose boxes touch the plane"""
    r = np.zeros(len(planes), dtype=L().REGION)
    r["plane"][:, 0, :3], r["plane"][:, 0, 3] = planes["n"], planes["d"]
    r["plane"][:, 1, :3], r["plane"][:, 1, 3] = -planes["n"], -planes["d"]
    r["plane"][:, 2:, 3] = 1.0
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grid_80x80", "cfg1_4096"])
def test_l5_candidates_lie_in_the_slab_regions_touching_lists(ctx, name):
    """normals without zero components: every tri of plane k's segment is in segment k of lbvh_region_overlaps_large (TOUCHING) on the
    slab regions, and triangle_tests of the count-only form is that list's total"""
    d, a, b, c, lo, hi, sets = gpu_case(ctx, name)
    label, planes, ref = sets[3]
    assert label == "random63" and (planes["n"] != 0).all()
    regions = Q.Regions(ctx, d, slab_regions(planes))
    off, tris = d.in_regions(regions.regions, L().REGION_TOUCHING, device_sort=True, large=True)
    assert (off[1:].astype(np.int64) - off[:-1].astype(np.int64) == PS.box_candidates(planes, lo, hi)).all()
    for k in range(len(planes)):
        mine = ref.records["tri"][int(ref.offsets[k]):int(ref.offsets[k + 1])]
        assert np.isin(mine, tris[int(off[k]):int(off[k + 1])]).all(), k
    q = Sections(ctx, d, planes)
    stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
    h, lib = ctx.handle, N().lib
    got = []
    for full in (False, True):
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            with task_cap(ctx, 8):
                if full:
                    buf = H().DataBuffer(ctx, int(ref.offsets[-1]), L().PLANE_SEGMENT)
                    assert (q.run(buf) == ref.offsets).all()
                    buf.dispose()
                else:
                    assert (q.run() == ref.offsets).all()
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        got.append({k: int(stats.get_data()[0][k]) for k in ("rays", "node_fetches", "triangle_tests")})
    assert got[0]["triangle_tests"] == int(off[-1]) and got[1]["triangle_tests"] == 2 * int(off[-1]), (got, int(off[-1]))
    assert 0 < got[0]["rays"] <= 8 * len(planes) and got[1]["rays"] == 2 * got[0]["rays"] and got[0]["node_fetches"] >= len(planes)
    for buf in (stats,):
        buf.dispose()
    regions.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_l6_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 planes of 8 task slots on 1, 2, 3 and 7 waves"""
    d, a, b, c, lo, hi, sets = gpu_case(ctx, "grid_80x80")
    label, planes, ref = sets[-1]
    q = Sections(ctx, d, planes)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        with task_cap(ctx, 8):
            got = q.lists()
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    assert_same_records(got, ref, waves)
    assert lib.lbvh_sync(h) == 0
    q.dispose()


@pytest.mark.gpu
def test_l6_the_stack_split_and_the_stack_limit():
    """four tasks per plane with one stack entry in LDS and the rest in device memory: the same records; with one entry in LDS and one
    in device memory the walk cannot keep its waiting siblings: LBVH_FAULT_RAY_STACK at the next lbvh_sync, not a short list"""
    tris = Q.scene("cfg1_4096")
    c2 = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        a, b, c = positions(tris)
        lo, hi = library_boxes(d)
        planes = random_planes(a, b, c, 3)
        ref = PS.reference(planes, a, b, c, lo, hi)
        assert int(np.diff(ref.offsets).min()) >= 20                 # every plane cuts the mesh: walks that keep siblings waiting
        q = Sections(c2, d, planes)
        h, lib = c2.handle, N().lib
        with task_cap(c2, 4):
            assert_same_records(q.lists(), ref)
            N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
            assert_same_records(q.lists(), ref, "split")
            assert lib.lbvh_sync(h) == 0
            N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
            s = d.container.scene()                                   # (no download here: it would report the fault before lbvh_sync does)
            N().check(h, lib.lbvh_plane_sections(h, q.planes.device, 3, C.byref(s), q.offsets.device, None, 0))
            assert lib.lbvh_sync(h) == -3
            assert b"stack" in lib.lbvh_last_error(h)
            N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
            N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
            assert_same_records(q.lists(), ref, "after the stack limit")
        assert lib.lbvh_sync(h) == 0
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_l7_rejections_a_stale_scene_a_failed_allocation_and_count_zero():
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        planes = random_planes(a, b, c, 130)
        ref = PS.reference(planes, a, b, c, lo, hi)
        assert int(ref.offsets[-1]) > 130
        q = Sections(ctx, d, planes)
        seg = H().DataBuffer(ctx, int(ref.offsets[-1]) + 1, L().PLANE_SEGMENT)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        call = lib.lbvh_plane_sections
        assert lib.lbvh_abi_version() == 11
        dq, do, ds = q.planes.device, q.offsets.device, seg.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, seg)
        for buf in bufs:
            buf.fill_u32(POISON)
        assert call(h, dq, 0, C.byref(s), do, ds, 64) == 0                                        # count == 0: a no-op
        for args in ((None, 10, C.byref(s), do, None, 0), (dq, 10, None, do, None, 0), (dq, 10, C.byref(s), None, None, 0),
                     (dq, 10, C.byref(s), do, None, 5), (at(q.planes, 8), 10, C.byref(s), do, None, 0),
                     (dq, 10, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, C.byref(s), do, at(seg, 8), 8),
                     (dq, 65537, C.byref(s), do, None, 0), (dq, 1 << 32, C.byref(s), do, None, 0)):
            assert call(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_plane_sections: "), lib.lbvh_last_error(h)
        assert call(None, dq, 10, C.byref(s), do, None, 0) == -1
        d.container.triangle_data.sync()                               # triangles uploaded without a rebuild: the derived scene is stale
        assert call(h, dq, 130, C.byref(s), do, None, 0) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_plane_sections: ") and b"stale" in msg, msg
        assert all((words(buf.get_data()) == POISON).all() for buf in bufs)                       # nothing above touched a buffer
        d.rebuild(fast=True)
        assert_same_records(q.lists(), ref)
        assert call(h, at(q.planes, 16), 10, C.byref(s), at(q.offsets, 8), at(seg, 32), 8) == 0   # aligned sub-ranges are fine
        # a failed growth of the ray scratch or of the task buffer: the error, and the context goes on
        for kth in (1, 2):
            ctx2 = H().Context(0)
            try:
                d2 = H().RaytracingMeshDrawer(ctx2, tris).awake()
                q2 = Sections(ctx2, d2, planes)
                few = Sections(ctx2, d2, planes[:1])
                with task_cap(ctx2, 4):
                    assert (few.run() == ref.offsets[:2]).all()        # the wide nodes, a small ray scratch and a small task buffer exist
                ctx2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, kth)
                q2.run(expect=-2)
                assert b"LBVH_DEBUG_FAIL_RESERVE" in lib.lbvh_last_error(ctx2.handle)
                assert_same_records(q2.lists(), ref, kth)
                assert lib.lbvh_sync(ctx2.handle) == 0
            finally:
                ctx2.close()
        assert lib.lbvh_sync(h) == 0
        seg.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_l7_the_live_path_list_is_dropped(ctx):
    """a path-traced frame with the call issued between the bounces equals the undisturbed frame"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    count = 160 * 96
    st0 = pt.states.get_data()[:count].copy()
    n = 4 * count                                                    # 61 440 planes, 64 task slots each: the scratch grows in mid-frame
    q = Sections(ctx, pt.drawer, random_planes(*positions(tris), n))
    cam = N().Camera.from_dict(cam_d)
    h, s, lib = ctx.handle, pt.drawer.container.scene(), N().lib

    def sections():
        N().check(h, lib.lbvh_plane_sections(h, q.planes.device, n, C.byref(s), q.offsets.device, None, 0))

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    sections()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        sections()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    sections()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    assert (words(pt.states.get_data()[:count]) == words(st0)).all()
    assert (pt.image().view(np.uint16) == img0.view(np.uint16)).all()
    assert int(q.offsets.get_data()[n]) > n
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
def test_l8_the_cpp_driver(ctx):
    """`lbvh_driver sections 200 7`: PlaneSections of lbvh_host.hpp on the mirrored generator"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    res = json.loads(subprocess.run([exe, "sections", "200", "7"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)
    planes = PS.driver_planes(lo, hi, 200, seed=7)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    off, rec = d.cross_sections(planes)
    ref = PS.reference(planes, pos[:, 0], pos[:, 1], pos[:, 2], *library_boxes(d))
    d.on_destroy()
    assert_same_records((off, rec), ref)
    offset_sum, record_sum = PS.checksums(off, rec)
    assert int(off[-1]) > 1000
    assert (res["triangles"], res["planes"], res["total"], res["non_empty"], res["offset_sum"], res["record_sum"]) == \
        (4096, 200, int(off[-1]), int((np.diff(off) > 0).sum()), offset_sum, record_sum)
