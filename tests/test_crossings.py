"""lbvh_count_hits / lbvh_point_crossings: how many triangles a ray crosses, and crossing parities of points along fixed directions.
The expectation is tests/ray_reference.py: the header's candidate rule in numpy float32, brute force over every (ray, triangle) pair
with the triangles' own boxes as the library produced them — no tree.  Every GPU comparison of a count or a parity word is word for
word.  Inside / outside is checked against the float64 generalised winding number (Van Oosterom & Strackee's solid angle per
triangle) of the same fp32 vertices."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import oracle as O
import point_reference as PR
import ray_reference as RR
from query_support import driver_mesh, driver_points, golden, H, library_boxes, make_rays, N, padded_boxes, positions, words
from unitysimpleraytracing_amd import layouts as L
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)


def make_points(p, r2=INF):
    q = np.zeros(len(p), dtype=L.POINT_QUERY)
    q["p"], q["max_dist2"] = p, r2
    return q


# ---- float64 truth: winding number and distance -------------------------------------------------------------------------

def winding(points, a, b, c, pairs_per_chunk=1 << 22):
    """generalised winding number of each point against the triangles, float64 on the fp32 vertices"""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    pts = np.asarray(points, dtype=np.float64)
    out = np.zeros(len(pts))
    step = max(1, pairs_per_chunk // max(len(a), 1))
    for s in range(0, len(pts), step):
        p = pts[s:s + step, None, :]
        x, y, z = a[None] - p, b[None] - p, c[None] - p
        lx, ly, lz = (np.linalg.norm(v, axis=-1) for v in (x, y, z))
        det = np.einsum("ijk,ijk->ij", x, np.cross(y, z))
        den = lx * ly * lz + np.einsum("ijk,ijk->ij", x, y) * lz + np.einsum("ijk,ijk->ij", y, z) * lx + \
            np.einsum("ijk,ijk->ij", z, x) * ly
        out[s:s + step] = (2.0 * np.arctan2(det, den)).sum(axis=1) / (4.0 * np.pi)
    return out


def truth_inside(points, a, b, c):
    return np.abs(winding(points, a, b, c)) > 0.5


def distance64(points, a, b, c):
    return np.sqrt(PR.nearest_dist2(points, a, b, c, dtype=np.float64))


# ---- the point sets of the vote -------------------------------------------------------------------------------------------

def torus():
    return scenes.tiled_torus(nu=80, nv=50, grid=1)


def vote_sets(a, b, c, seed=7):
    """A: 3 000 uniform in the torus box + 1 000 vertices jittered by N(0, 0.3).  B: 1 500 points a_i - s * d0 and 1 500 points
    (a_i + b_i) / 2 - s * d0, s ~ U(0.5, 8): ray 0 aimed at a vertex or at an edge midpoint."""
    rng = np.random.default_rng(seed)
    lo, hi = np.minimum(np.minimum(a, b), c).min(axis=0), np.maximum(np.maximum(a, b), c).max(axis=0)
    d0 = H().DEFAULT_DIRS[0].astype(np.float64)
    uni = rng.uniform(lo, hi, (3000, 3))
    jit = a[rng.integers(0, len(a), 1000)] + rng.normal(0.0, 0.3, (1000, 3))
    set_a = np.concatenate([uni, jit]).astype(F)
    i = rng.integers(0, len(a), 1500)
    s = rng.uniform(0.5, 8.0, (1500, 1))
    vert = a[i] - s * d0
    k = rng.integers(0, len(a), 1500)
    s2 = rng.uniform(0.5, 8.0, (1500, 1))
    mid = (a[k].astype(np.float64) + b[k]) / 2.0 - s2 * d0
    set_b = np.concatenate([vert, mid]).astype(F)
    return set_a, set_b


_VOTE = {}


def vote_case():
    """(a, b, c, sets, truth, distance, per-direction parities of the reference): computed once"""
    if not _VOTE:
        a, b, c = positions(torus())
        lo, hi = padded_boxes(a, b, c)
        dirs = H().DEFAULT_DIRS
        out = {}
        for name, pts in zip("AB", vote_sets(a, b, c)):
            ref = RR.reference(RR.crossing_rays(pts, dirs), a, b, c, lo, hi)
            out[name] = dict(points=pts, truth=truth_inside(pts, a, b, c), dist=distance64(pts, a, b, c),
                             parity=RR.parity_words(ref.counts, len(dirs)))
        _VOTE.update(a=a, b=b, c=c, sets=out)
    return _VOTE


# ---- CPU: the surface in every host ------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lbvh.h")).read(), flags=re.S)


def test_header_declares_both_calls():
    text = _header()
    norm = lambda s: [re.sub(r"\s+", " ", x).strip() for x in s.split(",")]
    count = re.search(r"lbvh_status lbvh_count_hits\s*\(([^;]*)\)\s*;", text, flags=re.S).group(1)
    assert norm(count) == ["lbvh_context* ctx", "const lbvh_ray* d_rays", "size_t count", "const lbvh_scene* h_scene", "uint32_t* d_counts"]
    cross = re.search(r"lbvh_status lbvh_point_crossings\s*\(([^;]*)\)\s*;", text, flags=re.S).group(1)
    assert norm(cross) == ["lbvh_context* ctx", "const lbvh_point_query* d_points", "size_t count", "const float* h_dirs",
                           "uint32_t n_dirs", "const lbvh_scene* h_scene", "uint32_t* d_parity"]
    assert re.search(r"#define LBVH_CROSSING_MAX_DIRS 32\b", text)
    assert "#define LBVH_ABI_VERSION 11" in text


def test_native_prototypes_and_csharp_imports():
    n = N()
    assert n.SIGNATURES["lbvh_count_hits"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(n.Scene), C.c_void_p])
    assert n.SIGNATURES["lbvh_point_crossings"] == (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.c_uint32,
                                                                C.POINTER(n.Scene), C.c_void_p])
    for fn in ("lbvh_count_hits", "lbvh_point_crossings"):
        assert getattr(n.lib, fn).argtypes == n.SIGNATURES[fn][1]
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_count_hits\(IntPtr ctx, IntPtr \w+, UIntPtr count, ref Scene scene, IntPtr \w+\);", cs)
    assert re.search(r"public static extern int lbvh_point_crossings\(IntPtr ctx, IntPtr \w+, UIntPtr count, float\[\] \w+, uint \w+, "
                     r"ref Scene scene,\s+IntPtr \w+\);", cs)
    cr = open(os.path.join(ROOT, "bindings", "csharp", "Crossings.cs")).read()
    assert "lbvh_count_hits" in cr and "lbvh_point_crossings" in cr and "unsafe" not in cr
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert "void CountHits(" in hpp and "void PointCrossings(" in hpp


def test_default_dirs_and_inside():
    d = H().DEFAULT_DIRS
    assert d.dtype == np.float32 and d.shape == (3, 3)
    want = np.array([[1, 1, 1], [-1, 2, 3], [4, -1, 2]], dtype=np.float64)
    assert (d == (want / np.linalg.norm(want, axis=1, keepdims=True)).astype(F)).all()
    p = np.array([0b000, 0b001, 0b011, 0b101, 0b111, 0b110, 0b1000], dtype=np.uint32)
    assert (H().inside(p, 3) == [False, False, True, True, True, True, False]).all()
    assert (H().inside(np.array([1, 0], dtype=np.uint32), 1) == [True, False]).all()


# ---- CPU: the reference against the C oracle, and the vote on the reference alone -----------------------------------------

def _scene(name):
    if name == "random":
        return scenes.random_triangles(4096)
    if name == "grid":
        return scenes.grid_scene()
    if name == "torus":
        return torus()
    if name == "duplicates":
        base = scenes.random_triangles(n=2000, seed=6, extent=40.0, edge=8.0)
        return np.concatenate([base, base[::2]])                   # every second triangle twice: exact t ties
    return golden(name)


def _random_rays(a, b, c, count, rng):
    """origins in the scene's box (half of them on vertices), random directions, a tenth along an axis (zero components)"""
    pts = np.concatenate([a, b, c])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    o = (lo + (hi - lo) * rng.random((count, 3))).astype(F)
    on = rng.random(count) < 0.5
    o[on] = a[rng.integers(0, len(a), on.sum())]
    d = rng.normal(size=(count, 3))
    axis = rng.random(count) < 0.1
    d[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-1.0, 1.0], axis.sum())[:, None]
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


@pytest.mark.parametrize("name", ["random", "grid", "example_object3", "viking_room"])
def test_reference_closest_equals_the_oracle(name):
    tris = _scene(name)
    a, b, c = positions(tris)
    bo = O.Built(tris, threads=8)
    box = bo.triangle_aabb[: len(tris)]
    o, d = _random_rays(a, b, c, 1500, np.random.default_rng(len(tris)))
    t_min = np.random.default_rng(1).choice(np.array([1e-3, 0.0, -3.0e38], dtype=F), len(o))
    ref = RR.reference(make_rays(o, d, t_min, INF), a, b, c, box["min"], box["max"])
    st = np.zeros(len(o), dtype=L.PATH_STATE)
    st["origin"], st["dir"], st["alive"] = o, d, 1
    want = np.empty(len(o), dtype=L.HIT)
    for tm in np.unique(t_min):
        sel = t_min == tm
        want[sel] = O.trace_rays(bo, st[sel], float(tm), threads=8)
    assert (words(ref.records) == words(want)).all()
    hit = want["t"] < L.MAX_FLOAT
    assert ((ref.counts >= 1) == hit).all() and (ref.flags == hit).all()
    assert hit.sum() > 100


def test_the_vote_on_the_reference_alone():
    """The cap: the majority over DEFAULT_DIRS disagrees with the winding number on 0 points farther than 1e-3 from the mesh.  The
    contrast: at least 100 aimed points (set B) have a wrong single-direction parity."""
    v = vote_case()
    for name, s in v["sets"].items():
        far = s["dist"] > 1e-3
        maj = H().inside(s["parity"], 3)
        wrong = (maj != s["truth"]) & far
        single = np.zeros(len(maj), dtype=bool)
        for j in range(3):
            single |= (((s["parity"] >> np.uint32(j)) & np.uint32(1)) == 1) != s["truth"]
        print(f"set {name}: {len(maj)} points, {int(far.sum())} far, {int(s['truth'].sum())} inside, majority wrong "
              f"{int(wrong.sum())}, >= 1 direction wrong {int((single & far).sum())}")
        assert wrong.sum() == 0
        assert 0 < s["truth"].sum() < len(maj)
        if name == "B":
            assert (single & far).sum() >= 100


# ---- GPU ------------------------------------------------------------------------------------------------------------

class Rays:
    def __init__(self, ctx, drawer, rays):
        self.ctx, self.drawer = ctx, drawer
        self.rays = H().DataBuffer(ctx, len(rays), L.RAY)
        self.rays.local[:] = rays
        self.rays.sync()
        self.out = H().DataBuffer(ctx, len(rays), np.uint32)
        self.hits = H().DataBuffer(ctx, len(rays), L.HIT)

    def count(self):
        self.out.fill_u32(0xDEADBEEF)
        self.drawer.count_hits(self.rays, self.out)
        return self.out.get_data().copy()

    def occluded(self):
        self.out.fill_u32(0xDEADBEEF)
        self.drawer.trace_occluded(self.rays, self.out)
        return self.out.get_data().copy()

    def closest(self):
        self.hits.fill_u32(0x7FC00000)
        self.drawer.trace_closest(self.rays, self.hits)
        return self.hits.get_data().copy()

    def dispose(self):
        for b in (self.rays, self.out, self.hits):
            b.dispose()


class Points:
    def __init__(self, ctx, drawer, points):
        self.drawer = drawer
        self.points = H().DataBuffer(ctx, len(points), L.POINT_QUERY)
        self.points.local[:] = points
        self.points.sync()
        self.parity = H().DataBuffer(ctx, len(points), np.uint32)

    def crossings(self, dirs=None):
        self.parity.fill_u32(0xDEADBEEF)                 # the call writes every word: no pre-zeroing
        self.drawer.point_crossings(self.points, self.parity, dirs)
        return self.parity.get_data().copy()

    def dispose(self):
        self.points.dispose()
        self.parity.dispose()


def mixed_rays(a, b, c, count, seed, closest_of):
    """random rays, a third of the directions scaled by 0.25 .. 8, a third aimed at a vertex or an edge midpoint from up to 8 units
    away; per-ray t_min in {1e-3, 0, 0.5, -3e38}; t_max: +inf, MAX_FLOAT, finite around the closest t, exactly that t and one ulp
    above it; inactive rays with t_max <= t_min and with NaN bounds"""
    rng = np.random.default_rng(seed)
    o, d = _random_rays(a, b, c, count, rng)
    scale = rng.random(count) < 0.33
    d[scale] *= rng.uniform(0.25, 8.0, scale.sum()).astype(F)[:, None]
    aim = rng.random(count) < 0.33
    k = rng.integers(0, len(a), count)
    target = np.where((rng.random(count) < 0.5)[:, None], a[k].astype(np.float64), (a[k].astype(np.float64) + b[k]) / 2.0)
    back = rng.uniform(0.5, 8.0, (count, 1)) * d
    o = np.where(aim[:, None], (target - back).astype(F), o)
    t_min = rng.choice(np.array([1e-3, 0.0, 0.5, -3.0e38], dtype=F), count)
    rays = make_rays(o, d, t_min, INF)
    t = closest_of(rays)["t"]
    hit = t < L.MAX_FLOAT
    kind = rng.integers(0, 8, count)
    span = np.where(hit, t, F(30.0))
    t_max = np.full(count, INF, dtype=F)
    t_max = np.where(kind == 0, (span * rng.uniform(0.5, 1.5, count)).astype(F), t_max)
    t_max = np.where(kind == 1, L.MAX_FLOAT, t_max)
    t_max = np.where((kind == 2) & hit, t, t_max)
    t_max = np.where((kind == 3) & hit, np.nextafter(t, INF), t_max)
    t_max = np.where(kind == 4, t_min, t_max)
    rays["t_max"] = t_max
    rays["t_min"] = np.where(kind == 5, F(np.nan), rays["t_min"])
    rays["t_max"] = np.where((kind == 6) & (rng.random(count) < 0.5), F(np.nan), rays["t_max"])
    return rays, aim, t


COUNT_SCENES = ["random", "grid", "example_object3", "viking_room", "torus", "duplicates"]
_CASES = {}


def count_case(ctx, name):
    if name not in _CASES:
        tris = _scene(name)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        a, b, c = positions(tris)
        lo, hi = library_boxes(d)
        rays, aim, t_open = mixed_rays(a, b, c, 3000, 11 + len(tris), lambda r: RR.reference(r, a, b, c, lo, hi).records)
        _CASES[name] = (d, rays, aim, RR.reference(rays, a, b, c, lo, hi), t_open)
    _CASES[name][0].build_fast_scene()
    return _CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNT_SCENES)
def test_count_equals_the_brute_force_on_every_walker(ctx, name):
    d, rays, aim, ref, t_open = count_case(ctx, name)
    q = Rays(ctx, d, rays)
    lib, h = N().lib, ctx.handle
    try:
        for walker in (0, 1, 2):
            N().check(h, lib.lbvh_debug_ray_walker(h, walker))
            for split in (16, 2):
                N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
                got = q.count()
                bad = np.nonzero(got != ref.counts)[0]
                assert len(bad) == 0, (walker, split, bad[:10], got[bad[:5]], ref.counts[bad[:5]])
    finally:
        N().check(h, lib.lbvh_debug_ray_walker(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    assert ((got >= 1) == (q.occluded() == 1)).all()
    assert (words(q.closest()) == words(ref.records)).all()
    q.dispose()
    act = RR.active(rays)
    hist = np.bincount(np.minimum(ref.counts[act], 3), minlength=4)
    t = t_open                                                       # the closest t with t_max = +inf
    at_t = act & (t < L.MAX_FLOAT) & (rays["t_max"] == t)
    above = act & (t < L.MAX_FLOAT) & (rays["t_max"] == np.nextafter(t, INF))
    print(f"{name}: counts 0/1/2/>=3 {hist.tolist()}, inactive {int((~act).sum())}, ties {int((ref.ties >= 2).sum())}, "
          f"aimed ties {int((aim & (ref.ties >= 2)).sum())}, t_max at t {int(at_t.sum())}, one ulp above {int(above.sum())}")
    assert (hist > 0).all() if name != "grid" else (hist[:3] > 0).all()
    assert (~act).sum() > 300 and (ref.counts[~act] == 0).all()
    assert np.isnan(rays["t_min"]).sum() > 100 and np.isnan(rays["t_max"]).sum() > 50
    assert (rays["dir"] == 0).any(axis=1).sum() > 100
    assert at_t.sum() > 0 and above.sum() > 0
    assert (ref.counts[at_t] == 0).all() and (ref.counts[above] >= 1).all()
    if name in ("grid", "torus", "example_object3", "viking_room"):
        assert (aim & (ref.ties >= 2)).sum() > 0                   # a ray through a shared edge or vertex counts every triangle
    if name == "duplicates":
        assert (ref.ties >= 2).sum() > 100


@pytest.mark.gpu
def test_count_statistics_and_occlusion_never_walk_more(ctx):
    d, rays, aim, ref, _ = count_case(ctx, "torus")
    q = Rays(ctx, d, rays)
    stats = H().DataBuffer(ctx, 1, L.RAY_STATS)
    lib, h = N().lib, ctx.handle
    per = {}
    try:
        for walker in (1, 2):
            N().check(h, lib.lbvh_debug_ray_walker(h, walker))
            for call in ("closest", "occluded", "count"):
                stats.fill_u32(0)
                N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
                getattr(q, call)()
                N().check(h, lib.lbvh_ray_stats_target(h, None))
                per[(walker, call)] = stats.get_data()[0].copy()
    finally:
        N().check(h, lib.lbvh_ray_stats_target(h, None))
        N().check(h, lib.lbvh_debug_ray_walker(h, 1))
    n_active = int(RR.active(rays).sum())
    for walker in (1, 2):
        cl, cn = per[(walker, "closest")], per[(walker, "count")]
        print(f"walker {walker}: closest {int(cl['node_fetches'])} / {int(cl['triangle_tests'])}, count {int(cn['node_fetches'])} / "
              f"{int(cn['triangle_tests'])}")
        assert int(cn["rays"]) == n_active
        assert int(cn["node_fetches"]) >= int(cl["node_fetches"]) and int(cn["triangle_tests"]) >= int(cl["triangle_tests"])
    # crossings: one ray per (point, direction)
    v = vote_case()
    pts = v["sets"]["A"]["points"]
    p = Points(ctx, d, make_points(pts))
    stats.fill_u32(0)
    N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
    p.crossings()
    N().check(h, lib.lbvh_ray_stats_target(h, None))
    assert int(stats.get_data()[0]["rays"]) == 3 * len(pts)
    p.dispose()
    stats.dispose()
    q.dispose()


def _point_buffer(a, b, c, rng):
    """a lbvh_closest_point_query buffer as a caller would pass it: mixed radii (+inf, finite, 0, -1, NaN) and NaN coordinates"""
    lo, hi = np.minimum(np.minimum(a, b), c).min(axis=0), np.maximum(np.maximum(a, b), c).max(axis=0)
    pts = rng.uniform(lo - 2.0, hi + 2.0, (1200, 3)).astype(F)
    pts[rng.random(1200) < 0.05, rng.integers(0, 3)] = np.nan
    r2 = rng.choice(np.array([np.inf, 4.0, 0.0, -1.0, np.nan], dtype=F), 1200)
    return make_points(pts, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", [1, 3, 32])
def test_crossings_equal_the_brute_force_bits(ctx, n_dirs):
    """n_dirs = 1 and 3: every point of the vote's sets A and B and of a closest-point buffer; 32 directions (32 rays per point,
    brute force ~16 s per 512 points): every eighth point of A and B and the whole closest-point buffer"""
    v = vote_case()
    a, b, c = v["a"], v["b"], v["c"]
    d, *_ = count_case(ctx, "torus")
    lo, hi = library_boxes(d)
    rng = np.random.default_rng(30 + n_dirs)
    dirs = H().DEFAULT_DIRS[:n_dirs] if n_dirs <= 3 else rng.normal(size=(n_dirs, 3)).astype(F)
    if n_dirs == 32:
        dirs[5] = (0.0, 0.0, -2.0)                                        # zero components
        dirs[6] = (3.0, 0.0, 0.0)
    buf = _point_buffer(a, b, c, rng)
    sets = [make_points(v["sets"][k]["points"]) for k in "AB"]
    if n_dirs == 32:
        sets = [s[::8] for s in sets]
    for pts in sets + [buf]:
        want = RR.parity_words(RR.reference(RR.crossing_rays(pts["p"], dirs), a, b, c, lo, hi).counts, n_dirs)
        p = Points(ctx, d, pts)
        got = p.crossings(dirs)
        p.dispose()
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (bad[:10], got[bad[:5]], want[bad[:5]])
        assert (got >> np.uint32(n_dirs) == 0).all() if n_dirs < 32 else True
        assert 0 < (got != 0).sum() < len(got)
    nan_pts = np.isnan(buf["p"]).any(axis=1)
    assert nan_pts.sum() > 20 and (got[nan_pts] == 0).all()


@pytest.mark.gpu
def test_inside_equals_truth_on_the_torus_sets(ctx):
    v = vote_case()
    d, *_ = count_case(ctx, "torus")
    for name, s in v["sets"].items():
        p = Points(ctx, d, make_points(s["points"]))
        got = p.crossings()
        p.dispose()
        assert (got == s["parity"]).all()
        far = s["dist"] > 1e-3
        wrong = (H().inside(got, 3) != s["truth"]) & far
        print(f"set {name}: majority wrong on {int(wrong.sum())} of {int(far.sum())} far points")
        assert wrong.sum() == 0


@pytest.mark.gpu
def test_inside_equals_truth_on_one_million_triangles(ctx):
    """cfg2's mesh; 4 096 points in the bounding balls of random tiles (radius 19: one tile each, 7.5 units from every other),
    half uniform, half jittered vertices of that tile.  Truth: the winding number against the point's own tile, float64."""
    tris, body, centres = scenes.tiled_torus(with_bodies=True)
    a, b, c = positions(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    rng = np.random.default_rng(9)
    n = 4096
    tile = rng.integers(0, len(centres), n)
    r = 19.0 * rng.random(n) ** (1.0 / 3.0)
    u = rng.normal(size=(n, 3))
    pts = centres[tile, :3] + u / np.linalg.norm(u, axis=1, keepdims=True) * r[:, None]
    for k in np.nonzero(rng.random(n) < 0.5)[0]:
        own = np.nonzero(body == tile[k])[0]
        pts[k] = a[own[rng.integers(0, len(own))]] + rng.normal(0.0, 0.3, 3)
    pts = pts.astype(F)
    p = Points(ctx, d, make_points(pts))
    got = p.crossings()
    p.dispose()
    d.on_destroy()
    truth = np.zeros(n, dtype=bool)
    dist = np.zeros(n)
    for t in np.unique(tile):
        sel = tile == t
        own = body == t
        truth[sel] = truth_inside(pts[sel], a[own], b[own], c[own])
        dist[sel] = distance64(pts[sel], a[own], b[own], c[own])
    far = dist > 1e-3
    wrong = (H().inside(got, 3) != truth) & far
    print(f"1 M triangles: {int(truth.sum())} inside, majority wrong on {int(wrong.sum())} of {int(far.sum())} far points")
    assert 500 < truth.sum() < n - 500
    assert wrong.sum() == 0


@pytest.mark.gpu
def test_identities_at_scale(ctx):
    """1 M triangles, 2^20 first-bounce rays and 2^20 shadow rays: count >= 1 <=> occluded; the count up to the closest t* is 0
    and up to nextafter(t*) >= 1; count(a, b) == count(a, m) + count(nextafter(m, -inf), b)"""
    W, Ht = 1024, 1024
    tris, body, centres = scenes.tiled_torus(with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=9)
    pt.animate(0.03)
    cam = scenes.camera(W, Ht, (0.0, 0.0, 250.0))
    pt.render(cam, bounces=1)
    c_ = N().Camera.from_dict(cam)
    h, s = ctx.handle, pt.drawer.container.scene()
    N().check(h, N().lib.lbvh_trace_primary(h, C.byref(c_), 0, 0, W, Ht, C.byref(s), L.TRACE_FAST, pt.hits.device, None))
    prim = pt.hits.get_data()[: W * Ht].copy()
    N().check(h, N().lib.lbvh_path_first_bounce(h, C.byref(c_), C.byref(s), pt.states.device, pt.hits.device, 9, 0.7, 1e-3))
    st = pt.states.get_data()[: W * Ht].copy()
    live = st["alive"] != 0
    first = make_rays(st["origin"], st["dir"], F(1e-3), np.where(live, INF, F(0.0)))
    st0 = O.path_begin(cam)
    hit = prim["t"] < L.MAX_FLOAT
    origin = (st0["origin"] + st0["dir"] * prim["t"][:, None]).astype(F)
    light = np.array([0.0, 250.0, 150.0], dtype=F)
    shadow = make_rays(origin, (light - origin).astype(F), F(1e-4), np.where(hit, F(1.0), F(0.0)))
    for name, rays in (("first bounce", first), ("shadow", shadow)):
        q = Rays(ctx, pt.drawer, rays)
        cnt, occ, cl = q.count(), q.occluded(), q.closest()
        assert ((cnt >= 1) == (occ == 1)).all()
        t = cl["t"]
        hit_ = RR.active(rays) & (t < L.MAX_FLOAT)
        assert hit_.sum() > 10000, name
        r2 = rays.copy()
        r2["t_max"] = np.where(hit_, t, r2["t_max"])
        q.rays.local[:] = r2
        q.rays.sync()
        assert (q.count()[hit_] == 0).all()
        r2["t_max"] = np.where(hit_, np.nextafter(t, INF), r2["t_max"])
        q.rays.local[:] = r2
        q.rays.sync()
        assert (q.count()[hit_] >= 1).all()
        # additivity over a split inside the range
        act = RR.active(rays)
        lo_t = np.where(rays["t_min"] > 0, rays["t_min"], F(0.0))
        hi_t = np.minimum(rays["t_max"], F(400.0))
        m = (lo_t + (hi_t - lo_t) * np.random.default_rng(3).uniform(0.2, 0.8, len(rays)).astype(F)).astype(F)
        m = np.where(act, m, rays["t_max"])
        left = rays.copy()
        left["t_max"] = m
        right = rays.copy()
        right["t_min"] = np.where(act, np.nextafter(m, -INF), rays["t_min"])
        parts = []
        for r in (left, right):
            q.rays.local[:] = r
            q.rays.sync()
            parts.append(q.count())
        whole = cnt
        assert (whole[act] == (parts[0] + parts[1])[act]).all(), name
        print(f"{name}: {int(act.sum())} active, counts 0/1/2/>=3 {np.bincount(np.minimum(whole[act], 3), minlength=4).tolist()}")
        q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
def test_errors_stale_scene_and_scratch_failure(ctx):
    tris = scenes.tiled_torus(nu=16, nv=10, grid=2)
    a, b, c = positions(tris)
    c2 = H().Context(0)                               # a context of its own: its ray scratch has never grown
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(2)
        o, dr = _random_rays(a, b, c, 3000, rng)
        rays = make_rays(o, dr, F(1e-3), INF)
        ref = RR.reference(rays, a, b, c, lo, hi)
        pts = make_points(o)
        want_p = RR.parity_words(RR.reference(RR.crossing_rays(o, H().DEFAULT_DIRS), a, b, c, lo, hi).counts, 3)
        q, p = Rays(c2, d, rays), Points(c2, d, pts)
        lib, h, s = N().lib, c2.handle, d.container.scene()
        n = len(rays)
        dirs = np.ascontiguousarray(H().DEFAULT_DIRS)
        fp = lambda x: np.ascontiguousarray(x, dtype=F).ctypes.data_as(C.POINTER(C.c_float))
        # a failed growth of the ray scratch: out of memory, nothing written; the next call on the context succeeds
        for call in ("count", "crossings"):
            c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 1)
            q.out.fill_u32(0xDEADBEEF)
            p.parity.fill_u32(0xDEADBEEF)
            if call == "count":
                assert lib.lbvh_count_hits(h, q.rays.device, n, C.byref(s), q.out.device) == -2
            else:
                assert lib.lbvh_point_crossings(h, p.points.device, n, fp(dirs), 3, C.byref(s), p.parity.device) == -2
            assert (q.out.get_data() == 0xDEADBEEF).all() and (p.parity.get_data() == 0xDEADBEEF).all()
            c2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, 0)
        assert (q.count() == ref.counts).all()
        assert (p.crossings() == want_p).all()
        # argument checks
        ptr = lambda buf, k: C.c_void_p(buf.device.value + k)
        cnt = lambda *args: lib.lbvh_count_hits(*args)
        assert cnt(h, None, n, C.byref(s), q.out.device) == -1
        assert cnt(h, q.rays.device, n, None, q.out.device) == -1
        assert cnt(h, q.rays.device, n, C.byref(s), None) == -1
        assert cnt(h, ptr(q.rays, 32), 10, C.byref(s), q.out.device) == 0
        assert cnt(h, ptr(q.rays, 8), 10, C.byref(s), q.out.device) == -1
        assert cnt(h, q.rays.device, 10, C.byref(s), ptr(q.out, 2)) == -1
        assert cnt(h, q.rays.device, 1 << 32, C.byref(s), q.out.device) == -1
        assert cnt(None, q.rays.device, 10, C.byref(s), q.out.device) == -1
        cr = lambda pts_, k, dv, nd, sc, out: lib.lbvh_point_crossings(h, pts_, k, dv, nd, sc, out)
        S = C.byref(s)
        assert cr(None, 10, fp(dirs), 3, S, p.parity.device) == -1
        assert cr(p.points.device, 10, None, 3, S, p.parity.device) == -1
        assert cr(p.points.device, 10, fp(dirs), 3, None, p.parity.device) == -1
        assert cr(p.points.device, 10, fp(dirs), 3, S, None) == -1
        assert cr(ptr(p.points, 16), 10, fp(dirs), 3, S, p.parity.device) == 0
        assert cr(ptr(p.points, 8), 10, fp(dirs), 3, S, p.parity.device) == -1
        assert cr(p.points.device, 10, fp(dirs), 3, S, ptr(p.parity, 2)) == -1
        assert cr(p.points.device, 1 << 32, fp(dirs), 3, S, p.parity.device) == -1
        assert lib.lbvh_point_crossings(None, p.points.device, 10, fp(dirs), 3, S, p.parity.device) == -1
        big = np.tile(dirs, (11, 1))
        assert cr(p.points.device, 10, fp(big), 0, S, p.parity.device) == -1
        assert cr(p.points.device, 10, fp(big), 33, S, p.parity.device) == -1
        assert cr(p.points.device, 10, fp(big), 32, S, p.parity.device) == 0
        for bad in ((np.nan, 1.0, 0.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 1.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
            dd = dirs.copy()
            dd[1] = bad
            assert cr(p.points.device, 10, fp(dd), 3, S, p.parity.device) == -1, bad
        # count == 0: a no-op, the outputs untouched
        q.out.fill_u32(0xDEADBEEF)
        p.parity.fill_u32(0xDEADBEEF)
        assert cnt(h, q.rays.device, 0, C.byref(s), q.out.device) == 0
        assert cr(p.points.device, 0, fp(dirs), 3, S, p.parity.device) == 0
        assert (q.out.get_data() == 0xDEADBEEF).all() and (p.parity.get_data() == 0xDEADBEEF).all()
        # a stale scene: triangles uploaded without a rebuild
        d.container.triangle_data.sync()
        assert cnt(h, q.rays.device, n, C.byref(s), q.out.device) == -1
        assert b"stale" in lib.lbvh_last_error(h)
        assert cr(p.points.device, n, fp(dirs), 3, S, p.parity.device) == -1
        assert b"stale" in lib.lbvh_last_error(h)
        d.rebuild(fast=True)
        assert (q.count() == ref.counts).all() and (p.crossings() == want_p).all()
        q.dispose()
        p.dispose()
        d.on_destroy()
    finally:
        c2.close()


@pytest.mark.gpu
def test_path_tracer_frame_undisturbed_by_counts_and_crossings_between_bounces(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    st0 = pt.states.get_data()[: 160 * 96].copy()
    # the same frame with both calls issued between the bounces, 4x the frame's count: the ray scratch grows in mid-frame
    a, b, c = positions(tris)
    o, dr = _random_rays(a, b, c, 4 * 160 * 96, np.random.default_rng(12))
    q = Rays(ctx, pt.drawer, make_rays(o, dr, F(1e-3), F(60.0)))
    p = Points(ctx, pt.drawer, make_points(o))
    cam = N().Camera.from_dict(cam_d)
    count = 160 * 96
    h, s = ctx.handle, pt.drawer.container.scene()
    lib = N().lib

    def both():
        pt.drawer.count_hits(q.rays, q.out)
        pt.drawer.point_crossings(p.points, p.parity)

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L.TRACE_FAST, pt.hits.device, None))
    both()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        both()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    both()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    img1 = pt.image()
    st1 = pt.states.get_data()[:count]
    assert (words(st1) == words(st0)).all()
    assert (img1.view(np.uint16) == img0.view(np.uint16)).all()
    assert q.out.get_data().sum() > 0 and 0 < (p.parity.get_data() != 0).sum() < len(o)
    q.dispose()
    p.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
def test_cpp_host_driver_crossings_matches_the_python_host(ctx):
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    n, count = 4096, 20000
    res = json.loads(subprocess.run([exe, "crossings", str(n), str(count)], check=True, capture_output=True, text=True).stdout)
    tris, _, lo, hi = driver_mesh(n)                                   # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    pts = driver_points(lo, hi, count)                                 # and its points (seed 2)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    p = Points(ctx, d, make_points(pts))
    q = Rays(ctx, d, RR.crossing_rays(pts, H().DEFAULT_DIRS))
    parity, counts = p.crossings(), q.count()
    assert (RR.parity_words(counts, 3) == parity).all()
    assert res["triangles"] == n and res["points"] == count and res["consistent"] is True
    assert res["count_sum"] == int(counts.astype(np.uint64).sum()) > 0
    assert res["parity_sum"] == int(parity.astype(np.uint64).sum()) > 0
    assert res["inside"] == int(H().inside(parity, 3).sum())
    p.dispose()
    q.dispose()
    d.on_destroy()
