"""lbvh_region_overlaps / lbvh_region_overlaps_any: which triangles lie in a convex region bounded by six planes, as a CSR list and as
a flag, over the four-wide derived traversal scene.  The expectation is tests/region_reference.py: the header's definition in numpy
float32 over every (region, triangle) pair, with the triangles' own boxes as the library produced them — no tree.  The order inside a
segment is not part of the contract, so every GPU comparison is word for word AFTER lbvh_sort_index_segments or a host sort of each
segment.
  CPU  the surface in every host; the reference against a float64 max / min over the eight corners on dyadic inputs; CONTAINED within
       TOUCHING and the monotonicity claim on random fp32 inputs; the three plane builders; the parity sets are not vacuous
  R1   parity on grid_80x80, example_object3, cfg1_4096       R2  the CSR contract
  R3   aabb_planes == lbvh_box_overlaps on a dyadic mesh; CONTAINED within TOUCHING
  R4   wave caps (the lane refill), counts across a scan-tile border, the stack limit
  R5   the entry contract: count == 0, every rejection, a stale scene, the live-path list
  R6   in_regions(device_sort=True) == in_regions() sorted on the host       R7  lbvh_driver regions: the C++ host end to end"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_reference as V
import region_reference as R
from query_support import driver_mesh, golden, H, L, library_boxes, N, padded_boxes, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNT = 1500
MESHES = ["grid_80x80", "example_object3", "cfg1_4096"]
MODES = [R.TOUCHING, R.CONTAINED]
POISON = 0x7FC0DEAD


def scene(name):
    """grid_80x80 and cfg1_4096 from the seeded generators that made the goldens (tests/test_gpu_parity.py checks they still do)"""
    if name == "grid_80x80":
        return scenes.grid_scene()
    if name == "cfg1_4096":
        return scenes.random_triangles(4096, seed=1)
    return golden(name)


# ---- the mixed regions of the parity sets ------------------------------------------------------------------------------------------

def _rotations(rng, count):
    q, r = np.linalg.qr(rng.normal(size=(count, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _look_at(eye, target):
    """camera_to_world matrices (row-major 4 x 4) of cameras at `eye` whose -z axis points at `target`"""
    z = eye - target
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    up = np.where(np.abs(z[:, 1:2]) < 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    x = np.cross(up, z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    m = np.zeros((len(eye), 4, 4))
    m[:, :3, 0], m[:, :3, 1], m[:, :3, 2], m[:, :3, 3], m[:, 3, 3] = x, y, z, eye, 1.0
    return m


def mixed_regions(a, b, c, lo, hi, count=COUNT, seed=17):
    """One interleaved buffer.  Around (or aimed at) a random triangle each, sizes log-uniform from half a triangle to the whole mesh:
    0 rotated boxes (obb_planes)          1 thin frusta (frustum_planes of an 8 x 8 pixel tile of a 64 x 64 image)
    2 slabs padded with {0, 0, 0, 1}      3 one plane repeated six times (a half space)
    4 axis-aligned boxes with -0 normals  5 boxes whose face is exactly a triangle box's face (aabb_planes from the library's
    boxes: P == 0 exactly), every other one moved one float beyond it
    6 empty regions: two opposed planes with a gap of the mesh's extent, or a small box far outside
    7 a rotated box with NaN, +inf or -inf in one word of n or in d"""
    rng = np.random.default_rng(seed + len(a))
    slo, shi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    ext = float((shi - slo).max())
    k = rng.integers(0, len(a), count)
    centre = ((a[k].astype(np.float64) + b[k]) + c[k]) / 3.0
    tri = np.maximum(np.linalg.norm((hi[k] - lo[k]).astype(np.float64), axis=1), 1e-3 * ext)
    size = tri * 0.5 * (1.5 * ext / (tri * 0.5)) ** (rng.random(count) ** 2)        # half of them below a tenth of the way up in log scale
    kind = rng.choice(8, count, p=[0.36, 0.14, 0.08, 0.05, 0.07, 0.08, 0.14, 0.08])
    rot = _rotations(rng, count)
    half = size[:, None] * rng.uniform(0.5, 1.5, (count, 3))
    planes = H().obb_planes(centre, rot, half)["plane"].copy()                     # kinds 0 and 7 start from these
    pad = np.array(R.PAD, dtype=F)
    # 1: frusta
    idx = np.nonzero(kind == 1)[0]
    d = rng.normal(size=(len(idx), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = size[idx] * rng.uniform(2.0, 6.0, len(idx))
    mats = _look_at(centre[idx] + d * dist[:, None], centre[idx])
    for j, i in enumerate(idx):
        cam = {"screen_width": 64, "screen_height": 64, "camera_fov": 0.5, "near_plane": float(0.1 * dist[j]), "camera_to_world": mats[j].astype(F)}
        x0, y0 = rng.integers(16, 40, 2)
        planes[i] = H().frustum_planes(cam, far=float(dist[j] * rng.uniform(1.0, 3.0)), rect=(x0, y0, x0 + 8, y0 + 8))["plane"][0]
    # 2: slabs, 3: half spaces, 6 (even): opposed planes with a gap
    n = rng.normal(size=(count, 3))
    n *= rng.uniform(0.25, 4.0, (count, 1)) / np.linalg.norm(n, axis=1, keepdims=True)        # normals need not be unit length
    s = (n * centre).sum(axis=1)
    w = size * np.linalg.norm(n, axis=1)
    gap = rng.random(count) < 0.5
    for i in np.nonzero(kind == 2)[0]:
        planes[i] = [np.append(n[i], w[i] - s[i]), np.append(-n[i], w[i] + s[i]), pad, pad, pad, pad]
    for i in np.nonzero(kind == 3)[0]:
        planes[i] = np.append(n[i], -s[i])
    for i in np.nonzero((kind == 6) & gap)[0]:
        g = ext * np.linalg.norm(n[i])
        planes[i] = [np.append(n[i], -s[i] - g), np.append(-n[i], s[i] - g), pad, pad, pad, pad]
    # 6 (odd): a small box far outside the mesh
    idx = np.nonzero((kind == 6) & ~gap)[0]
    away = centre[idx] + 3.0 * ext * np.sign(rng.normal(size=(len(idx), 3)))
    planes[idx] = H().obb_planes(away, rot[idx], half[idx] / size[idx, None] * tri[idx, None])["plane"]
    # 4: -0 normals
    idx = np.nonzero(kind == 4)[0]
    p = H().aabb_planes(centre[idx] - half[idx], centre[idx] + half[idx])["plane"].copy()
    p[..., :3] = np.where(p[..., :3] == 0.0, F(-0.0), p[..., :3])
    planes[idx] = p
    # 5: a face exactly on a triangle box's face: the region starts where the box of triangle k ends in x
    idx = np.nonzero(kind == 5)[0]
    qlo = (centre[idx] - half[idx]).astype(F)
    qhi = (centre[idx] + half[idx]).astype(F)
    qlo[:, 0] = hi[k[idx], 0]
    qlo[1::2, 0] = np.nextafter(qlo[1::2, 0], F(np.inf))
    qhi[:, 0] = np.maximum(qhi[:, 0], qlo[:, 0] + F(1.0))
    planes[idx] = H().aabb_planes(qlo, qhi)["plane"]
    # 7: NaN and +-inf
    idx = np.nonzero(kind == 7)[0]
    bad = np.array([np.nan, np.inf, -np.inf], dtype=F)[rng.integers(0, 3, len(idx))]
    planes[idx, rng.integers(0, 6, len(idx)), rng.integers(0, 4, len(idx))] = bad
    return R.make_regions(planes), kind, k


_CASES = {}


def case(name, lo=None, hi=None):
    """(a, b, c, lo, hi, regions, kinds, reference), once per mesh.  The CPU tests pass no boxes and get the padded ones; the GPU
    tests pass the library's and get the same set and reference when the boxes are the same words (they are, on these meshes)."""
    a, b, c = positions(scene(name))
    plo, phi = padded_boxes(a, b, c)
    if name not in _CASES:
        regions, kind, k = mixed_regions(a, b, c, plo, phi)
        _CASES[name] = (a, b, c, plo, phi, regions, kind, R.reference(regions, plo, phi))
    if lo is None or ((words(lo) == words(plo)).all() and (words(hi) == words(phi)).all()):
        return _CASES[name]
    regions, kind = _CASES[name][5:7]               # (other boxes: the same regions, the reference on the boxes given)
    return (a, b, c, lo, hi, regions, kind, R.reference(regions, lo, hi))


def sizes(ref, mode):
    return np.diff(ref[mode][0]).astype(np.int64)


def check_not_vacuous(name, ref, kind):
    """conditions on the brute force alone: at least a third of the regions non-empty in TOUCHING, a tenth non-empty in CONTAINED, a
    tenth empty, some region with CONTAINED strictly smaller than TOUCHING — and every kind present"""
    t, c = sizes(ref, R.TOUCHING), sizes(ref, R.CONTAINED)
    print(f"{name}: TOUCHING {100.0 * (t > 0).mean():.1f} % non-empty (total {int(t.sum())}, longest {int(t.max())}), "
          f"CONTAINED {100.0 * (c > 0).mean():.1f} % (total {int(c.sum())}), empty {100.0 * (t == 0).mean():.1f} %, "
          f"CONTAINED < TOUCHING in {int((c < t).sum())}")
    assert len(t) == COUNT and (np.bincount(kind, minlength=8) >= 30).all()
    assert (t > 0).mean() >= 1.0 / 3.0 and (c > 0).mean() >= 0.1 and (t == 0).mean() >= 0.1
    assert (c <= t).all() and (c < t).any() and ((c > 0) & (c < t)).any()


# ---- CPU: the surface in every host ----------------------------------------------------------------------------------------------

def test_header_declares_the_struct_the_modes_and_both_calls():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"#define LBVH_REGION_PLANES\s+6\b", h) and re.search(r"#define LBVH_REGION_TOUCHING\s+0u", h)
    assert re.search(r"#define LBVH_REGION_CONTAINED\s+1u", h)
    assert re.search(r"typedef struct lbvh_region \{ float plane\[LBVH_REGION_PLANES\]\[4\]; \} lbvh_region;", h)
    assert re.search(r"lbvh_status lbvh_region_overlaps\(lbvh_context\*( ctx)?, const lbvh_region\* d_regions, size_t count, uint32_t mode,\s+"
                     r"const lbvh_scene\* h_scene,\s+uint64_t\* d_offsets, uint32_t\* d_tris, uint64_t capacity\);", h)
    assert re.search(r"lbvh_status lbvh_region_overlaps_any\(lbvh_context\*( ctx)?, const lbvh_region\* d_regions, size_t count, uint32_t mode,\s+"
                     r"const lbvh_scene\* h_scene,\s+uint32_t\* d_flags\);", h)
    assert re.search(r"#define LBVH_ABI_VERSION\s+11\b", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_region_overlaps" in bounce and "lbvh_region_overlaps_any" in bounce
    text = h[h.index("Region queries: WHICH"):h.index("lbvh_status lbvh_region_overlaps(")]
    for must in ("P = ((nx * (nx >= 0 ? hi.x : lo.x) + ny * (ny >= 0 ? hi.y : lo.y)) + nz * (nz >= 0 ? hi.z : lo.z)) + d",
                 "N = ((nx * (nx >= 0 ? lo.x : hi.x) + ny * (ny >= 0 ? lo.y : hi.y)) + nz * (nz >= 0 ? lo.z : hi.z)) + d",
                 "true for -0 and false for NaN", "no \"inactive query\" rule", "conservative frustum test", "wholly inside",
                 "monotone", "exact min / max union", "NOT PART OF THE CONTRACT", "d_offsets[0] included", "mode > 1",
                 "One region per lane"):
        assert must in text, must


def test_native_prototypes_and_the_other_hosts():
    nat = N()
    res, args = nat.SIGNATURES["lbvh_region_overlaps"]
    assert res is C.c_int32 and len(args) == 8 and args[2] is C.c_size_t and args[3] is C.c_uint32 and args[7] is C.c_uint64
    res, args = nat.SIGNATURES["lbvh_region_overlaps_any"]
    assert res is C.c_int32 and len(args) == 6 and args[2] is C.c_size_t and args[3] is C.c_uint32
    assert nat.ABI_VERSION == 11 and nat.lib.lbvh_abi_version() == 11
    assert callable(nat.lib.lbvh_region_overlaps) and callable(nat.lib.lbvh_region_overlaps_any)
    lay = L()
    assert lay.REGION.itemsize == 96 and lay.REGION["plane"].shape == (6, 4) and (lay.REGION_TOUCHING, lay.REGION_CONTAINED) == (0, 1)
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_region_overlaps\(IntPtr ctx, IntPtr \w+, UIntPtr count, uint mode, ref Scene scene,\s+IntPtr \w+,"
                     r"\s+IntPtr \w+,\s+ulong capacity\);", cs)
    assert re.search(r"public static extern int lbvh_region_overlaps_any\(IntPtr ctx, IntPtr \w+, UIntPtr count, uint mode, ref Scene scene,\s+IntPtr \w+\);", cs)
    rq = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "RegionQueries.cs")).read())
    assert "lbvh_region_overlaps(" in rq and "lbvh_region_overlaps_any(" in rq and "unsafe" not in rq
    hpp = open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    for must in ("void RegionOverlaps(", "void RegionOverlapsAny(", "FrustumPlanes(", "ObbPlanes(", "AabbPlanes("):
        assert must in hpp, must
    drawer = H().RaytracingMeshDrawer
    assert all(hasattr(drawer, m) for m in ("region_overlaps", "region_overlaps_any", "in_regions"))
    assert all(hasattr(H(), m) for m in ("frustum_planes", "obb_planes", "aabb_planes"))


# ---- CPU: the reference --------------------------------------------------------------------------------------------------------------

def dyadic_inputs(rng, n_regions, n_boxes):
    """planes and boxes on multiples of 1/8 below 16 in magnitude: every fp32 product and sum of the definition is exact"""
    planes = rng.integers(-16, 17, (n_regions, 6, 4)) / 8.0
    planes[..., 3] = rng.integers(-256, 257, (n_regions, 6)) / 8.0
    planes[rng.random((n_regions, 6)) < 0.3] = R.PAD
    lo = rng.integers(-64, 64, (n_boxes, 3)) / 8.0
    hi = lo + rng.integers(0, 24, (n_boxes, 3)) / 8.0
    return planes.astype(F), lo.astype(F), hi.astype(F)


def test_reference_equals_a_float64_max_and_min_over_the_eight_corners_on_dyadic_inputs():
    rng = np.random.default_rng(3)
    planes, lo, hi = dyadic_inputs(rng, 300, 400)
    ref = R.reference(R.make_regions(planes), lo, hi)
    corners = np.stack([np.where(np.array([(m >> k) & 1 for k in range(3)], dtype=bool), hi, lo) for m in range(8)], axis=1).astype(np.float64)
    value = np.einsum("rjk,bck->rjbc", planes[..., :3].astype(np.float64), corners) + planes[..., 3].astype(np.float64)[:, :, None, None]
    touching = (value.max(axis=3) >= 0.0).all(axis=1)             # [regions, boxes]: the farthest corner of every plane is kept
    contained = (value.min(axis=3) >= 0.0).all(axis=1)
    for mode, m in ((R.TOUCHING, touching), (R.CONTAINED, contained)):
        off, tris = ref[mode]
        assert (np.diff(off).astype(np.int64) == m.sum(axis=1)).all() and (tris == np.nonzero(m)[1]).all()
        assert 0.02 < m.mean() < 0.98
    assert (contained & ~touching).sum() == 0 and (touching & ~contained).sum() > 0


def random_floats(rng, shape):
    """fp32 values of every magnitude from denormals to 1e18, both signs, with exact zeros and -0 among them"""
    v = (rng.uniform(-1.0, 1.0, shape) * 10.0 ** rng.choice([-42.0, -20.0, -3.0, 0.0, 0.0, 2.0, 18.0], shape)).astype(F)
    v[rng.random(shape) < 0.05] = F(0.0)
    v[rng.random(shape) < 0.02] = F(-0.0)
    return v


def test_contained_is_within_touching_and_an_ancestor_box_passes_touching_on_random_fp32_inputs():
    """the two inequalities the order-independence argument of the header rests on, N(A) <= P(A) <= P(B) for a box A inside a box B,
    on 10^5 random (box, sub-box, plane) triples, and what follows for the candidates"""
    rng = np.random.default_rng(4)
    n = 100000
    p0, p1, q0, q1 = (random_floats(rng, (n, 3)) for _ in range(4))
    a_lo, a_hi = np.minimum(p0, p1), np.maximum(p0, p1)
    b_lo, b_hi = np.minimum(a_lo, np.minimum(q0, q1)), np.maximum(a_hi, np.maximum(q0, q1))       # the exact min / max union of two boxes
    planes = random_floats(rng, (n, 4))
    PA, NA = R.corner_values(planes, a_lo, a_hi)
    PB, _ = R.corner_values(planes, b_lo, b_hi)
    assert np.isfinite(PA).all() and np.isfinite(PB).all()
    assert (NA <= PA).all() and (PA <= PB).all()
    assert (PA < PB).sum() > n // 10 and (NA < PA).sum() > n // 2
    assert not ((NA >= 0) & ~(PA >= 0)).any() and not ((PA >= 0) & ~(PB >= 0)).any()
    assert 0.1 < (PA >= 0).mean() < 0.9 and 0.1 < (NA >= 0).mean() < 0.9
    assert ((np.abs(PA) < F(1.2e-38)) & (PA != 0)).sum() > 0        # denormal sums occur: the claim includes gradual underflow


@pytest.mark.parametrize("name", MESHES)
def test_the_parity_sets_are_not_vacuous(name):
    a, b, c, lo, hi, regions, kind, ref = case(name)
    check_not_vacuous(name, ref, kind)
    planes = regions["plane"]
    assert np.isnan(planes).any() and np.isinf(planes).any() and (np.signbit(planes[..., :3]) & (planes[..., :3] == 0)).any()
    exact = np.nonzero(kind == 5)[0]
    t = sizes(ref, R.TOUCHING)
    assert (t[exact[::2]] > 0).sum() > len(exact) // 4               # the touched triangle is a candidate of the even ones


def test_driver_generator_is_deterministic_and_has_both_kinds_of_region():
    tris, pos, lo, hi = driver_mesh(4096)
    r = R.driver_regions(lo, hi, 200, seed=6)
    assert (words(r["plane"]) == words(R.driver_regions(lo, hi, 200, seed=6)["plane"])).all()
    assert (r["plane"] != R.driver_regions(lo, hi, 200, seed=7)["plane"]).any()
    p = r["plane"]
    assert (p[:, 0::2, :3] == -p[:, 1::2, :3]).all() and (p[:, 0, 0] == 1).all() and (np.abs(p[:, 0, 1:3]) <= 0.5).all()
    ref = R.reference(r, *padded_boxes(pos[:, 0], pos[:, 1], pos[:, 2]))
    t, c = np.diff(ref[R.TOUCHING][0]).astype(np.int64), np.diff(ref[R.CONTAINED][0]).astype(np.int64)
    assert (t > 0).sum() > 50 and (t == 0).sum() > 5 and (c > 0).sum() > 20 and (c < t).any()


# ---- CPU: the plane builders -----------------------------------------------------------------------------------------------------------

def test_aabb_planes_give_the_box_lists_of_the_overlap_reference_on_dyadic_coordinates():
    rng = np.random.default_rng(5)
    _, lo, hi = dyadic_inputs(rng, 1, 500)
    qlo = (rng.integers(-72, 64, (200, 3)) / 8.0).astype(F)
    qhi = qlo + (rng.integers(0, 40, (200, 3)) / 8.0).astype(F)
    regions = H().aabb_planes(qlo, qhi)
    assert regions.dtype == L().REGION and regions.shape == (200,)
    off, tris = R.reference(regions, lo, hi)[R.TOUCHING]
    boff, btris = V.box_overlaps(V.make_boxes(qlo, qhi), lo, hi)
    assert (off == boff).all() and (tris == btris).all() and 0 < len(tris) < 200 * 500
    assert (qlo[:, None, :] == hi[None]).any()                       # faces that touch exactly occur


def test_obb_planes_with_identity_axes_equal_aabb_planes():
    rng = np.random.default_rng(6)
    lo = rng.integers(-64, 64, (50, 3)) / 8.0
    hi = lo + rng.integers(1, 40, (50, 3)) / 8.0
    a = H().aabb_planes(lo, hi)["plane"]
    o = H().obb_planes((lo + hi) / 2.0, np.eye(3), (hi - lo) / 2.0)["plane"]
    assert a.dtype == F and (a == o).all()
    # a turned box: its eight corners are on or inside every plane, points beyond a face are outside
    rot = _rotations(rng, 1)[0]
    centre, half = np.array([1.0, -2.0, 3.0]), np.array([0.5, 2.0, 1.0])
    p = H().obb_planes(centre, rot, half)["plane"][0].astype(np.float64)
    sign = np.array([[(m >> k) & 1 for k in range(3)] for m in range(8)]) * 2.0 - 1.0
    corners = centre + (sign * half) @ rot
    assert (corners @ p[:, :3].T + p[:, 3] > -1e-5).all()
    beyond = centre + (sign * half * 1.01) @ rot
    assert ((beyond @ p[:, :3].T + p[:, 3] < 0).sum(axis=1) == 3).all()


def test_frustum_planes_hold_the_primary_rays_between_near_and_far():
    """ray generation from the Python oracle (oracle/literal_emulation.py make_ray, the convention of lbvh_trace_primary): every
    pixel-centre ray's points at depths strictly between near_plane and far are inside all six planes in float64; a point mirrored
    just beyond face j is outside plane j"""
    from oracle import literal_emulation as E
    rng = np.random.default_rng(7)
    m = np.eye(4)
    m[:3, :3] = _rotations(rng, 1)[0]
    m[:3, 3] = (3.0, -7.0, 11.0)
    far = 40.0
    for cam in (scenes.camera(16, 12, (0.0, 0.0, 300.0)),
                {"screen_width": 12, "screen_height": 16, "camera_fov": 0.35, "near_plane": 0.5, "camera_to_world": m.astype(F).reshape(-1)}):
        planes = H().frustum_planes(cam, far)["plane"][0].astype(np.float64)
        mat = np.asarray(cam["camera_to_world"], dtype=np.float64).reshape(4, 4)
        axis = -mat[:3, 2]                                            # the view direction in world space
        near = float(F(cam["near_plane"]))
        pts = []
        for idy in range(cam["screen_height"]):
            for idx in range(cam["screen_width"]):
                origin, direction, _ = E.make_ray(cam, idx, idy)
                o, d = np.array(origin, dtype=np.float64), np.array(direction, dtype=np.float64)
                for depth in (near * 1.001, 0.5 * (near + far), far * 0.999):
                    pts.append(o + d * (depth / (d @ axis)))
        pts = np.array(pts)
        value = pts @ planes[:, :3].T + planes[:, 3]
        assert (value > 0).all(), value.min()
        for j in range(6):
            nj = planes[j, :3]
            mirrored = pts - (1.001 * value[:, j] / (nj @ nj))[:, None] * nj
            assert (mirrored @ nj + planes[j, 3] < 0).all(), j
        # the corner pixels' rays graze the side planes within a pixel: a ray one pixel outside the image is outside
        origin, direction, _ = E.make_ray(cam, -1, 0)
        out = np.array(origin, dtype=np.float64) + np.array(direction, dtype=np.float64) * 5.0
        assert (out @ planes[:, :3].T + planes[:, 3] < 0).any()
    # rect: the tile's frustum is inside the whole image's
    cam = scenes.camera(64, 64, (0.0, 0.0, 300.0))
    tile = H().frustum_planes(cam, far, rect=(8, 16, 16, 24))["plane"][0].astype(np.float64)
    origin, direction, _ = E.make_ray(cam, 12, 20)
    p = np.array(origin, dtype=np.float64) + np.array(direction, dtype=np.float64) * 10.0
    assert (p @ tile[:, :3].T + tile[:, 3] > 0).all()
    origin, direction, _ = E.make_ray(cam, 20, 20)
    p = np.array(origin, dtype=np.float64) + np.array(direction, dtype=np.float64) * 10.0
    assert (p @ tile[:, :3].T + tile[:, 3] < 0).any()


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------

class Regions:
    """device buffers of one region set; run() = one lbvh_region_overlaps call on caller-owned buffers"""

    def __init__(self, ctx, drawer, regions):
        self.ctx, self.drawer, self.count = ctx, drawer, len(regions)
        self.regions = H().DataBuffer(ctx, max(len(regions), 1), L().REGION)
        self.regions.local[:len(regions)] = regions
        self.regions.sync()
        self.offsets = H().DataBuffer(ctx, len(regions) + 1, np.uint64)
        self.flags = H().DataBuffer(ctx, max(len(regions), 1), np.uint32)

    def run(self, mode, tris=None, capacity=None, poison=0xDEADBEEF):
        """offsets (host copy) after one call; tris: a uint32 DataBuffer or None, capacity defaults to its size"""
        self.offsets.fill_u32(poison)
        s = self.drawer.container.scene()
        cap = 0 if tris is None else (tris.size if capacity is None else capacity)
        N().check(self.ctx.handle, N().lib.lbvh_region_overlaps(self.ctx.handle, self.regions.device, self.count, mode, C.byref(s),
                                                                self.offsets.device, tris.device if tris is not None else None, cap))
        return self.offsets.get_data().copy()

    def lists(self, mode, device_sort=True):
        """(offsets, tris) through count -> allocate -> fill, every segment ascending"""
        off, tris = self.drawer.in_regions(self.regions, mode, device_sort=device_sort)
        return (off, tris) if device_sort else (off, V.sort_segments(off, tris))

    def any(self, mode):
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.region_overlaps_any(self.regions, mode, self.flags)
        return self.flags.get_data()[:self.count].copy()

    def dispose(self):
        for b in (self.regions, self.offsets, self.flags):
            b.dispose()


def assert_equal_lists(got, ref, what=""):
    (go, gt), (ro, rt) = got, ref
    assert len(go) == len(ro) and (go == ro).all(), (what, np.nonzero(go[:len(ro)] != ro)[0][:10])
    assert len(gt) == len(rt) == int(ro[-1]), (what, len(gt), len(rt))
    bad = np.nonzero(gt != rt)[0]
    assert len(bad) == 0, (what, bad[:10], gt[bad[:10]], rt[bad[:10]])


_GPU = {}


def gpu_case(ctx, name):
    """(a, b, c, lo, hi, regions, kinds, reference with the library's boxes, drawer); a context keeps one derived traversal scene, so
    it is derived again for the test that asks"""
    if name not in _GPU:
        d = H().RaytracingMeshDrawer(ctx, scene(name)).awake()
        lo, hi = library_boxes(d)
        _GPU[name] = case(name, lo, hi) + (d,)
    _GPU[name][-1].build_fast_scene()
    return _GPU[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MESHES)
def test_r1_parity_with_the_brute_force(ctx, name):
    a, b, c, lo, hi, regions, kind, ref, d = gpu_case(ctx, name)
    check_not_vacuous(name, ref, kind)
    q = Regions(ctx, d, regions)
    for mode in MODES:
        ro, rt = ref[mode]
        assert (ro == np.concatenate([[0], np.cumsum(np.diff(ro))]).astype(np.uint64)).all()
        assert_equal_lists(q.lists(mode, device_sort=(mode == R.TOUCHING)), ref[mode], (name, mode))
        assert (q.run(mode) == ro).all()                             # the offsets are the brute force's prefix sums
        assert (q.any(mode) == (np.diff(ro) > 0)).all(), (name, mode)
    assert N().lib.lbvh_sync(ctx.handle) == 0
    q.dispose()


@pytest.mark.gpu
def test_r2_the_csr_contract(ctx):
    a, b, c, lo, hi, regions, kind, ref, d = gpu_case(ctx, "cfg1_4096")
    h, lib, s = ctx.handle, N().lib, d.container.scene()
    q = Regions(ctx, d, regions)
    for mode in MODES:
        ro, rt = ref[mode]
        total = int(ro[-1])
        assert (q.run(mode, None) == ro).all()                       # capacity == 0, d_tris == NULL
        # a capacity that cuts a segment in half
        n = np.diff(ro).astype(np.int64)
        cut = int(np.nonzero((n >= 2) & (ro[:-1] > total // 3))[0][0])
        cap, guard = int(ro[cut]) + int(n[cut]) // 2, 4096
        assert int(ro[cut]) < cap < int(ro[cut + 1])
        buf = H().DataBuffer(ctx, total + guard, np.uint32)
        buf.fill_u32(0xABABABAB)
        off = q.run(mode, buf, capacity=cap)
        got = buf.get_data().copy()
        assert (off == ro).all() and int(off[-1]) == total           # d_offsets[count] still says what was needed
        assert (got[cap:] == 0xABABABAB).all()                       # nothing at the capacity or beyond
        last = int(ro[cut])
        assert (V.sort_segments(ro[:cut + 1], got[:last]) == rt[:last]).all()       # the complete segments are complete
        # the retry with what the offsets asked for, then the device sort: strictly ascending segments equal to the reference
        buf.fill_u32(0xABABABAB)
        off = q.run(mode, buf, capacity=total)
        H().sort_index_segments(ctx, q.offsets, buf, q.count)
        got = buf.get_data().copy()
        assert (got[total:] == 0xABABABAB).all() and (got[:total] == rt).all()
        seg = np.repeat(np.arange(q.count), n)
        assert ((np.diff(got[:total].astype(np.int64)) > 0) | (np.diff(seg) != 0)).all()
        # count == 0 touches nothing, d_offsets[0] included; every flag of the any form is written over poison
        q.offsets.fill_u32(POISON)
        buf.fill_u32(POISON)
        q.flags.fill_u32(POISON)
        assert lib.lbvh_region_overlaps(h, q.regions.device, 0, mode, C.byref(s), q.offsets.device, buf.device, total) == 0
        assert lib.lbvh_region_overlaps_any(h, q.regions.device, 0, mode, C.byref(s), q.flags.device) == 0
        assert all((words(x.get_data()) == POISON).all() for x in (q.offsets, buf, q.flags))
        flags = q.any(mode)
        assert np.isin(flags, (0, 1)).all() and (flags == (n > 0)).all()
        buf.dispose()
    assert lib.lbvh_sync(h) == 0
    q.dispose()


@pytest.mark.gpu
def test_r3_axis_aligned_regions_equal_box_overlaps_and_contained_is_within_touching(ctx):
    """a mesh snapped to a grid of 1 / 8 and boxes on that grid: aabb_planes(box) in TOUCHING mode asks hi - q.lo >= 0 where
    lbvh_box_overlaps asks q.lo <= hi.  With gradual underflow the two agree for every pair of floats; were denormal results
    flushed to zero, a box missing a face by less than 1.2e-38 would pass — that would be a finding about how the file is compiled."""
    tris = scenes.random_triangles(n=3000, seed=31, extent=12.0, edge=3.0)
    for key in "abc":
        tris[key][:, :3] = np.round(tris[key][:, :3] * 8.0) / 8.0
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    rng = np.random.default_rng(32)
    count = 1200
    qlo = (rng.integers(-13 * 8, 12 * 8, (count, 3)) / 8.0).astype(F)
    qhi = qlo + (rng.integers(0, 6 * 8, (count, 3)) / 8.0).astype(F)
    third = count // 3                                               # a third of the boxes start exactly where a triangle's box ends
    qlo[:third, 0] = hi[rng.integers(0, len(hi), third), 0]
    qhi[:third, 0] = qlo[:third, 0] + F(1.0)
    boxes = H().DataBuffer(ctx, count, L().AABB)
    boxes.local[:] = V.make_boxes(qlo, qhi)
    boxes.sync()
    boff, btris = d.overlaps(boxes, device_sort=True)
    q = Regions(ctx, d, H().aabb_planes(qlo, qhi))
    off, t = q.lists(R.TOUCHING)
    assert_equal_lists((off, t), (boff, btris), "aabb_planes against lbvh_box_overlaps")
    assert_equal_lists((off, t), V.box_overlaps(boxes.local, lo, hi), "... and the brute force")
    assert len(t) > count
    coff, ct = q.lists(R.CONTAINED)
    seg = np.repeat(np.arange(count, dtype=np.int64), np.diff(off).astype(np.int64))
    cseg = np.repeat(np.arange(count, dtype=np.int64), np.diff(coff).astype(np.int64))
    n = len(tris)
    assert np.isin(cseg * n + ct, seg * n + t).all() and 0 < len(ct) < len(t)
    assert_equal_lists((coff, ct), R.reference(q.regions.local, lo, hi)[R.CONTAINED])
    # ... and on the mixed set of a golden mesh
    boxes.dispose()
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 2, 3, 7])
def test_r4_wave_caps_refill_the_lanes(ctx, cap):
    """1 500 regions on 1, 2, 3 and 7 waves: runs of 1 500 .. 215, every lane refilled several times"""
    a, b, c, lo, hi, regions, kind, ref, d = gpu_case(ctx, "grid_80x80")
    q = Regions(ctx, d, regions)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, cap))
    try:
        got = [(q.lists(mode), q.any(mode)) for mode in MODES]
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    for mode, (lists, flags) in zip(MODES, got):
        assert_equal_lists(lists, ref[mode], (cap, mode))
        assert (flags == (np.diff(ref[mode][0]) > 0)).all()
    assert lib.lbvh_sync(h) == 0
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 1023, 1024, 1025])
def test_r4_counts_across_a_scan_tile_border(ctx, count):
    a, b, c, lo, hi, regions, kind, ref, d = gpu_case(ctx, "cfg1_4096")
    sub = regions[100:100 + count]
    q = Regions(ctx, d, sub)
    for mode in MODES:
        ro, rt = ref[mode]
        first, last = int(ro[100]), int(ro[100 + count])
        want = (ro[100:100 + count + 1] - ro[100], rt[first:last])
        assert count == 1 or last > first
        assert_equal_lists(q.lists(mode), want, (count, mode))
        assert (q.any(mode) == (np.diff(want[0]) > 0)).all()
    q.dispose()


@pytest.mark.gpu
def test_r4_the_stack_limit_is_reported_not_a_short_list():
    """lbvh_debug_ray_stack_limit: with one stack entry in LDS and one in device memory a region around the whole mesh cannot keep
    its waiting siblings; the call reports LBVH_FAULT_RAY_STACK through the next lbvh_sync instead of returning a short list"""
    tris = scene("cfg1_4096")
    c2 = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        lo, hi = library_boxes(d)
        whole = H().aabb_planes(lo.min(axis=0) - F(1.0), hi.max(axis=0) + F(1.0))
        ref = R.reference(whole, lo, hi)
        assert int(ref[R.TOUCHING][0][-1]) == len(tris) == int(ref[R.CONTAINED][0][-1])
        q = Regions(c2, d, whole)
        h, lib = c2.handle, N().lib
        assert_equal_lists(q.lists(R.TOUCHING), ref[R.TOUCHING])
        assert lib.lbvh_sync(h) == 0
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
        s = d.container.scene()                                       # (no download here: it would report the fault before lbvh_sync does)
        N().check(h, lib.lbvh_region_overlaps(h, q.regions.device, 1, R.TOUCHING, C.byref(s), q.offsets.device, None, 0))
        assert lib.lbvh_sync(h) == -3
        assert b"stack" in lib.lbvh_last_error(h)
        N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
        assert_equal_lists(q.lists(R.CONTAINED), ref[R.CONTAINED], "after the stack limit")
        assert lib.lbvh_sync(h) == 0
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_r5_count_zero_rejections_and_a_stale_scene():
    """the rows tests/test_query_entry_contract.py has for the other entry points, for these two, on a context of its own: every
    rejection is LBVH_ERR_INVALID_ARG with the entry point's name in the error text, and writes nothing"""
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        k = rng.integers(0, 64, 130)
        regions = H().obb_planes(a[k] + rng.normal(size=(130, 3)), _rotations(rng, 130), rng.uniform(0.5, 6.0, (130, 3)))
        ref = R.reference(regions, lo, hi)
        flags_t = np.diff(ref[R.TOUCHING][0]) > 0
        assert 0 < np.diff(ref[R.CONTAINED][0]).astype(bool).sum() < flags_t.sum() <= 130
        q = Regions(ctx, d, regions)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, np.uint32)
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        both, flag = lib.lbvh_region_overlaps, lib.lbvh_region_overlaps_any
        dq, do, df, dl = q.regions.device, q.offsets.device, q.flags.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, q.flags, lst)

        def poison():
            for buf in bufs:
                buf.fill_u32(POISON)

        def untouched():
            return all((words(buf.get_data()) == POISON).all() for buf in bufs)

        poison()
        assert both(h, dq, 0, 0, C.byref(s), do, dl, 64) == 0 and flag(h, dq, 0, 1, C.byref(s), df) == 0     # count == 0: a no-op
        for args in ((None, 10, 0, C.byref(s), do, None, 0), (dq, 10, 0, None, do, None, 0), (dq, 10, 0, C.byref(s), None, None, 0),
                     (dq, 10, 2, C.byref(s), do, None, 0), (dq, 10, 0xFFFFFFFF, C.byref(s), do, None, 0),
                     (dq, 10, 1, C.byref(s), do, None, 5), (at(q.regions, 8), 10, 0, C.byref(s), do, None, 0),
                     (dq, 10, 0, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, 1, C.byref(s), do, at(lst, 2), 8),
                     (dq, 1 << 32, 0, C.byref(s), do, None, 0)):
            assert both(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_region_overlaps: "), lib.lbvh_last_error(h)
        for args in ((None, 10, 0, C.byref(s), df), (dq, 10, 0, None, df), (dq, 10, 1, C.byref(s), None), (dq, 10, 2, C.byref(s), df),
                     (at(q.regions, 8), 10, 0, C.byref(s), df), (dq, 10, 0, C.byref(s), at(q.flags, 2)), (dq, 1 << 32, 1, C.byref(s), df)):
            assert flag(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_region_overlaps_any: "), lib.lbvh_last_error(h)
        assert both(None, dq, 10, 0, C.byref(s), do, None, 0) == -1 and flag(None, dq, 10, 0, C.byref(s), df) == -1
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names the entry point
        d.container.triangle_data.sync()
        for fn, args, name in ((both, (do, None, 0), b"lbvh_region_overlaps"), (flag, (df,), b"lbvh_region_overlaps_any")):
            assert fn(h, dq, 130, 0, C.byref(s), *args) == -1
            msg = lib.lbvh_last_error(h)
            assert msg.startswith(name + b": ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        # aligned sub-ranges are fine; the plain and the counting instantiation write the same words, and the latter counts
        assert both(h, at(q.regions, 96), 10, 0, C.byref(s), at(q.offsets, 8), at(lst, 4), 8) == 0
        stats.fill_u32(POISON)
        plain = [(q.lists(mode), q.any(mode)) for mode in MODES]
        assert (words(stats.get_data()) == POISON).all()
        for mode, (lists, flags) in zip(MODES, plain):
            assert_equal_lists(lists, ref[mode], mode)
            assert (flags == (np.diff(ref[mode][0]) > 0)).all()
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            counted = [(q.lists(mode), q.any(mode)) for mode in MODES]
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        st = stats.get_data()[0]
        for (pl, pf), (cl, cf) in zip(plain, counted):
            assert (pl[0] == cl[0]).all() and (pl[1] == cl[1]).all() and (pf == cf).all()
        assert st["rays"] == 130 * 8 and st["node_fetches"] > 0 and st["triangle_tests"] > 0, st      # per mode: count, count + fill, any — every region walks
        for buf in (lst, stats):
            buf.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_r5_the_live_path_list_is_dropped(ctx):
    """a path-traced frame with both calls issued between the bounces equals the undisturbed frame"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    count = 160 * 96
    st0 = pt.states.get_data()[:count].copy()
    lo, hi = library_boxes(pt.drawer)
    rng = np.random.default_rng(12)
    n = 4 * count                                                    # 4x the frame: the scratch grows in mid-frame
    k = rng.integers(0, len(lo), n)
    q = Regions(ctx, pt.drawer, H().obb_planes((lo[k] + hi[k]) * F(0.5), _rotations(rng, n), rng.uniform(0.5, 3.0, (n, 3))))
    cam = N().Camera.from_dict(cam_d)
    h, s, lib = ctx.handle, pt.drawer.container.scene(), N().lib

    def both():
        N().check(h, lib.lbvh_region_overlaps(h, q.regions.device, n, R.TOUCHING, C.byref(s), q.offsets.device, None, 0))
        N().check(h, lib.lbvh_region_overlaps_any(h, q.regions.device, n, R.CONTAINED, C.byref(s), q.flags.device))

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    both()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        both()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    both()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    assert (words(pt.states.get_data()[:count]) == words(st0)).all()
    assert (pt.image().view(np.uint16) == img0.view(np.uint16)).all()
    assert int(q.offsets.get_data()[n]) > n and 0 < int(q.flags.get_data()[:n].sum()) < n
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
def test_r6_the_device_sorted_lists_equal_the_host_sorted_ones(ctx):
    a, b, c, lo, hi, regions, kind, ref, d = gpu_case(ctx, "example_object3")
    q = Regions(ctx, d, regions)
    for mode in MODES:
        off, tris = d.in_regions(q.regions, mode)
        soff, stris = d.in_regions(q.regions, mode, device_sort=True)
        assert (off == soff).all() and (V.sort_segments(off, tris) == stris).all() and len(stris) == int(ref[mode][0][-1])
    off, tris = d.in_regions(q.regions)                              # the default mode is TOUCHING
    assert_equal_lists((off, V.sort_segments(off, tris)), ref[R.TOUCHING])
    q.dispose()


@pytest.mark.gpu
def test_r7_the_cpp_driver_end_to_end(ctx):
    """`lbvh_driver regions 2000 6`: RegionOverlaps in both modes, SortIndexSegments and RegionOverlapsAny of lbvh_host.hpp on the
    driver's own mesh and regions, against the brute force on the Python mirrors of its generators and the library's boxes"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "regions", str(count), "6"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)                              # the mesh lbvh_driver.cpp generates (SplitMix64, seed 1)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    ref = R.reference(R.driver_regions(lo, hi, count, seed=6), *library_boxes(d))
    d.on_destroy()
    assert (res["triangles"], res["regions"]) == (4096, count)
    for mode, key in ((R.TOUCHING, "touching"), (R.CONTAINED, "contained")):
        ro, rt = ref[mode]
        n = np.diff(ro).astype(np.int64)
        weighted = int(((np.arange(len(rt), dtype=np.uint64) + np.uint64(1)) * rt.astype(np.uint64)).sum())
        assert int(ro[-1]) > 0
        assert (res[key]["total"], res[key]["non_empty"], res[key]["flagged"], res[key]["weighted_index_sum"]) == \
            (int(ro[-1]), int((n > 0).sum()), int((n > 0).sum()), weighted), key
    ro, rt = ref[R.TOUCHING]
    first = np.nonzero(np.diff(ro))[0][:3]
    assert res["segments"] == [[int(k)] + rt[int(ro[k]):int(ro[k + 1])].tolist() for k in first]
