#!/usr/bin/env python3
"""lbvh_region_overlaps / lbvh_region_overlaps_any on the cfg2 mesh (1 M triangles), next to the workaround they replace:
lbvh_box_overlaps on the regions' axis-aligned bounding boxes.  Prints one JSON line.

Region sets, 2^20 regions each, every one about the size of a few triangles (--size times the median triangle-box diagonal):
  cubes     cubes centred on seeded scene triangles, turned about a seeded axis by a seeded angle (host.obb_planes)
  frusta    thin cluster frusta: an eye 8 sizes away from a seeded triangle, looking at it, the frustum of one 8 x 8 pixel tile of a
            64 x 64 image between 0.75 and 1.25 of that distance (host.frustum_planes with rect)
Per set, in LBVH_REGION_TOUCHING mode (CONTAINED: the count-only form beside it):
  count_only / full / any          the three forms of the call
  box_overlaps                     lbvh_box_overlaps (count only and full) on the bounding boxes of the regions' eight corners
  time_ratio                       workaround / region call, per form
  candidate_ratio                  workaround segments' total / TOUCHING segments' total
The priced caveat: one camera frustum covering about half the mesh, alone (count 1) and as region 0 among the 2^20 small cubes.

Before anything is printed `--check` regions of every set are compared with tests/region_reference.py (every segment sorted, word for
word, both modes; the flags), and the offsets of the count-only call with those of count + fill.  Times: device events around
`--launches` back-to-back calls, `--reps` times after `--warmup`; per call = median (min / max beside it)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def corners_box(planes):
    """the axis-aligned bounding box of a bounded region's eight corners: the intersections of one plane of each opposed pair
    (planes 2k, 2k + 1), in float64 -> (lo, hi) rounded outward to fp32"""
    p = planes.astype(np.float64)
    pts = []
    for pick in itertools.product((0, 1), repeat=3):
        m = np.stack([p[:, 2 * k + pick[k]] for k in range(3)], axis=1)              # [regions, 3 planes, 4]
        pts.append(np.linalg.solve(m[..., :3], -m[..., 3:])[..., 0])
    pts = np.stack(pts, axis=1)
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    return np.nextafter(lo.astype(np.float32), np.float32(-np.inf)), np.nextafter(hi.astype(np.float32), np.float32(np.inf))


def look_at(eye, target):
    z = eye - target
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    up = np.where(np.abs(z[:, 1:2]) < 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    x = np.cross(up, z)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(z, x)
    m = np.zeros((len(eye), 4, 4))
    m[:, :3, 0], m[:, :3, 1], m[:, :3, 2], m[:, :3, 3], m[:, 3, 3] = x, y, z, eye, 1.0
    return m


def main():
    ap = Q.arguments(launches=10, reps=5, warmup=2)
    ap.add_argument("--log2-regions", type=int, default=20)
    ap.add_argument("--size", type=float, default=3.0, help="region size in median triangle-box diagonals")
    ap.add_argument("--check", type=int, default=24, help="regions per set compared with the brute force")
    a = ap.parse_args()

    import region_reference as R
    import overlap_reference as V
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import host as HO
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = 1 << a.log2_regions
    tris = scenes.tiled_torus()
    nt = len(tris)
    ctx = Context(0)
    h, lib = ctx.handle, N.lib
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[:nt]
    lo, hi = box["min"][:, :3].copy(), box["max"][:, :3].copy()
    size = a.size * float(np.median(np.linalg.norm((hi - lo).astype(np.float64), axis=1)))
    rng = np.random.default_rng(37)
    k = rng.integers(0, nt, n)
    centre = (lo[k].astype(np.float64) + hi[k]) * 0.5
    # cubes turned about a random axis (Rodrigues), frusta looking at the triangle
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    kx = np.zeros((n, 3, 3))
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0], kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    rot = np.eye(3) + np.sin(angle)[:, None, None] * kx + (1.0 - np.cos(angle))[:, None, None] * (kx @ kx)
    cubes = HO.obb_planes(centre, rot, np.full((n, 3), 0.5 * size))
    view = rng.normal(size=(n, 3))
    view /= np.linalg.norm(view, axis=1, keepdims=True)
    dist = 8.0 * size
    inv = np.linalg.inv(look_at(centre + view * dist, centre))
    t = 0.5                                                       # the tangent of half the vertical angle; 64 x 64 pixels, tile (28 .. 36)^2
    e0, e1 = (-1.0 + 2.0 * 28 / 64) * t, (-1.0 + 2.0 * 36 / 64) * t
    cam = np.array([[1.0, 0.0, e0, 0.0], [-1.0, 0.0, -e1, 0.0], [0.0, 1.0, e0, 0.0], [0.0, -1.0, -e1, 0.0],
                    [0.0, 0.0, -1.0, -0.75 * dist], [0.0, 0.0, 1.0, 1.25 * dist]])
    frusta = R.make_regions((cam[None] @ inv).astype(np.float32))       # host.frustum_planes' arithmetic, for all regions at once
    one = HO.frustum_planes({"screen_width": 64, "screen_height": 64, "camera_fov": 0.5, "near_plane": 0.75 * dist,
                             "camera_to_world": look_at(centre[:1] + view[:1] * dist, centre[:1])[0].astype(np.float32)}, 1.25 * dist, rect=(28, 28, 36, 36))
    assert np.allclose(one["plane"][0], frusta["plane"][0], rtol=1e-5, atol=1e-4 * dist)

    offsets = DataBuffer(ctx, n + 1, np.uint64)
    flags = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    regions = DataBuffer(ctx, n, L.REGION)
    boxes = DataBuffer(ctx, n, L.AABB)

    def total_of(count=n):
        last = np.zeros(1, dtype=np.uint64)
        N.check(h, lib.lbvh_buffer_download(h, last.ctypes.data_as(C.c_void_p), C.c_void_p(offsets.device.value + 8 * count), 8))
        return int(last[0])

    def times(call):
        return Q.timed(ctx, call, None, a.launches, a.reps, a.warmup)

    res = {"workload": "region queries on the cfg2 mesh (%d triangles), 2^%d regions per set of %.3g units (%.3g triangle-box diagonals)"
                       % (nt, a.log2_regions, size, a.size), "launches": a.launches, "reps": a.reps, "sets": {}}
    for name, recs in (("cubes", cubes), ("frusta", frusta)):
        regions.local[:] = recs
        regions.sync()
        blo, bhi = corners_box(recs["plane"])
        boxes.local[:] = V.make_boxes(blo, bhi)
        boxes.sync()
        row = {}
        calls = (("touching", lambda o, t, cap: lib.lbvh_region_overlaps(h, regions.device, n, L.REGION_TOUCHING, C.byref(s), o, t, cap)),
                 ("contained", lambda o, t, cap: lib.lbvh_region_overlaps(h, regions.device, n, L.REGION_CONTAINED, C.byref(s), o, t, cap)),
                 ("box_overlaps", lambda o, t, cap: lib.lbvh_box_overlaps(h, boxes.device, n, C.byref(s), o, t, cap)))
        for form, fn in calls:
            count_only = lambda: fn(offsets.device, None, 0)
            N.check(h, count_only())
            m = total_of()
            off0 = offsets.get_data().copy()
            lst = DataBuffer(ctx, max(m, 1), np.uint32)
            fill = lambda: fn(offsets.device, lst.device, m)
            N.check(h, fill())
            off = offsets.get_data().copy()
            assert (off == off0).all() and int(off[-1]) == m, "count-only offsets " + form
            if form != "box_overlaps":                                # parity on a sample, before any number is printed
                mode = L.REGION_TOUCHING if form == "touching" else L.REGION_CONTAINED
                got = lst.get_data()
                N.check(h, lib.lbvh_region_overlaps_any(h, regions.device, n, mode, C.byref(s), flags.device))
                fl = flags.get_data()
                sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
                ro, rt = R.reference(recs[sub], lo, hi)[mode]
                for j, q in enumerate(sub):
                    seg = np.sort(got[int(off[q]):int(off[q + 1])])
                    assert len(seg) == int(ro[j + 1] - ro[j]) and (seg == rt[int(ro[j]):int(ro[j + 1])]).all(), (form, int(q))
                assert ((np.diff(off) > 0) == (fl == 1)).all()
            c = Q.counters(ctx, stats, count_only)
            lines, tests = Q.per_active(c)
            row[form] = {"M": m, "candidates_per_region": round(m / n, 3), "longest_segment": int(np.diff(off).max()),
                         "count_only": times(count_only), "node_lines_per_region": lines, "leaf_slots_per_region": tests}
            if form != "contained":
                row[form]["full"] = times(fill)
            lst.dispose()
        any_call = lambda: lib.lbvh_region_overlaps_any(h, regions.device, n, L.REGION_TOUCHING, C.byref(s), flags.device)
        row["touching"]["any"] = times(any_call)
        t_, b_ = row["touching"], row["box_overlaps"]
        row["time_ratio_workaround_over_region"] = {"count_only": round(b_["count_only"]["ms"] / t_["count_only"]["ms"], 3),
                                                    "full": round(b_["full"]["ms"] / t_["full"]["ms"], 3),
                                                    "count_only_workaround_over_any": round(b_["count_only"]["ms"] / t_["any"]["ms"], 3)}
        row["candidate_ratio_workaround_over_touching"] = round(b_["M"] / max(t_["M"], 1), 3)
        res["sets"][name] = row

    # the priced caveat: one frustum over about half the mesh, alone and among the small cubes
    pts = np.concatenate([lo, hi]).astype(np.float64)
    slo, shi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (slo + shi) * 0.5, float(np.linalg.norm(shi - slo))
    eye = mid + np.array([0.0, 0.0, 1.0]) * ext
    camera = {"screen_width": 64, "screen_height": 64, "camera_fov": 1.0, "near_plane": 0.01 * ext,
              "camera_to_world": look_at(eye[None], mid[None])[0].astype(np.float32)}
    big = HO.frustum_planes(camera, far=2.0 * ext, rect=(0, 0, 32, 64))  # the left half of a view that holds the whole mesh
    regions.local[:] = cubes
    regions.local[0] = big[0]
    regions.sync()
    alone = lambda: lib.lbvh_region_overlaps(h, regions.device, 1, L.REGION_TOUCHING, C.byref(s), offsets.device, None, 0)
    N.check(h, alone())
    m_big = total_of(1)
    among = lambda: lib.lbvh_region_overlaps(h, regions.device, n, L.REGION_TOUCHING, C.byref(s), offsets.device, None, 0)
    slow = lambda call: Q.timed(ctx, call, None, 2, 3, 1)              # (one lane walks half the mesh: few launches)
    res["one_large_frustum"] = {"candidates": m_big, "share_of_the_mesh": round(m_big / nt, 3), "alone_count_only": slow(alone),
                                "among_the_cubes_count_only": slow(among),
                                "the_cubes_without_it_count_only": res["sets"]["cubes"]["touching"]["count_only"]}
    Q.emit(res, a.out)
    for buf in (offsets, flags, stats, regions, boxes):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
