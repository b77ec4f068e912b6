#!/usr/bin/env python3
"""lbvh_sphere_cast / lbvh_sphere_cast_any on the cfg2 mesh (1 M triangles).  Prints one JSON line.

`--casts` spheres start on a sphere around the scene's box and aim at points inside it (unit directions, t_max = +inf), at the
radii 0.5 %, 2 % and 10 % of the scene's extent.  For each radius: time per call of both entry points, casts per second, node
lines and triangle tests per cast (lbvh_ray_stats_target on one more call), how many casts touch and how many start in overlap.
In the same process, on the same origins and directions: lbvh_trace_closest (t in (0, +inf)), the r -> 0 floor of the walk.

Before anything is printed the outputs are checked: the flags equal (t < LBVH_MAX_FLOAT) of the records on every cast, and
`--check` casts of each radius against tests/sweep_reference.py (brute force over all triangles, word for word).  Times: device
events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls (the clocks settle there); per call = median
over the reps (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RADII = (0.005, 0.02, 0.1)


def main():
    ap = Q.arguments(launches=10, reps=5, warmup=3)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=16, help="casts of each radius compared with the brute force")
    a = ap.parse_args()

    import sweep_reference as S
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = a.casts
    tris = scenes.tiled_torus()
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    pts = np.concatenate([ta, tb, tc])
    lo_s, hi_s = pts.min(axis=0), pts.max(axis=0)
    extent = float((hi_s - lo_s).max())
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[: len(tris)]
    lo, hi = box["min"].copy(), box["max"].copy()

    rng = np.random.default_rng(1)
    target = rng.uniform(lo_s, hi_s, (n, 3))
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    origin = (target - direction * (0.75 * np.linalg.norm(hi_s - lo_s) + 0.2 * extent)).astype(np.float32)
    direction = direction.astype(np.float32)

    casts = DataBuffer(ctx, n, L.SPHERE_RAY)
    rays = DataBuffer(ctx, n, L.RAY)
    rays.local["origin"], rays.local["dir"], rays.local["t_min"], rays.local["t_max"] = origin, direction, np.float32(0.0), np.float32(np.inf)
    rays.sync()
    rec = DataBuffer(ctx, n, L.HIT)
    flg = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(fn):
        steps, tests = Q.per_active(Q.counters(ctx, stats, fn))
        return {"steps_per_cast": steps, "triangle_tests_per_cast": tests}

    def times(fn):
        return Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mcasts_s")

    closest = lambda: N.lib.lbvh_trace_closest(h, rays.device, n, C.byref(s), rec.device)
    cast = lambda: N.lib.lbvh_sphere_cast(h, casts.device, n, C.byref(s), rec.device)
    cast_any = lambda: N.lib.lbvh_sphere_cast_any(h, casts.device, n, C.byref(s), flg.device)
    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d casts from outside the box at points inside it, unit directions, open range"
                       % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps,
           "checks": "flags == (t < LBVH_MAX_FLOAT) on every cast; records and flags word for word against the brute force on %d casts "
                     "of each radius: hold" % a.check,
           "trace_closest": {**times(closest), **work(closest)}, "radius": {}}
    for radius in RADII:
        casts.local["origin"], casts.local["dir"] = origin, direction
        casts.local["radius"], casts.local["t_max"] = np.float32(radius * extent), np.float32(np.inf)
        casts.sync()
        # ---- checks, before any number of this radius is kept
        N.check(h, cast())
        N.check(h, cast_any())
        got, flags = rec.get_data().copy(), flg.get_data().copy()
        assert ((got["t"] < L.MAX_FLOAT) == (flags == 1)).all(), "flags == touching, radius %g" % radius
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = S.reference(casts.local[sub], ta, tb, tc, lo, hi, casts_per_chunk=1)
        assert (np.ascontiguousarray(got[sub]).view(np.uint32) == ref.records.view(np.uint32)).all(), "records, radius %g" % radius
        assert (flags[sub] == ref.flags).all(), "flags, radius %g" % radius
        res["radius"][str(radius)] = {"radius": round(radius * extent, 4), "touching": int(flags.sum()), "start_in_overlap": int((got["t"] == 0).sum()),
                                      "sphere_cast": {**times(cast), **work(cast)},
                                      "sphere_cast_any": {**times(cast_any), **work(cast_any)}}
    Q.emit(res, a.out)
    for b in (casts, rays, rec, flg, stats):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
