#!/usr/bin/env python3
"""lbvh_box_cast on the cfg2 mesh (1 M triangles) against the two sphere casts a caller had before it.  Prints one JSON line.

`--casts` boxes start on a sphere around the scene's box and aim at points inside it (unit directions, t_max = +inf; the origins
and directions of tools/sphere_cast_bench.py): cubes of half extent 0.5 %, 2 % and 10 % of the scene's extent, turned at random.
For each size, in the same process on the same origins and directions:
    box_cast           lbvh_box_cast
    sphere_inscribed   lbvh_sphere_cast with the radius of the inscribed sphere (the half extent): a floor — smaller boxes in the
                       tree, a cheaper triangle test
    sphere_workaround  lbvh_sphere_cast with the radius of the circumscribed sphere (half extent * sqrt 3): the conservative
                       stand-in the box cast replaces
each with the time per call, casts per second, node steps and triangle lines per cast (lbvh_ray_stats_target on one more call) and
how many casts touch; the ratios box / inscribed and box / workaround of the times; and the share of casts on which the
workaround's answer differs from the box cast's (touches where the box does not, or a time that differs by more than 1e-3 of the
scene's extent).

Before anything is printed the outputs are checked: `--check` casts of each size against tests/box_cast_reference.py (brute force
over all triangles, word for word), and lbvh_box_cast_any's flags equal (t < LBVH_MAX_FLOAT) on every cast.
Times: device events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls; per call = median over the
reps (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (0.005, 0.02, 0.1)


def main():
    ap = Q.arguments(launches=5, reps=5, warmup=2)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=8, help="casts of each size compared with the brute force")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="half extents, of the scene's extent")
    a = ap.parse_args()

    import box_cast_reference as BR
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
    turn = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]               # columns: the cube's axes

    boxes = DataBuffer(ctx, n, L.BOX_RAY)
    sph = DataBuffer(ctx, n, L.SPHERE_RAY)
    rec = DataBuffer(ctx, n, L.BOX_HIT)
    srec = DataBuffer(ctx, n, L.HIT)
    flg = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def measure(fn, out):
        steps, tests = Q.per_active(Q.counters(ctx, stats, fn))
        touching = int((out.get_data()["t"] < L.MAX_FLOAT).sum())
        return {**Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mcasts_s"), "steps_per_cast": steps,
                "triangle_lines_per_cast": tests, "touching": touching}

    cast = lambda: N.lib.lbvh_box_cast(h, boxes.device, n, C.byref(s), rec.device)
    cast_any = lambda: N.lib.lbvh_box_cast_any(h, boxes.device, n, C.byref(s), flg.device)
    sphere = lambda: N.lib.lbvh_sphere_cast(h, sph.device, n, C.byref(s), srec.device)

    def spheres(radius):
        sph.local["origin"], sph.local["dir"] = origin, direction
        sph.local["radius"], sph.local["t_max"] = np.float32(radius), np.float32(np.inf)
        sph.sync()

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d casts from outside the box at points inside it, unit directions, open "
                       "range, cubes turned at random" % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps,
           "checks": "box_cast_any's flags == (t < LBVH_MAX_FLOAT) on every cast; records word for word against the brute force on %d "
                     "casts of each size: hold" % a.check,
           "cases": {}}
    for size in a.sizes:
        half = size * extent
        axes = (turn * half).astype(np.float32)
        boxes.local["centre"], boxes.local["dir"], boxes.local["t_max"] = origin, direction, np.float32(np.inf)
        boxes.local["ax"], boxes.local["ay"], boxes.local["az"] = axes[:, :, 0], axes[:, :, 1], axes[:, :, 2]
        boxes.sync()
        # ---- checks, before any number of this case is kept
        N.check(h, cast())
        N.check(h, cast_any())
        got, flags = rec.get_data().copy(), flg.get_data().copy()
        assert ((got["t"] < L.MAX_FLOAT) == (flags == 1)).all(), "flags == touching, size %g" % size
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = BR.reference(boxes.local[sub], ta, tb, tc, lo, hi, casts_per_chunk=1)
        assert (np.ascontiguousarray(got[sub]).view(np.uint32) == ref.records.view(np.uint32)).all(), "records, size %g" % size
        case = {"half_extent": round(half, 4), "box_cast": measure(cast, rec)}
        spheres(half)
        case["sphere_inscribed"] = measure(sphere, srec)
        spheres(half * np.sqrt(3.0))
        case["sphere_workaround"] = measure(sphere, srec)
        around = srec.get_data()["t"]
        differs = ((around < L.MAX_FLOAT) != (got["t"] < L.MAX_FLOAT)) | \
                  ((got["t"] < L.MAX_FLOAT) & (np.abs(np.minimum(around, 1e30) - got["t"]) > 1e-3 * extent))
        case["workaround_differs_share"] = round(float(differs.mean()), 4)
        case["box_over_inscribed"] = round(case["box_cast"]["ms"] / case["sphere_inscribed"]["ms"], 2)
        case["box_over_workaround"] = round(case["box_cast"]["ms"] / case["sphere_workaround"]["ms"], 2)
        res["cases"]["half=%g" % size] = case
    Q.emit(res, a.out)
    for b in (boxes, sph, rec, srec, flg, stats):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
