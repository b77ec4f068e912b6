#!/usr/bin/env python3
"""lbvh_capsule_cast on the cfg2 mesh (1 M triangles) against the two sphere casts a caller had before it.  Prints one JSON line.

`--casts` capsules start on a sphere around the scene's box and aim at points inside it (unit directions, t_max = +inf; the origins
and directions of tools/sphere_cast_bench.py), at the radii 0.5 %, 2 % and 10 % of the scene's extent and axis lengths of 0, 2 and
8 radii, the axis in a random direction.  For each (radius, length), in the same process on the same origins and directions:
    capsule_cast       lbvh_capsule_cast
    sphere_floor       lbvh_sphere_cast with radius r: one of the eight tests per triangle and smaller boxes
    sphere_workaround  lbvh_sphere_cast with radius r + |axis| / 2 from the middle of the axis: the conservative stand-in
each with the time per call, casts per second, node lines and triangle lines per cast (lbvh_ray_stats_target on one more call) and
how many casts touch; and the ratios capsule / floor and capsule / workaround of the times.

Before anything is printed the outputs are checked: `--check` casts of each (radius, length) against tests/capsule_reference.py
(brute force over all triangles, word for word), and lbvh_capsule_cast_any's flags equal (t < LBVH_MAX_FLOAT) on every cast.
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

RADII = (0.005, 0.02, 0.1)
LENGTHS = (0.0, 2.0, 8.0)


def main():
    ap = Q.arguments(launches=5, reps=5, warmup=2)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=8, help="casts of each (radius, length) compared with the brute force")
    ap.add_argument("--radii", type=float, nargs="+", default=list(RADII), help="of the scene's extent")
    a = ap.parse_args()

    import capsule_reference as CR
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
    unit = rng.normal(size=(n, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)

    caps = DataBuffer(ctx, n, L.CAPSULE_RAY)
    sph = DataBuffer(ctx, n, L.SPHERE_RAY)
    rec = DataBuffer(ctx, n, L.HIT)
    flg = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def measure(fn):
        steps, tests = Q.per_active(Q.counters(ctx, stats, fn))
        touching = int((rec.get_data()["t"] < L.MAX_FLOAT).sum())
        return {**Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mcasts_s"), "steps_per_cast": steps,
                "triangle_lines_per_cast": tests, "touching": touching}

    capsule = lambda: N.lib.lbvh_capsule_cast(h, caps.device, n, C.byref(s), rec.device)
    capsule_any = lambda: N.lib.lbvh_capsule_cast_any(h, caps.device, n, C.byref(s), flg.device)
    sphere = lambda: N.lib.lbvh_sphere_cast(h, sph.device, n, C.byref(s), rec.device)

    def spheres(centre, radius):
        sph.local["origin"], sph.local["dir"] = centre, direction
        sph.local["radius"], sph.local["t_max"] = np.float32(radius), np.float32(np.inf)
        sph.sync()

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d casts from outside the box at points inside it, unit directions, open "
                       "range, axes in random directions" % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps,
           "checks": "capsule_cast_any's flags == (t < LBVH_MAX_FLOAT) on every cast; records word for word against the brute force on %d "
                     "casts of each (radius, length): hold" % a.check,
           "cases": {}}
    for radius in a.radii:
        r = np.float32(radius * extent)
        for length in LENGTHS:
            axis = (unit * (length * float(r))).astype(np.float32)
            caps.local["origin"], caps.local["dir"], caps.local["axis"] = origin, direction, axis
            caps.local["radius"], caps.local["t_max"] = r, np.float32(np.inf)
            caps.sync()
            # ---- checks, before any number of this case is kept
            N.check(h, capsule())
            N.check(h, capsule_any())
            got, flags = rec.get_data().copy(), flg.get_data().copy()
            assert ((got["t"] < L.MAX_FLOAT) == (flags == 1)).all(), "flags == touching, radius %g length %g" % (radius, length)
            sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
            ref = CR.reference(caps.local[sub], ta, tb, tc, lo, hi, casts_per_chunk=1)
            assert (np.ascontiguousarray(got[sub]).view(np.uint32) == ref.records.view(np.uint32)).all(), "records, radius %g length %g" % (radius, length)
            case = {"radius": round(float(r), 4), "axis_length": round(length * float(r), 4), "capsule_cast": measure(capsule)}
            spheres(origin, r)
            case["sphere_floor"] = measure(sphere)
            spheres(origin + axis * np.float32(0.5), np.float32(float(r) * (1.0 + 0.5 * length)))
            case["sphere_workaround"] = measure(sphere)
            case["capsule_over_floor"] = round(case["capsule_cast"]["ms"] / case["sphere_floor"]["ms"], 2)
            case["capsule_over_workaround"] = round(case["capsule_cast"]["ms"] / case["sphere_workaround"]["ms"], 2)
            res["cases"]["r=%g,len=%gr" % (radius, length)] = case
    Q.emit(res, a.out)
    for b in (caps, sph, rec, flg, stats):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
