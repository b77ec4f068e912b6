#!/usr/bin/env python3
"""lbvh_triangle_cast on the cfg2 mesh (1 M triangles) against the two stand-ins a caller had before it.  Prints one JSON line.

`--casts` triangles start on a sphere around the scene's box and move 10 % of the scene's extent per unit of t towards points inside
it (open range; the origins and directions of tools/sphere_cast_bench.py, the directions scaled): triangles with edges of 0.5 %,
2 % and 10 % of the extent, turned at random.  For each size, in the same process on the same origins and directions, in
interleaved rounds (one repetition of each arm per round):
    triangle_cast     lbvh_triangle_cast
    three_rays        three lbvh_trace_closest calls, one from each vertex along dir (t_min = 0): blind to every edge against an
                      edge and to every scene vertex that pokes into the moving face
    sphere_workaround lbvh_sphere_cast with the circumscribed radius from the circumcentre: stops too early
each with the time per call (three_rays: per three calls), casts per second, and for the cast the node steps and triangle lines per
cast (lbvh_ray_stats_target on one more call) and how many casts touch; the ratios of the times; the share of casts on which each
stand-in's answer differs from the cast's (touches where the other does not, or a time that differs by more than 1e-3 of the
extent, in units of distance); and how the winning features split between vertex / face (0 - 5), edge / edge (6 - 14) and a start in
overlap.

Before anything is printed the outputs are checked: `--check` casts of each size against tests/triangle_cast_reference.py (brute
force over all triangles, word for word), and lbvh_triangle_cast_any's flags equal (t < LBVH_MAX_FLOAT) on every cast.
Times: device events around `--launches` back-to-back calls, `--reps` rounds after `--warmup` calls of each arm; per call = median
over the rounds (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (0.005, 0.02, 0.1)
MOVE = 0.1


def main():
    ap = Q.arguments(launches=5, reps=5, warmup=2)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=8, help="casts of each size compared with the brute force")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="edge lengths, of the scene's extent")
    a = ap.parse_args()

    import triangle_cast_reference as TR
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
    unit_dir = rng.normal(size=(n, 3))
    unit_dir /= np.linalg.norm(unit_dir, axis=1, keepdims=True)
    origin = target - unit_dir * (0.75 * np.linalg.norm(hi_s - lo_s) + 0.2 * extent)
    speed = MOVE * extent
    direction = (unit_dir * speed).astype(np.float32)
    turn = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]               # columns 0 and 1: the triangle's plane

    casts = DataBuffer(ctx, n, L.TRI_RAY)
    rays = [DataBuffer(ctx, n, L.RAY) for _ in range(3)]
    sph = DataBuffer(ctx, n, L.SPHERE_RAY)
    rec = DataBuffer(ctx, n, L.TRI_CAST_HIT)
    rrec = [DataBuffer(ctx, n, L.HIT) for _ in range(3)]
    srec = DataBuffer(ctx, n, L.HIT)
    flg = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    cast = lambda: N.lib.lbvh_triangle_cast(h, casts.device, n, C.byref(s), rec.device)
    cast_any = lambda: N.lib.lbvh_triangle_cast_any(h, casts.device, n, C.byref(s), flg.device)
    sphere = lambda: N.lib.lbvh_sphere_cast(h, sph.device, n, C.byref(s), srec.device)

    def three_rays():
        for r, out in zip(rays, rrec):
            rc = N.lib.lbvh_trace_closest(h, r.device, n, C.byref(s), out.device)
            if rc != 0:
                return rc
        return 0

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d triangles from outside the box at points inside it, moving %g of the "
                       "extent per unit of t, open range, turned at random" % (len(tris), extent, n, MOVE),
           "launches": a.launches, "reps": a.reps,
           "checks": "triangle_cast_any's flags == (t < LBVH_MAX_FLOAT) on every cast; records word for word against the brute force on "
                     "%d casts of each size: hold" % a.check,
           "cases": {}}
    for size in a.sizes:
        edge = size * extent
        # an equilateral triangle of that edge around `origin`, in the plane of the first two columns of `turn`
        ring = [np.array([np.cos(w), np.sin(w)]) * edge / np.sqrt(3.0) for w in (0.5 * np.pi, 0.5 * np.pi + 2.0 * np.pi / 3.0, 0.5 * np.pi + 4.0 * np.pi / 3.0)]
        verts = [(origin + turn[:, :, 0] * p[0] + turn[:, :, 1] * p[1]).astype(np.float32) for p in ring]
        casts.local["a"], casts.local["b"], casts.local["c"] = verts
        casts.local["dir"], casts.local["t_max"], casts.local["skip"] = direction, np.float32(np.inf), L.NULL
        casts.sync()
        for r, v in zip(rays, verts):
            r.local["origin"], r.local["dir"], r.local["t_min"], r.local["t_max"] = v, direction, np.float32(0), np.float32(np.inf)
            r.sync()
        sph.local["origin"], sph.local["dir"] = origin.astype(np.float32), direction
        sph.local["radius"], sph.local["t_max"] = np.float32(edge / np.sqrt(3.0)), np.float32(np.inf)
        sph.sync()
        # ---- checks, before any number of this case is kept
        N.check(h, cast())
        N.check(h, cast_any())
        got, flags = rec.get_data().copy(), flg.get_data().copy()
        touch = got["t"] < L.MAX_FLOAT
        assert (touch == (flags == 1)).all(), "flags == touching, size %g" % size
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = TR.reference(casts.local[sub], ta, tb, tc, lo, hi, casts_per_chunk=1)
        assert (np.ascontiguousarray(got[sub]).view(np.uint32) == ref.records.view(np.uint32)).all(), "records, size %g" % size
        # ---- interleaved rounds
        arms = {"triangle_cast": cast, "three_rays": three_rays, "sphere_workaround": sphere}
        for fn in arms.values():
            for _ in range(a.warmup):
                N.check(h, fn())
        events = (ctx.event(), ctx.event())
        per = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                per[k].append(Q.rep(ctx, events, fn, a.launches))
        for e in events:
            ctx.destroy_event(e)
        steps, tests = Q.per_active(Q.counters(ctx, stats, cast))
        case = {"edge": round(edge, 4)}
        for k in arms:
            case[k] = Q.summary(per[k], n, "Mcasts_s")
        case["triangle_cast"].update({"steps_per_cast": steps, "triangle_lines_per_cast": tests, "touching": int(touch.sum())})
        ray_t = np.minimum.reduce([r.get_data()["t"] for r in rrec])
        sphere_t = srec.get_data()["t"]

        def differs(other):
            on = other < L.MAX_FLOAT
            return round(float(((on != touch) | (touch & on & (np.abs(np.where(on, other, 0.0) - np.where(touch, got["t"], 0.0)) * speed > 1e-3 * extent))).mean()), 4)

        case["three_rays_differ_share"] = differs(ray_t)
        case["sphere_differs_share"] = differs(sphere_t)
        case["cast_over_three_rays"] = round(case["triangle_cast"]["ms"] / case["three_rays"]["ms"], 2)
        case["cast_over_sphere"] = round(case["triangle_cast"]["ms"] / case["sphere_workaround"]["ms"], 2)
        f = got["feature"][touch]
        m = max(int(touch.sum()), 1)
        case["features"] = {"vertex_face": round(float((f < 6).sum()) / m, 4), "edge_edge": round(float(((f >= 6) & (f < 15)).sum()) / m, 4),
                            "start_overlap": round(float((f >= L.TRI_CAST_START).sum()) / m, 4)}
        res["cases"]["edge=%g" % size] = case
    Q.emit(res, a.out)
    for b in [casts, sph, rec, srec, flg, stats] + rays + rrec:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
