#!/usr/bin/env python3
"""lbvh_count_hits and lbvh_point_crossings on the cfg2 mesh (1 M triangles).  Prints one JSON line.

  (a) count against closest and occlusion at 1920x1080, on the same buffers: the first-bounce rays of lbvh_path_first_bounce
      (live rays only, compacted on the host; t in (1e-3, +inf)) and shadow rays from every primary hit toward a point light
      outside the scene box (t in (1e-4, 1); pixels without a hit: inactive).  ms, node fetches and triangle tests per active ray.
  (b) lbvh_point_crossings with the three default directions on 2^20 points (uniform in the scene box, and near the surface:
      triangle points moved by N(0, 0.5)) against lbvh_count_hits on the same 3 * 2^20 rays written out point-major (the order
      the kernel walks them), timed alternately in the same process.  Bar: crossings <= count + 3 * the larger min-max spread.

Before anything is printed the outputs are checked: count >= 1 <=> occluded; with t_max = the closest t the count is 0 and
with t_max one ulp above it >= 1 (a); every parity bit == its ray's count AND 1 (b).  Times: device events around `--launches`
back-to-back calls, `--reps` times after `--warmup` calls; per call = median over the reps (min / max beside it)."""
import ctypes as C
import json
import os
import sys

import numpy as np

import query_bench as Q
from query_bench import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32


def main():
    ap = Q.arguments(launches=100, reps=5, warmup=10)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--crossings-out", default=None, help="write part (b) alone here")
    a = ap.parse_args()

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import DEFAULT_DIRS, Context, DataBuffer, RaytracingMeshDrawer

    W, Ht = 1920, 1080
    n = W * Ht
    ctx = Context(0)
    h = ctx.handle
    tris = scenes.tiled_torus()
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))

    first, live, hit, origin, set_buffers = Q.ray_sets(ctx, s, cam, W, Ht)
    sec = Q.ray_buffer(ctx, first["origin"][live], first["dir"][live], F(1e-3), F(np.inf))     # the live rays only
    shadow = Q.ray_buffer(ctx, origin, (LIGHT - origin).astype(F), F(1e-4), np.where(hit, F(1.0), F(0.0)))
    out_hits = DataBuffer(ctx, n, L.HIT)
    out_u32 = DataBuffer(ctx, max(3 * a.points, n), np.uint32)      # part (a) writes one word per pixel into it, whatever --points is

    def call(fn, rays):
        return lambda: fn(h, rays.device, rays.size, C.byref(s), out_hits.device if fn is N.lib.lbvh_trace_closest else out_u32.device)

    calls = {}
    for tag, rays in (("first_bounce_live", sec), ("shadow", shadow)):
        calls[tag + "_count"] = call(N.lib.lbvh_count_hits, rays)
        calls[tag + "_closest"] = call(N.lib.lbvh_trace_closest, rays)
        calls[tag + "_occluded"] = call(N.lib.lbvh_trace_occluded, rays)

    # ---- checks of (a), before any number is printed
    def u32(name, size):
        out_u32.fill_u32(0xDEADBEEF)
        N.check(h, calls[name]())
        return out_u32.get_data()[:size].copy()

    active = {}
    for tag, rays in (("first_bounce_live", sec), ("shadow", shadow)):
        cnt, occ = u32(tag + "_count", rays.size), u32(tag + "_occluded", rays.size)
        assert ((cnt >= 1) == (occ == 1)).all(), tag
        N.check(h, calls[tag + "_closest"]())
        t = out_hits.get_data()[: rays.size]["t"].copy()
        act = rays.local["t_min"] < rays.local["t_max"]
        active[tag] = int(act.sum())
        got = act & (t < L.MAX_FLOAT)
        keep = rays.local["t_max"].copy()
        for bound, check in ((t, lambda c: (c[got] == 0).all()), (np.nextafter(t, F(np.inf)), lambda c: (c[got] >= 1).all())):
            rays.local["t_max"] = np.where(got, bound, keep)
            rays.sync()
            assert check(u32(tag + "_count", rays.size)), tag
        rays.local["t_max"] = keep
        rays.sync()

    # ---- (b) the point sets and the materialised rays
    rng = np.random.default_rng(5)
    a_, b_, c_ = (np.ascontiguousarray(tris[k][:, :3], dtype=F) for k in "abc")
    lo, hi = np.minimum(np.minimum(a_, b_), c_).min(axis=0), np.maximum(np.maximum(a_, b_), c_).max(axis=0)
    k = rng.integers(0, len(a_), a.points)
    w = rng.dirichlet((1, 1, 1), a.points).astype(F)
    point_sets = {"uniform": rng.uniform(lo, hi, (a.points, 3)).astype(F),
                  "near_surface": (a_[k] * w[:, :1] + b_[k] * w[:, 1:2] + c_[k] * w[:, 2:] + rng.normal(0, 0.5, (a.points, 3))).astype(F)}
    dirs = np.ascontiguousarray(DEFAULT_DIRS)
    dptr = dirs.ctypes.data_as(C.POINTER(C.c_float))
    pbuf = DataBuffer(ctx, a.points, L.POINT_QUERY)
    rbuf = DataBuffer(ctx, 3 * a.points, L.RAY)
    parity = DataBuffer(ctx, a.points, np.uint32)

    def load(pts):
        pbuf.local["p"], pbuf.local["max_dist2"] = pts, F(np.inf)
        pbuf.sync()
        rbuf.local["origin"] = np.repeat(pts, 3, axis=0)
        rbuf.local["dir"] = np.tile(dirs, (a.points, 1))
        rbuf.local["t_min"], rbuf.local["t_max"] = F(0), F(np.inf)
        rbuf.sync()

    cross_calls = {"crossings": lambda: N.lib.lbvh_point_crossings(h, pbuf.device, a.points, dptr, 3, C.byref(s), parity.device),
                   "materialised_count": lambda: N.lib.lbvh_count_hits(h, rbuf.device, rbuf.size, C.byref(s), out_u32.device)}

    # ---- work per ray
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(fn):
        c = Q.counters(ctx, stats, fn)
        fetches, tests = Q.per_active(c)
        return {"rays": c.rays, "node_fetches_per_ray": fetches, "triangle_tests_per_ray": tests}

    res = {"workload": "lbvh_count_hits / lbvh_point_crossings on the cfg2 mesh (1 M triangles)", "launches": a.launches, "reps": a.reps,
           "checks": "count >= 1 <=> occluded; count(t_max = t*) == 0, count(nextafter(t*)) >= 1; parity bit == count AND 1: hold",
           "a": {}, "b": {}}
    for name, fn in calls.items():
        tag = name.rsplit("_", 1)[0]
        res["a"][name] = {**Q.timed(ctx, fn, None, a.launches, a.reps, a.warmup), "active_rays": active[tag], **work(fn)}
    events = (ctx.event(), ctx.event())
    for set_name, pts in point_sets.items():
        load(pts)
        parity.fill_u32(0xDEADBEEF)
        N.check(h, cross_calls["crossings"]())
        N.check(h, cross_calls["materialised_count"]())
        par = parity.get_data().copy()
        cnt = out_u32.get_data()[: 3 * a.points].reshape(-1, 3)
        want = (cnt[:, 0] & 1) | ((cnt[:, 1] & 1) << 1) | ((cnt[:, 2] & 1) << 2)
        assert (par == want).all(), set_name
        for fn in cross_calls.values():
            for _ in range(a.warmup):
                N.check(h, fn())
        per = {k: [] for k in cross_calls}
        for _ in range(a.reps):                                   # alternating
            for k2, fn in cross_calls.items():
                per[k2].append(Q.rep(ctx, events, fn, a.launches))
        row = {k2: {**Q.summary(v), **work(cross_calls[k2])} for k2, v in per.items()}
        spread = max(row[k2]["ms_max"] - row[k2]["ms_min"] for k2 in row)
        bar = row["materialised_count"]["ms"] + 3 * spread
        row.update(points=a.points, directions=3, inside_majority=int((np.unpackbits(par.view(np.uint8)).reshape(-1, 32).sum(axis=1) >= 2).sum()),
                   bar_ms=round(bar, 4), bar_holds=bool(row["crossings"]["ms"] <= bar))
        res["b"][set_name] = row
    Q.emit(res, a.out)
    if a.crossings_out:
        with open(a.crossings_out, "w") as f:
            f.write(json.dumps({"workload": res["workload"], "launches": a.launches, "reps": a.reps, **res["b"]}) + "\n")
    for b in set_buffers + [sec, shadow, out_hits, out_u32, pbuf, rbuf, parity, stats]:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
