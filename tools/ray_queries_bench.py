#!/usr/bin/env python3
"""lbvh_trace_closest / lbvh_trace_occluded on the cfg2 mesh (1 M triangles) at 1920x1080.  Prints one JSON line.

  (a) first-bounce secondary rays (lbvh_path_first_bounce's states): lbvh_trace_rays on the path states against
      lbvh_trace_closest on the same rays as lbvh_ray records (dead paths: inactive rays), t_min = 1e-3, t_max = +inf
  (b) shadow rays from every primary hit toward a point light outside the scene box (dir = light - hit point, not
      normalised; t in (1e-4, 1); pixels without a hit: inactive): lbvh_trace_closest against lbvh_trace_occluded
  (c) lbvh_trace_occluded on the rays of (a)
(a) is also timed on a buffer that holds only the live rays (compacted on the host): the price of inactive rays left in place.

Before anything is printed the outputs are checked against the header's equalities, GPU against GPU: E1 (a)'s two record
arrays word for word; E2 (b)'s closest records == the unbounded closest records where t < 1, else the miss record; E3 every
occlusion flag == (active and unbounded t < min(t_max, MAX_FLOAT)).  Times: device events around `--launches` back-to-back
calls, `--reps` times after `--warmup` calls; per call = median over the reps (min / max beside it).  Node fetches and
triangle tests per active ray: lbvh_ray_stats_target on one more call of each (the four-wide walker, the default)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q
from query_bench import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = Q.arguments(launches=100, reps=5, warmup=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    W, Ht = a.width, a.height
    n = W * Ht
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, scenes.tiled_torus()).awake()
    s = d.container.scene()
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))

    # primary hits + first-bounce states
    first, live, hit, origin, set_buffers = Q.ray_sets(ctx, s, cam, W, Ht)
    states = set_buffers[0]                                  # the first-bounce states on the device

    sec = Q.ray_buffer(ctx, first["origin"], first["dir"], np.float32(1e-3), np.where(live, np.float32(np.inf), np.float32(0.0)))
    # (a) once more with the live rays only, compacted on the host: what the inactive rays left in place cost
    sec_live = DataBuffer(ctx, int(live.sum()), L.RAY)
    sec_live.local[:] = sec.local[live]
    sec_live.sync()
    shadow_bound = np.where(hit, np.float32(1.0), np.float32(0.0))
    shadow = Q.ray_buffer(ctx, origin, (LIGHT - origin).astype(np.float32), np.float32(1e-4), shadow_bound)
    shadow_inf = Q.ray_buffer(ctx, origin, (LIGHT - origin).astype(np.float32), np.float32(1e-4), np.where(hit, np.float32(np.inf), np.float32(0.0)))
    out_hits = DataBuffer(ctx, n, L.HIT)
    out_flags = DataBuffer(ctx, n, np.uint32)

    calls = {
        "a_trace_rays": lambda: N.lib.lbvh_trace_rays(h, states.device, n, 1e-3, C.byref(s), out_hits.device),
        "a_trace_closest": lambda: N.lib.lbvh_trace_closest(h, sec.device, n, C.byref(s), out_hits.device),
        "a_trace_closest_live_only": lambda: N.lib.lbvh_trace_closest(h, sec_live.device, sec_live.size, C.byref(s), out_hits.device),
        "b_trace_closest": lambda: N.lib.lbvh_trace_closest(h, shadow.device, n, C.byref(s), out_hits.device),
        "b_trace_occluded": lambda: N.lib.lbvh_trace_occluded(h, shadow.device, n, C.byref(s), out_flags.device),
        "c_trace_occluded": lambda: N.lib.lbvh_trace_occluded(h, sec.device, n, C.byref(s), out_flags.device),
    }

    def run(name, out):
        out.fill_u32(0x7FC00000)
        N.check(h, calls[name]())
        return out.get_data().copy()

    # ---- the equalities, before any number is printed
    MAXF = L.MAX_FLOAT
    a_rays = run("a_trace_rays", out_hits)
    a_closest = run("a_trace_closest", out_hits)
    assert (a_rays.view(np.uint32) == a_closest.view(np.uint32)).all(), "E1"
    a_live = run("a_trace_closest_live_only", out_hits)[: int(live.sum())]
    assert (a_live.view(np.uint32) == a_rays[live].view(np.uint32)).all(), "E1 (live rays only)"
    c_occ = run("c_trace_occluded", out_flags)
    assert (c_occ == (live & (a_closest["t"] < MAXF))).all(), "E3 (c)"
    b_closest = run("b_trace_closest", out_hits)
    b_occ = run("b_trace_occluded", out_flags)
    N.check(h, N.lib.lbvh_trace_closest(h, shadow_inf.device, n, C.byref(s), out_hits.device))
    b_unb = out_hits.get_data().copy()
    keep = hit & (b_unb["t"] < 1.0)
    want = np.zeros(n, dtype=L.HIT)
    want["t"] = MAXF
    want[keep] = b_unb[keep]
    assert (b_closest.view(np.uint32) == want.view(np.uint32)).all(), "E2 (b)"
    assert (b_occ == keep).all(), "E3 (b)"

    # ---- work per ray
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(name):
        c = Q.counters(ctx, stats, calls[name])
        fetches, tests = Q.per_active(c)
        return {"rays": c.rays, "node_fetches_per_ray": fetches, "triangle_tests_per_ray": tests}

    # ---- times
    res = {"workload": "ray queries on the cfg2 mesh (1 M triangles), %dx%d" % (W, Ht), "launches": a.launches, "reps": a.reps,
           "equalities": "E1 (a) word for word, E2 (b), E3 (b) and (c): hold", "sets": {}}
    active = {"a": int(live.sum()), "b": int(hit.sum()), "c": int(live.sum())}
    for name in calls:
        k = name[0]
        t = Q.timed(ctx, calls[name], active[k], a.launches, a.reps, a.warmup)
        res["sets"][name] = {"ms": t["ms"], "ms_min": t["ms_min"], "ms_max": t["ms_max"],
                             "rays_in_buffer": int(live.sum()) if "live_only" in name else n, "active_rays": active[k],
                             "Mrays_s_active": t["Mrays_s_active"], **work(name)}
    res["sets"]["b_trace_occluded"]["occluded_rays"] = int(b_occ.sum())
    res["sets"]["c_trace_occluded"]["occluded_rays"] = int(c_occ.sum())
    Q.emit(res, a.out)
    for b in set_buffers + [sec, sec_live, shadow, shadow_inf, out_hits, out_flags, stats]:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
