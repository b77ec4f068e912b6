#!/usr/bin/env python3
"""lbvh_trace_k_closest on the cfg2 mesh (1 M triangles) at 1920x1080, on the rays of tools/ray_queries_bench.py.  Prints one
JSON line.

  (a) first-bounce secondary rays (lbvh_path_first_bounce's states as lbvh_ray records; dead paths: inactive rays),
      t_min = 1e-3, t_max = +inf
  (b) shadow rays from every primary hit toward a point light outside the scene box (dir = light - hit point, not normalised;
      t in (1e-4, 1); pixels without a hit: inactive)
For k in --ks on each set: time per call, active rays per second, node lines and triangle tests per active ray
(lbvh_ray_stats_target on one more call), the found counts' sum and the full rows, LDS per wave and the waves per CU that
leaves.  In the same process, on the same buffers: lbvh_trace_closest, the yardstick for k = 1 (the same decisions plus the
list), and lbvh_count_hits, the yardstick for k = 32 (the walk without a shrinking bound).

Before anything is printed the outputs are checked, GPU against GPU on every ray and for every k: record 0 of every row ==
lbvh_trace_closest's record word for word (k = 1: the whole output), found == min(k, lbvh_count_hits); and `--check` rays of
each set against tests/k_hits_reference.py (brute force over all triangles, word for word).  Times: device events around
`--launches` back-to-back calls, `--reps` times after `--warmup` calls (the clocks settle there); per call = median over the
reps (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q
from query_bench import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LDS_PER_CU = 160 * 1024          # gfx950
STACK_LDS = 16 * 64 * 4          # the walk's 16-entry stack


def main():
    ap = Q.arguments(launches=20, reps=5, warmup=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--check", type=int, default=16, help="rays of each set compared with the brute force")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]

    import k_hits_reference as K
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    W, Ht = a.width, a.height
    n = W * Ht
    tris = scenes.tiled_torus()
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[: len(tris)]
    lo, hi = box["min"].copy(), box["max"].copy()
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))

    # primary hits + first-bounce states, as tools/ray_queries_bench.py makes them
    first, live, hit, origin, set_buffers = Q.ray_sets(ctx, s, cam, W, Ht)
    sets = {"a": (Q.ray_buffer(ctx, first["origin"], first["dir"], np.float32(1e-3), np.where(live, np.float32(np.inf), np.float32(0.0))), int(live.sum())),
            "b": (Q.ray_buffer(ctx, origin, (LIGHT - origin).astype(np.float32), np.float32(1e-4), np.where(hit, np.float32(1.0), np.float32(0.0))),
                  int(hit.sum()))}
    rows = DataBuffer(ctx, n * max(ks), L.HIT)
    found = DataBuffer(ctx, n, np.uint32)
    rec = DataBuffer(ctx, n, L.HIT)
    cnt = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(fn):
        lines, tests = Q.per_active(Q.counters(ctx, stats, fn))
        return {"node_lines_per_ray": lines, "triangle_tests_per_ray": tests}

    def times(fn, active):
        return Q.timed(ctx, fn, active, a.launches, a.reps, a.warmup)

    res = {"workload": "cfg2 mesh (%d triangles), %dx%d: (a) first-bounce rays, open range; (b) shadow rays, t in (1e-4, 1)" % (len(tris), W, Ht),
           "launches": a.launches, "reps": a.reps,
           "checks": "for every k and every ray: record 0 == lbvh_trace_closest word for word (k = 1: the whole output), found == "
                     "min(k, lbvh_count_hits); rows and found word for word against the brute force on %d rays of each set: hold" % a.check,
           "sets": {}}
    for name, (rays, active) in sets.items():
        closest = lambda: N.lib.lbvh_trace_closest(h, rays.device, n, C.byref(s), rec.device)
        count = lambda: N.lib.lbvh_count_hits(h, rays.device, n, C.byref(s), cnt.device)
        khits = lambda k: (lambda: N.lib.lbvh_trace_k_closest(h, rays.device, n, k, C.byref(s), rows.device, found.device))
        # ---- checks, before any number of this set is kept
        N.check(h, closest())
        N.check(h, count())
        one, counts = rec.get_data().copy(), cnt.get_data().copy()
        act = np.nonzero(rays.local["t_min"] < rays.local["t_max"])[0]
        sub = act[(np.arange(a.check) * (len(act) // max(a.check, 1))).astype(np.int64)]
        ref = K.reference(rays.local[sub], ta, tb, tc, lo, hi, max(ks))
        per_k = {}
        for k in ks:
            rows.fill_u32(0x7FC00000)
            N.check(h, khits(k)())
            got = rows.get_data()[: n * k].reshape(n, k)
            f = found.get_data()
            want = K.truncate(ref, k)
            assert (np.ascontiguousarray(got[sub]).view(np.uint32) == want.records.view(np.uint32)).all(), "rows, set %s, k = %d" % (name, k)
            assert (f[sub] == want.found).all(), "found, set %s, k = %d" % (name, k)
            assert (np.ascontiguousarray(got[:, 0]).view(np.uint32) == one.view(np.uint32)).all(), "record 0 == closest, set %s, k = %d" % (name, k)
            assert (f == np.minimum(counts, k)).all(), "found == min(k, count), set %s, k = %d" % (name, k)
            per_k[k] = {"found_sum": int(f.sum()), "full_rows": int((f == k).sum())}
        out = {"rays_in_buffer": n, "active_rays": active, "candidates_per_active_ray": round(float(counts.sum()) / max(active, 1), 3),
               "most_candidates": int(counts.max()),
               "trace_closest": {**times(closest, active), **work(closest)}, "count_hits": {**times(count, active), **work(count)},
               "k": {}}
        for k in ks:
            lds = STACK_LDS + 3 * k * 64 * 4
            out["k"][str(k)] = {**times(khits(k), active), **work(khits(k)), **per_k[k], "lds_bytes_per_wave": lds,
                                "waves_per_cu_by_lds": min(LDS_PER_CU // lds, 32)}
        tc_, ch = out["trace_closest"], out["count_hits"]
        if "1" in out["k"]:
            k1 = out["k"]["1"]
            out["k1_vs_trace_closest"] = {"ratio": round(k1["ms"] / tc_["ms"], 3),
                                          "ratio_range": [round(k1["ms_min"] / tc_["ms_max"], 3), round(k1["ms_max"] / tc_["ms_min"], 3)]}
        if "32" in out["k"]:
            k32 = out["k"]["32"]
            out["k32_vs_count_hits"] = {"ratio": round(k32["ms"] / ch["ms"], 3),
                                        "ratio_range": [round(k32["ms_min"] / ch["ms_max"], 3), round(k32["ms_max"] / ch["ms_min"], 3)]}
        res["sets"][name] = out
    Q.emit(res, a.out)
    for b in set_buffers + [rows, found, rec, cnt, stats, sets["a"][0], sets["b"][0]]:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
