#!/usr/bin/env python3
"""lbvh_k_closest_points on the cfg2 mesh (1 M triangles), 2^20 surface-near queries, unbounded radius.  Prints one JSON line.

Queries: random barycentric combinations of random triangles, moved by a normal-distributed offset of --offset units per axis
(a fraction of a triangle edge): registration / distance-field samples near the surface.  For k in --ks: time per call, queries
per second, node lines and triangle tests per query (lbvh_ray_stats_target on one more call), LDS per block and the waves per CU
that leaves.  In the same process, on the same buffer:
  * lbvh_closest_point_query, the yardstick for k = 1;
  * lbvh_gather_within_distance (count walk + scan + fill walk) with the radius at which the median segment holds 8 triangles
    (found by bisection on count-only calls): the route k = 8 replaces; the host-side sort and selection it still needs is
    not counted.

Before anything is printed the outputs are checked: `--check` queries against tests/k_closest_reference.py for every k (brute
force over all triangles, word for word, zero box-rule rejections), k = 1 against lbvh_closest_point_query on every query, and
record 0 of every row of every k against it.  Times: device events around `--launches` back-to-back calls, `--reps` times after
`--warmup` calls (the clocks settle there); per call = median over the reps (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LDS_PER_CU = 160 * 1024          # gfx950
STACK_LDS = 16 * 64 * 4          # the walk's 16-entry stack


def main():
    ap = Q.arguments(launches=20, reps=5, warmup=5)
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--offset", type=float, default=0.05)
    ap.add_argument("--ks", default="1,4,8,16,32")
    ap.add_argument("--check", type=int, default=16, help="queries compared with the brute force")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]

    import k_closest_reference as K
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = 1 << a.log2_queries
    tris = scenes.tiled_torus()
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[: len(tris)]
    lo, hi = box["min"].copy(), box["max"].copy()

    rng = np.random.default_rng(23)
    t = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    pts = (ta[t] * w[:, :1] + tb[t] * w[:, 1:2] + tc[t] * w[:, 2:] + rng.normal(0.0, a.offset, (n, 3))).astype(np.float32)
    q = DataBuffer(ctx, n, L.POINT_QUERY)
    q.local["p"], q.local["max_dist2"] = pts, np.float32(np.inf)
    q.sync()
    rows = DataBuffer(ctx, n * max(ks), L.CLOSEST_POINT)
    found = DataBuffer(ctx, n, np.uint32)
    rec = DataBuffer(ctx, n, L.CLOSEST_POINT)

    closest = lambda: N.lib.lbvh_closest_point_query(h, q.device, n, C.byref(s), rec.device)
    knn = lambda k: (lambda: N.lib.lbvh_k_closest_points(h, q.device, n, k, C.byref(s), rows.device, found.device))

    # ---- checks, before any number is printed
    N.check(h, closest())
    one = rec.get_data().copy()
    sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
    ref = K.reference(q.local[sub], ta, tb, tc, lo, hi, max(ks))
    assert ref.rejected == 0, "box-rule rejections"
    for k in ks:
        rows.fill_u32(0x7FC00000)
        N.check(h, knn(k)())
        got = rows.get_data()[: n * k].reshape(n, k)
        want = K.truncate(ref, k)
        assert (np.ascontiguousarray(got[sub]).view(np.uint32) == want.records.view(np.uint32)).all(), "rows, k = %d" % k
        assert (found.get_data()[sub] == want.found).all(), "found, k = %d" % k
        assert (np.ascontiguousarray(got[:, 0]).view(np.uint32) == one.view(np.uint32)).all(), "record 0 == closest point, k = %d" % k

    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(fn):
        lines, tests = Q.per_active(Q.counters(ctx, stats, fn))
        return {"node_lines_per_query": lines, "triangle_tests_per_query": tests}

    def times(fn):
        return Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mqueries_s", digits=2)

    # ---- the gather route: the radius whose median segment length is 8
    offsets = DataBuffer(ctx, n + 1, np.uint64)

    def median_len(r2):
        q.local["max_dist2"] = np.float32(r2)
        q.sync()
        N.check(h, N.lib.lbvh_gather_within_distance(h, q.device, n, C.byref(s), offsets.device, None, 0))
        off = offsets.get_data()
        return float(np.median(np.diff(off.astype(np.int64)))), int(off[n])

    r_lo, r_hi = 0.0, 64.0
    for _ in range(18):
        mid = 0.5 * (r_lo + r_hi)
        if median_len(mid)[0] < 8:
            r_lo = mid
        else:
            r_hi = mid
    med, total = median_len(r_hi)
    seg = DataBuffer(ctx, max(total, 1), np.uint32)
    gather = lambda: N.lib.lbvh_gather_within_distance(h, q.device, n, C.byref(s), offsets.device, seg.device, seg.size)
    res_gather = {**times(gather), **work(gather), "max_dist2": round(r_hi, 5), "median_segment": med, "total_triangles": total,
                  "note": "count walk + scan + fill walk; the host-side sort and cut at 8 is not counted"}
    q.local["max_dist2"] = np.float32(np.inf)
    q.sync()

    res = {"workload": "cfg2 mesh (%d triangles), 2^%d surface-near queries (offset sigma %.3g), unbounded radius" % (len(tris), a.log2_queries, a.offset),
           "launches": a.launches, "reps": a.reps,
           "checks": "rows and found word for word against the brute force on %d queries for every k, record 0 of every row == "
                     "lbvh_closest_point_query on every query for every k, zero box-rule rejections: hold" % a.check,
           "closest_point_query": {**times(closest), **work(closest)}, "k": {}, "gather_within_distance_median_8": res_gather}
    for k in ks:
        lds = STACK_LDS + 3 * k * 64 * 4
        res["k"][str(k)] = {**times(knn(k)), **work(knn(k)), "lds_bytes_per_wave": lds, "waves_per_cu_by_lds": min(LDS_PER_CU // lds, 32)}
    cp = res["closest_point_query"]
    if "1" in res["k"]:
        k1 = res["k"]["1"]
        res["k1_vs_closest_point_query"] = {"ms_difference": round(k1["ms"] - cp["ms"], 4),
                                            "spread_ms": round(max(k1["ms_max"] - k1["ms_min"], cp["ms_max"] - cp["ms_min"]), 4),
                                            "ratio": round(k1["ms"] / cp["ms"], 3)}
    if "8" in res["k"]:
        res["k8_vs_gather"] = {"ratio": round(res["k"]["8"]["ms"] / res_gather["ms"], 3)}
    Q.emit(res, a.out)
    for b in (q, rows, found, rec, stats, offsets, seg):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
