#!/usr/bin/env python3
"""lbvh_closest_point_query / lbvh_within_distance on the cfg2 mesh (1 M triangles), 2^21 queries.  Prints one JSON line.

  (a) points on the surface (random barycentric combinations of random triangles), unbounded radius: the floor, a walk that
      prunes at once
  (b) points uniform in the scene box, unbounded radius: the distance-field case
  (c) the points of (b) with max_dist2 = --radius^2 (a few triangle edges): closest against within-distance
  (d) lbvh_trace_closest on 2^21 camera rays (a 2048 x 1024 frame from the bench camera), t in (0, +inf): the per-ray walk as
      a yardstick in the same run

Before anything is printed the outputs are checked: `--check` queries of every set against tests/point_reference.py (brute force
over all triangles, word for word: P1 records, P2 flags, zero box-rule rejections), and on every query of every set
within-distance == (closest found a triangle).  Times: device events around `--launches` back-to-back calls, `--reps` times
after `--warmup` calls; per call = median over the reps (min / max beside it: the spread).  Node lines and triangle tests per
active query: lbvh_ray_stats_target on one more call of each.  The CPU restatement's rate comes from the check itself."""
import ctypes as C
import os
import sys
import time

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = Q.arguments(launches=100, reps=5, warmup=10)
    ap.add_argument("--log2-queries", type=int, default=21)
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--check", type=int, default=24, help="queries per set compared with the brute force")
    a = ap.parse_args()

    import point_reference as R
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

    rng = np.random.default_rng(17)
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    surface = (ta[k] * w[:, :1] + tb[k] * w[:, 1:2] + tc[k] * w[:, 2:]).astype(np.float32)
    uniform = rng.uniform(lo.min(axis=0), hi.max(axis=0), (n, 3)).astype(np.float32)

    def query_buffer(p, r2):
        b = DataBuffer(ctx, n, L.POINT_QUERY)
        b.local["p"], b.local["max_dist2"] = p, np.float32(r2)
        b.sync()
        return b

    qa = query_buffer(surface, np.inf)
    qb = query_buffer(uniform, np.inf)
    qc = query_buffer(uniform, a.radius * a.radius)
    # (d): the camera rays of a 2048 x 1024 frame as lbvh_ray records
    W, Ht = 1 << ((a.log2_queries + 1) // 2), 1 << (a.log2_queries // 2)
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))
    states = DataBuffer(ctx, n, L.PATH_STATE)
    N.check(h, N.lib.lbvh_path_begin(h, C.byref(cam), states.device))
    st = states.get_data()
    rays = DataBuffer(ctx, n, L.RAY)
    rays.local["origin"], rays.local["dir"], rays.local["t_min"], rays.local["t_max"] = st["origin"], st["dir"], np.float32(0.0), np.float32(np.inf)
    rays.sync()
    states.dispose()
    out_rec = DataBuffer(ctx, n, L.CLOSEST_POINT)
    out_flags = DataBuffer(ctx, n, np.uint32)
    out_hits = DataBuffer(ctx, n, L.HIT)

    calls = {
        "a_closest_surface": (lambda: N.lib.lbvh_closest_point_query(h, qa.device, n, C.byref(s), out_rec.device), qa, out_rec),
        "b_closest_uniform_unbounded": (lambda: N.lib.lbvh_closest_point_query(h, qb.device, n, C.byref(s), out_rec.device), qb, out_rec),
        "c_closest_uniform_radius": (lambda: N.lib.lbvh_closest_point_query(h, qc.device, n, C.byref(s), out_rec.device), qc, out_rec),
        "c_within_uniform_radius": (lambda: N.lib.lbvh_within_distance(h, qc.device, n, C.byref(s), out_flags.device), qc, out_flags),
        "a_within_surface": (lambda: N.lib.lbvh_within_distance(h, qa.device, n, C.byref(s), out_flags.device), qa, out_flags),
        "d_trace_closest_camera_rays": (lambda: N.lib.lbvh_trace_closest(h, rays.device, n, C.byref(s), out_hits.device), rays, out_hits),
    }

    def run(name):
        fn, _, out = calls[name]
        out.fill_u32(0x7FC00000)
        N.check(h, fn())
        return out.get_data().copy()

    # ---- P1 / P2 on a subset of every set, and within == (closest found) on all of it, before any number is printed
    sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
    cpu_pairs, cpu_s = 0, 0.0
    found = {}
    for cl, wi, qbuf in (("a_closest_surface", "a_within_surface", qa), ("b_closest_uniform_unbounded", None, qb),
                         ("c_closest_uniform_radius", "c_within_uniform_radius", qc)):
        got = run(cl)
        t0 = time.perf_counter()
        ref = R.reference(qbuf.local[sub], ta, tb, tc, lo, hi)
        cpu_s += time.perf_counter() - t0
        cpu_pairs += len(sub) * len(tris)
        assert ref.rejected == 0, "box-rule rejections on " + cl
        assert (got[sub].view(np.uint32) == ref.records.view(np.uint32)).all(), "P1 " + cl
        found[cl] = got["dist2"] < L.MAX_FLOAT
        if wi:
            flags = run(wi)
            assert (flags[sub] == ref.flags).all(), "P2 " + wi
            assert (flags == found[cl]).all(), "within == (closest found) " + wi

    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(name):
        c = Q.counters(ctx, stats, calls[name][0])
        lines, tests = Q.per_active(c)
        return {"active": c.rays, "node_lines": c.node_fetches, "triangle_tests": c.triangle_tests,
                "node_lines_per_query": lines, "triangle_tests_per_query": tests}

    res = {"workload": "point queries on the cfg2 mesh (1 M triangles), 2^%d queries; (d) %dx%d camera rays" % (a.log2_queries, W, Ht),
           "launches": a.launches, "reps": a.reps, "radius": a.radius,
           "checks": "P1 / P2 word for word on %d queries per set, zero box-rule rejections, within == (closest found) on every query: hold" % a.check,
           "cpu_restatement": {"pairs": cpu_pairs, "seconds": round(cpu_s, 2), "Mpairs_s": round(cpu_pairs / cpu_s / 1e6, 2),
                               "queries_s": round(cpu_pairs / len(tris) / cpu_s, 2)},
           "sets": {}}
    for name in calls:
        row = {**Q.timed(ctx, calls[name][0], n, a.launches, a.reps, a.warmup, rate="Mqueries_s"), **work(name)}
        key = name.replace("within", "closest")
        if key in found:
            row["found"] = int(found[key].sum())
        res["sets"][name] = row
    c, w_ = res["sets"]["c_closest_uniform_radius"], res["sets"]["c_within_uniform_radius"]
    res["structural_bar"] = {
        "within_node_lines_le_closest": all(res["sets"][x.replace("closest", "within")]["node_lines"] <= res["sets"][x]["node_lines"]
                                            for x in ("a_closest_surface", "c_closest_uniform_radius")),
        "within_triangle_tests_le_closest": all(res["sets"][x.replace("closest", "within")]["triangle_tests"] <= res["sets"][x]["triangle_tests"]
                                                for x in ("a_closest_surface", "c_closest_uniform_radius")),
        "c_within_ms_minus_closest_ms": round(w_["ms"] - c["ms"], 4),
        "c_spread_ms": round(max(c["ms_max"] - c["ms_min"], w_["ms_max"] - w_["ms_min"]), 4)}
    Q.emit(res, a.out)
    for b in (qa, qb, qc, rays, out_rec, out_flags, out_hits, stats):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
