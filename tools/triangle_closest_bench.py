#!/usr/bin/env python3
"""lbvh_triangle_closest_point / lbvh_triangle_within_distance on the cfg2 mesh (1 M triangles) beside the floor and the workaround.
Prints one JSON line.

`--queries` query triangles about points of the surface moved off by up to one size along a random direction, the three vertices
one size from that centre in random directions, with a search radius of one size, at sizes of 0.5 %, 2 % and 10 % of the scene's
extent.  For each size, in the same process on the same queries, in INTERLEAVED rounds (one repetition of each form after the
other, `--reps` rounds: drift of the clock or the device falls on all four alike):
    triangle_closest        lbvh_triangle_closest_point
    triangle_within         lbvh_triangle_within_distance
    three_edges             lbvh_segment_closest_point on the query's three edges with the same max_dist2, three calls: the workaround
    point_closest           lbvh_closest_point_query at the centroids with the same max_dist2: the floor
each with the time per call (three_edges: per three calls), queries per second, node steps and triangle lines per query
(lbvh_ray_stats_target on one more call), and the ratios triangle_closest / point_closest, three_edges / triangle_closest and
triangle_within / triangle_closest.  `workaround_farther` is the share of the queries with a record on which the least dist2 of the
three edges is larger than the record's (none counts as larger): the cases the workaround gets wrong; `edge_nearer_than_triangle` counts the
queries on which an edge's dist2 is below the record's (relation (c): none where the accept rules rejected nothing).

Before a number of a case is kept its outputs are checked: the flag is 1 exactly where the record's dist2 != MAX_FLOAT, and `--check`
queries against tests/triangle_closest_reference.py, every word of the record.
Times: device events around `--launches` back-to-back calls; per call = median over the rounds (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (0.005, 0.02, 0.1)
FORMS = ("triangle_closest", "triangle_within", "three_edges", "point_closest")


def main():
    ap = Q.arguments(launches=2, reps=5, warmup=1)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=16, help="queries of each case compared with the reference")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="of the scene's extent")
    a = ap.parse_args()

    import triangle_closest_reference as T
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = a.queries
    tris = scenes.tiled_torus()
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    pts = np.concatenate([ta, tb, tc])
    extent = float((pts.max(axis=0) - pts.min(axis=0)).max())
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[: len(tris)]
    lo, hi = box["min"].copy(), box["max"].copy()

    rng = np.random.default_rng(1)
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n)
    surface = ta[k] * w[:, :1] + tb[k] * w[:, 1:2] + tc[k] * w[:, 2:]
    off = rng.normal(size=(n, 3))
    off *= (rng.uniform(0.0, 1.0, n) / np.linalg.norm(off, axis=1))[:, None]
    arms = rng.normal(size=(3, n, 3))
    arms /= np.linalg.norm(arms, axis=2, keepdims=True)

    tri, pnt = DataBuffer(ctx, n, L.TRI_DISTANCE_QUERY), DataBuffer(ctx, n, L.POINT_QUERY)
    seg = [DataBuffer(ctx, n, L.SEGMENT_QUERY) for _ in range(3)]
    rec, flg = DataBuffer(ctx, n, L.TRI_CLOSEST), DataBuffer(ctx, n, np.uint32)
    edge = [DataBuffer(ctx, n, L.SEGMENT_CLOSEST) for _ in range(3)]
    near = DataBuffer(ctx, n, L.CLOSEST_POINT)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    lib = N.lib

    def three_edges():
        for m in range(3):
            rc = lib.lbvh_segment_closest_point(h, seg[m].device, n, C.byref(s), edge[m].device)
            if rc != 0:
                return rc
        return 0
    forms = {"triangle_closest": lambda: lib.lbvh_triangle_closest_point(h, tri.device, n, C.byref(s), rec.device),
             "triangle_within": lambda: lib.lbvh_triangle_within_distance(h, tri.device, n, C.byref(s), flg.device),
             "three_edges": three_edges,
             "point_closest": lambda: lib.lbvh_closest_point_query(h, pnt.device, n, C.byref(s), near.device)}

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d query triangles within one size of the surface (vertices one size from "
                       "the centre, search radius one size)" % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps, "rounds": "interleaved",
           "checks": "flag == (dist2 != MAX_FLOAT) on every query; the record word for word against "
                     "the reference on %d queries of each case: hold" % a.check,
           "cases": {}}
    words = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for size in a.sizes:
        sz = size * extent
        r = np.float32(sz)
        centre = surface + off * sz
        q = tri.local
        q["a"], q["b"], q["c"] = centre + arms[0] * sz, centre + arms[1] * sz, centre + arms[2] * sz
        q["skip"], q["max_dist2"] = L.NULL, r * r
        for m, (p, e) in enumerate(((q["a"], q["b"] - q["a"]), (q["b"], q["c"] - q["b"]), (q["c"], q["a"] - q["c"]))):
            seg[m].local["origin"], seg[m].local["axis"], seg[m].local["max_dist2"] = p, e, r * r
        pnt.local["p"], pnt.local["max_dist2"] = (q["a"].astype(np.float64) + q["b"] + q["c"]) / 3.0, r * r
        for b in [tri, pnt] + seg:
            b.sync()
        # ---- checks, before any number of this case is kept
        for name in FORMS:
            N.check(h, forms[name]())
        got, flags = rec.get_data(), flg.get_data()
        least = np.minimum(np.minimum(edge[0].get_data()["dist2"], edge[1].get_data()["dist2"]), edge[2].get_data()["dist2"])
        found = got["dist2"] != L.MAX_FLOAT
        assert (found == (flags == 1)).all(), "flags, %g" % size
        nearer = int((least < got["dist2"]).sum())               # relation (c): none where the accept rules rejected nothing
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = T.reference(tri.local[sub], ta, tb, tc, lo, hi)
        assert (words(got[sub]) == words(ref.records)).all(), "records, %g" % size
        # ---- interleaved rounds
        for _ in range(a.warmup):
            for name in FORMS:
                N.check(h, forms[name]())
        events = (ctx.event(), ctx.event())
        per = {name: [] for name in FORMS}
        for _ in range(a.reps):
            for name in FORMS:
                per[name].append(Q.rep(ctx, events, forms[name], a.launches))
        for e in events:
            ctx.destroy_event(e)
        case = {"size": round(sz, 4), "found": int(found.sum()), "edge_nearer_than_triangle": nearer, "pierced": int((got["edge"][found] & 8 != 0).sum()),
                "won_by_a_scene_edge": int(((got["edge"][found] & 7) >= 3).sum()),
                "workaround_farther": round(float((least[found] > got["dist2"][found]).sum()) / max(int(found.sum()), 1), 4)}
        for name in FORMS:
            steps, tests = Q.per_active(Q.counters(ctx, stats, forms[name]))
            case[name] = {**Q.summary(per[name], n, "Mqueries_s"), "steps_per_query": steps, "triangle_lines_per_query": tests}
        case["triangle_over_point"] = round(case["triangle_closest"]["ms"] / case["point_closest"]["ms"], 2)
        case["edges_over_triangle"] = round(case["three_edges"]["ms"] / case["triangle_closest"]["ms"], 2)
        case["within_over_closest"] = round(case["triangle_within"]["ms"] / case["triangle_closest"]["ms"], 2)
        res["cases"]["size=%g" % size] = case
        print("size=%g: %s" % (size, case), file=sys.stderr, flush=True)
    Q.emit(res, a.out)
    for buf in [tri, pnt, rec, flg, near, stats] + seg + edge:
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
