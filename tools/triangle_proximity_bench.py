#!/usr/bin/env python3
"""lbvh_triangle_gather_within_distance on the cfg2 mesh (1 M triangles) beside the pruned walk and the workaround.  Prints one JSON
line.

`--queries` query triangles about points of the surface moved off by up to one size along a random direction, the three vertices
one size from that centre in random directions, with a margin (search radius) of one size, at sizes of 0.5 %, 2 % and 10 % of the
scene's extent: the queries of tools/triangle_closest_bench.py.  For each size, in the same process on the same queries, in
INTERLEAVED rounds (one repetition of each form after the other, `--reps` rounds: drift of the clock or the device falls on all
alike):
    gather_count            lbvh_triangle_gather_within_distance, capacity 0: one walk and the scan
    gather_full             the same with records: two walks; the expectation to confirm or refute is about twice gather_count
    triangle_closest        lbvh_triangle_closest_point on the same queries: the pruned walk, the floor
    triangle_within         lbvh_triangle_within_distance
    padded_boxes            the workaround's device part alone: lbvh_box_overlaps (full form) on the query boxes padded by the margin;
                            its host narrow phase, 54 point tests per listed pair, is not measured
each with the time per call, queries per second, node steps and triangle lines per query (lbvh_ray_stats_target on one more call),
and full_over_count, full_over_closest, `records` and `records_per_query` of the gather, `box_list_over_gather` = how many times
longer the padded boxes' list is.  `--max-records` bounds the record buffers (the total is read from the count-only form first):
a case whose lists do not fit is measured with the capacity it has — both walks still run in full, the stores beyond the capacity
are not made — and says so in `truncated`.

Before a number of a case is kept its outputs are checked: count-only and full offsets are equal, a segment is non-empty exactly
where the flag is 1, and `--check` queries against tests/triangle_proximity_reference.py, every word of every record.
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
FORMS = ("gather_count", "gather_full", "triangle_closest", "triangle_within", "padded_boxes")


def main():
    ap = Q.arguments(launches=1, reps=5, warmup=1)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=16, help="queries of each case compared with the reference")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="of the scene's extent")
    ap.add_argument("--max-records", type=int, default=1 << 28, help="upper bound of each record buffer")
    a = ap.parse_args()

    import triangle_proximity_reference as X
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

    tri, boxes = DataBuffer(ctx, n, L.TRI_DISTANCE_QUERY), DataBuffer(ctx, n, L.AABB)
    off_count, off_full, off_box = (DataBuffer(ctx, n + 1, np.uint64) for _ in range(3))
    rec, flg = DataBuffer(ctx, n, L.TRI_CLOSEST), DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    lib = N.lib

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d query triangles within one size of the surface (vertices one size from "
                       "the centre, margin one size)" % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps, "rounds": "interleaved",
           "checks": "count-only offsets == full offsets; non-empty == flag; every record word for word against the reference on %d "
                     "queries of each case: hold" % a.check,
           "cases": {}}
    words = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for size in a.sizes:
        sz = size * extent
        r = np.float32(sz)
        centre = surface + off * sz
        q = tri.local
        q["a"], q["b"], q["c"] = centre + arms[0] * sz, centre + arms[1] * sz, centre + arms[2] * sz
        q["skip"], q["max_dist2"] = L.NULL, r * r
        boxes.local["min"] = np.minimum(np.minimum(q["a"], q["b"]), q["c"]) - r
        boxes.local["max"] = np.maximum(np.maximum(q["a"], q["b"]), q["c"]) + r
        tri.sync()
        boxes.sync()
        # ---- the sizes of the two lists, from the count-only forms
        N.check(h, lib.lbvh_triangle_gather_within_distance(h, tri.device, n, C.byref(s), off_count.device, None, 0))
        N.check(h, lib.lbvh_box_overlaps(h, boxes.device, n, C.byref(s), off_box.device, None, 0))
        counted = off_count.get_data()[: n + 1].copy()
        total, box_total = int(counted[n]), int(off_box.get_data()[n])
        cap, box_cap = min(max(total, 1), a.max_records), min(max(box_total, 1), a.max_records)
        records, listed = DataBuffer(ctx, cap, L.TRI_CLOSEST), DataBuffer(ctx, box_cap, np.uint32)
        forms = {"gather_count": lambda: lib.lbvh_triangle_gather_within_distance(h, tri.device, n, C.byref(s), off_count.device, None, 0),
                 "gather_full": lambda: lib.lbvh_triangle_gather_within_distance(h, tri.device, n, C.byref(s), off_full.device, records.device, cap),
                 "triangle_closest": lambda: lib.lbvh_triangle_closest_point(h, tri.device, n, C.byref(s), rec.device),
                 "triangle_within": lambda: lib.lbvh_triangle_within_distance(h, tri.device, n, C.byref(s), flg.device),
                 "padded_boxes": lambda: lib.lbvh_box_overlaps(h, boxes.device, n, C.byref(s), off_box.device, listed.device, box_cap)}
        # ---- checks, before any number of this case is kept
        for name in FORMS:
            N.check(h, forms[name]())
        filled = off_full.get_data()[: n + 1].copy()
        assert (filled == counted).all(), "offsets, %g" % size
        assert ((np.diff(counted) > 0) == (flg.get_data()[:n] == 1)).all(), "flags, %g" % size
        got = records.get_data()
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        sub = sub[counted[sub + 1] <= cap]                         # (segments that fit are complete)
        ref = X.reference(tri.local[sub], ta, tb, tc, lo, hi)
        for j, at in enumerate(sub):
            seg = got[int(counted[at]):int(counted[at + 1])]
            want = ref.records[int(ref.offsets[j]):int(ref.offsets[j + 1])]
            assert len(seg) == len(want) and (words(seg[np.argsort(seg["tri"])]) == words(want)).all(), "records, %g, query %d" % (size, at)
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
        case = {"size": round(sz, 4), "records": total, "records_per_query": round(total / n, 2), "nonempty": int((np.diff(counted) > 0).sum()),
                "longest": int(np.diff(counted).max()), "box_list": box_total, "box_list_over_gather": round(box_total / max(total, 1), 2),
                "truncated": bool(total > cap or box_total > box_cap)}
        for name in FORMS:
            steps, tests = Q.per_active(Q.counters(ctx, stats, forms[name]))
            case[name] = {**Q.summary(per[name], n, "Mqueries_s"), "steps_per_query": steps, "triangle_lines_per_query": tests}
        case["full_over_count"] = round(case["gather_full"]["ms"] / case["gather_count"]["ms"], 2)
        case["full_over_closest"] = round(case["gather_full"]["ms"] / case["triangle_closest"]["ms"], 2)
        case["count_over_within"] = round(case["gather_count"]["ms"] / case["triangle_within"]["ms"], 2)
        case["boxes_over_full"] = round(case["padded_boxes"]["ms"] / case["gather_full"]["ms"], 2)
        res["cases"]["size=%g" % size] = case
        print("size=%g: %s" % (size, case), file=sys.stderr, flush=True)
        records.dispose()
        listed.dispose()
    Q.emit(res, a.out)
    for buf in (tri, boxes, off_count, off_full, off_box, rec, flg, stats):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
