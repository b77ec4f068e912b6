#!/usr/bin/env python3
"""lbvh_triangle_cast_all on the cfg2 mesh (1 M triangles) against lbvh_triangle_cast (the floor: it prunes) and against the
workaround a caller had before it, lbvh_triangle_intersections sampled at 8 positions along the move.  Prints one JSON line.

`--casts` triangles start on a sphere around the scene's box and aim at points inside it (the origins and directions of
tools/cast_all_bench.py), moved to `--start` of their way so that the move of length t_max = `--move` (of the scene's extent, unit
directions) lies inside the scene; the edges b - a and c - a have random directions and 0.5 %, 2 % and 10 % of the extent.  For each
size, in interleaved rounds (every variant once per round, `--reps` rounds after `--warmup`):
    count_only      lbvh_triangle_cast_all with capacity 0: one walk
    full            the call with the records (capacity = the total, at most `--max-records`; beyond it the fill walk still makes
                    every decision and only skips the store)
    full_sorted     full, then lbvh_sort_hit_segments
    first_contact   lbvh_triangle_cast on the same casts
    sampled_8       lbvh_triangle_intersections, count-only form, with the triangle at t = k * t_max / 7, k = 0 .. 7: eight calls
with the mean and the longest segment, count_over_first (the price of not pruning), full_over_count, and, on the first
`--miss-sample` casts, the share of the cast-all contacts that none of the eight sampled intersection lists holds.

Before anything is printed the outputs are checked on `--check` casts of each size against tests/triangle_cast_all_reference.py
(brute force over all triangles, word for word after the canonical sort)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (0.005, 0.02, 0.1)
SAMPLES = 8


def main():
    ap = Q.arguments(launches=1, reps=5, warmup=1)
    ap.add_argument("--casts", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=4, help="casts of each size compared with the brute force")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="edge lengths, of the scene's extent")
    ap.add_argument("--move", type=float, default=0.1, help="t_max, of the scene's extent")
    ap.add_argument("--start", type=float, default=0.45, help="where on its way from outside the move starts")
    ap.add_argument("--max-records", type=int, default=1 << 27)
    ap.add_argument("--miss-sample", type=int, default=4096)
    a = ap.parse_args()

    import triangle_cast_all_reference as TA
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer, sort_hit_segments

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
    reach = 0.75 * np.linalg.norm(hi_s - lo_s) + 0.2 * extent
    centre = target - direction * reach * (1.0 - a.start)
    direction = direction.astype(np.float32)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    e1, e2 = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
    t_max = np.float32(a.move * extent)

    casts = DataBuffer(ctx, n, L.TRI_RAY)
    first_out = DataBuffer(ctx, n, L.TRI_CAST_HIT)
    stills = [DataBuffer(ctx, n, L.TRI_QUERY) for _ in range(SAMPLES)]
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    sample_offsets = DataBuffer(ctx, n + 1, np.uint64)
    events = (ctx.event(), ctx.event())

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d moves of %.3g x extent inside the scene, unit directions" % (len(tris), extent, n, a.move),
           "launches": a.launches, "reps": a.reps,
           "checks": "records word for word against the brute force after the canonical sort on %d casts of each size: hold" % a.check,
           "cases": {}}
    for size in a.sizes:
        edge = size * extent
        qa = centre - (e1 + e2) * (edge / 3.0)
        c = casts.local
        c["a"], c["b"], c["c"] = qa.astype(np.float32), (qa + e1 * edge).astype(np.float32), (qa + e2 * edge).astype(np.float32)
        c["dir"], c["t_max"], c["skip"] = direction, t_max, L.NULL
        casts.sync()
        for k, still in enumerate(stills):                             # the triangle where it stands at t = k * t_max / 7
            step = direction * np.float32(k * float(t_max) / (SAMPLES - 1))
            q = still.local
            q["a"], q["b"], q["c"], q["skip"] = c["a"] + step, c["b"] + step, c["c"] + step, L.NULL
            still.sync()
        count_only = lambda: N.lib.lbvh_triangle_cast_all(h, casts.device, n, C.byref(s), offsets.device, None, 0)
        N.check(h, count_only())
        m = np.diff(offsets.get_data().astype(np.int64))
        total = int(m.sum())
        capacity = max(min(total, a.max_records), 1)
        records = DataBuffer(ctx, capacity, L.TRI_CAST_HIT)
        full = lambda: N.lib.lbvh_triangle_cast_all(h, casts.device, n, C.byref(s), offsets.device, records.device, capacity)

        def full_sorted():
            rc = full()
            sort_hit_segments(ctx, offsets, records, n)
            return rc

        first = lambda: N.lib.lbvh_triangle_cast(h, casts.device, n, C.byref(s), first_out.device)

        def sampled():
            for still in stills:
                rc = N.lib.lbvh_triangle_intersections(h, still.device, n, C.byref(s), sample_offsets.device, None, 0)
                if rc != 0:
                    return rc
            return 0

        # ---- checks, before any number of this size is kept
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        small = DataBuffer(ctx, len(sub), L.TRI_RAY)
        small.local[:] = casts.local[sub]
        small.sync()
        off, rec = d.cast_all(small, sort=True)
        ref = TA.reference(small.local, ta, tb, tc, lo, hi, casts_per_chunk=1)
        assert (off == ref.offsets).all() and (np.ascontiguousarray(rec).view(np.uint32) == ref.records.view(np.uint32)).all(), size
        small.dispose()
        # ---- what the sampled intersection lists miss, on the first casts
        k = min(a.miss_sample, n)
        head = DataBuffer(ctx, k, L.TRI_RAY)
        head.local[:] = casts.local[:k]
        head.sync()
        off, rec = d.cast_all(head)
        head.dispose()
        seen = set()
        for still in stills:
            part = DataBuffer(ctx, k, L.TRI_QUERY)
            part.local[:] = still.local[:k]
            part.sync()
            o2, t2 = d.intersections(part)
            seen.update((np.repeat(np.arange(k), np.diff(o2.astype(np.int64))).astype(np.int64) << 32 | t2.astype(np.int64)).tolist())
            part.dispose()
        pairs = np.repeat(np.arange(k), np.diff(off.astype(np.int64))).astype(np.int64) << 32 | rec["tri"].astype(np.int64)
        missed = sum(1 for p in pairs.tolist() if p not in seen)
        # ---- interleaved rounds
        variants = {"count_only": count_only, "full": full, "full_sorted": full_sorted, "first_contact": first, "sampled_8": sampled}
        for _ in range(a.warmup):
            for fn in variants.values():
                N.check(h, fn())
        per = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, fn in variants.items():
                per[name].append(Q.rep(ctx, events, fn, a.launches))
        case = {name: Q.summary(per[name], n, rate="Mcasts_s") for name in variants}
        case.update({"edge": round(float(edge), 4), "t_max": round(float(t_max), 4), "records": total, "capacity": capacity,
                     "mean_segment": round(total / n, 2), "longest_segment": int(m.max()), "empty_share": round(float((m == 0).mean()), 4),
                     "count_over_first": round(case["count_only"]["ms"] / case["first_contact"]["ms"], 2),
                     "full_over_count": round(case["full"]["ms"] / case["count_only"]["ms"], 2),
                     "sorted_over_full": round(case["full_sorted"]["ms"] / case["full"]["ms"], 2),
                     "sampled_over_full": round(case["sampled_8"]["ms"] / case["full"]["ms"], 2),
                     "sampled_misses_share": round(missed / max(len(pairs), 1), 4), "miss_sample_contacts": len(pairs)})
        res["cases"]["triangle size=%g" % size] = case
        print("triangle size=%g: done" % size, file=sys.stderr, flush=True)
        records.dispose()
    Q.emit(res, a.out)
    for e in events:
        ctx.destroy_event(e)
    for b in [casts, first_out, offsets, sample_offsets] + stills:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
