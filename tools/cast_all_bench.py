#!/usr/bin/env python3
"""lbvh_sphere_cast_all / lbvh_capsule_cast_all / lbvh_box_cast_all on the cfg2 mesh (1 M triangles) against the first-contact cast
(the floor: it prunes) and against the workaround a caller had before them, the shape's overlap list sampled at 8 positions along
the move.  Prints one JSON line.

`--casts` shapes start on a sphere around the scene's box and aim at points inside it (the origins and directions of
tools/sphere_cast_bench.py, capsule_cast_bench.py and box_cast_bench.py), moved to `--start` of their way so that the move of
length t_max = `--move` (of the scene's extent, unit directions) lies inside the scene: spheres of radius, capsules of radius (axis
4 radii, random direction) and cubes of half extent 0.5 %, 2 % and 10 % of the extent.  For each shape and size, in interleaved
rounds (every variant once per round, `--reps` rounds after `--warmup`):
    count_only      the cast-all call with capacity 0: one walk
    full            the cast-all call with the records (capacity = the total, at most `--max-records`; beyond it the fill walk still
                    makes every decision and only skips the store)
    full_sorted     full, then lbvh_sort_hit_segments
    first_contact   lbvh_*_cast on the same casts
    sampled_8       lbvh_gather_within_distance / lbvh_capsule_overlaps / lbvh_obb_overlaps, count-only form, at t = k * t_max / 7,
                    k = 0 .. 7: eight calls
with the mean and the longest segment, count_over_first (the price of not pruning), full_over_count, and, on the first
`--miss-sample` casts, the share of the cast-all contacts that none of the eight sampled overlap lists holds.

Before anything is printed the outputs are checked on `--check` casts of each case against tests/cast_all_reference.py (brute force
over all triangles, word for word after the canonical sort)."""
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
    ap.add_argument("--check", type=int, default=4, help="casts of each case compared with the brute force")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="radii / half extents, of the scene's extent")
    ap.add_argument("--shapes", nargs="+", default=["sphere", "capsule", "box"])
    ap.add_argument("--move", type=float, default=0.1, help="t_max, of the scene's extent")
    ap.add_argument("--start", type=float, default=0.45, help="where on its way from outside the move starts")
    ap.add_argument("--max-records", type=int, default=1 << 27)
    ap.add_argument("--miss-sample", type=int, default=4096)
    a = ap.parse_args()

    import cast_all_reference as CA
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
    origin = (target - direction * reach * (1.0 - a.start)).astype(np.float32)
    direction = direction.astype(np.float32)
    turn = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]               # columns: the cube's axes
    axis_dir = rng.normal(size=(n, 3))
    axis_dir /= np.linalg.norm(axis_dir, axis=1, keepdims=True)
    t_max = np.float32(a.move * extent)

    layout = {"sphere": (L.SPHERE_RAY, L.HIT, L.POINT_QUERY), "capsule": (L.CAPSULE_RAY, L.HIT, L.CAPSULE), "box": (L.BOX_RAY, L.BOX_HIT, L.OBB)}
    entry = {"sphere": (N.lib.lbvh_sphere_cast_all, N.lib.lbvh_sphere_cast, N.lib.lbvh_gather_within_distance),
             "capsule": (N.lib.lbvh_capsule_cast_all, N.lib.lbvh_capsule_cast, N.lib.lbvh_capsule_overlaps),
             "box": (N.lib.lbvh_box_cast_all, N.lib.lbvh_box_cast, N.lib.lbvh_obb_overlaps)}
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    sample_offsets = DataBuffer(ctx, n + 1, np.uint64)
    events = (ctx.event(), ctx.event())

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d moves of %.3g x extent inside the scene, unit directions" % (len(tris), extent, n, a.move),
           "launches": a.launches, "reps": a.reps,
           "checks": "records word for word against the brute force after the canonical sort on %d casts of each case: hold" % a.check,
           "cases": {}}
    for shape in a.shapes:
        ray_t, hit_t, still_t = layout[shape]
        all_fn, first_fn, overlap_fn = entry[shape]
        casts = DataBuffer(ctx, n, ray_t)
        first_out = DataBuffer(ctx, n, hit_t)
        stills = [DataBuffer(ctx, n, still_t) for _ in range(SAMPLES)]
        for size in a.sizes:
            r = np.float32(size * extent)
            c = casts.local
            c["centre" if shape == "box" else "origin"], c["dir"], c["t_max"] = origin, direction, t_max
            if shape == "box":
                axes = (turn * r).astype(np.float32)
                c["ax"], c["ay"], c["az"] = axes[:, :, 0], axes[:, :, 1], axes[:, :, 2]
            else:
                c["radius"] = r
            if shape == "capsule":
                c["axis"] = (axis_dir * (4.0 * r)).astype(np.float32)
            casts.sync()
            for k, still in enumerate(stills):                         # the shape where it stands at t = k * t_max / 7
                at = (origin + direction * np.float32(k * float(t_max) / (SAMPLES - 1))).astype(np.float32)
                q = still.local
                if shape == "sphere":
                    q["p"], q["max_dist2"] = at, r * r
                elif shape == "capsule":
                    q["origin"], q["radius"], q["axis"] = at, r, c["axis"]
                else:
                    q["centre"], q["ax"], q["ay"], q["az"] = at, c["ax"], c["ay"], c["az"]
                still.sync()
            count_only = lambda: all_fn(h, casts.device, n, C.byref(s), offsets.device, None, 0)
            N.check(h, count_only())
            m = np.diff(offsets.get_data().astype(np.int64))
            total = int(m.sum())
            capacity = max(min(total, a.max_records), 1)
            records = DataBuffer(ctx, capacity, hit_t)
            full = lambda: all_fn(h, casts.device, n, C.byref(s), offsets.device, records.device, capacity)

            def full_sorted():
                rc = full()
                sort_hit_segments(ctx, offsets, records, n)
                return rc

            first = lambda: first_fn(h, casts.device, n, C.byref(s), first_out.device)

            def sampled():
                for still in stills:
                    rc = overlap_fn(h, still.device, n, C.byref(s), sample_offsets.device, None, 0)
                    if rc != 0:
                        return rc
                return 0

            # ---- checks, before any number of this case is kept
            sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
            small = DataBuffer(ctx, len(sub), ray_t)
            small.local[:] = casts.local[sub]
            small.sync()
            off, rec = d.cast_all(small, sort=True)
            ref = CA.reference(small.local, ta, tb, tc, lo, hi, casts_per_chunk=1)
            assert (off == ref.offsets).all() and (np.ascontiguousarray(rec).view(np.uint32) == ref.records.view(np.uint32)).all(), (shape, size)
            small.dispose()
            # ---- what the sampled overlaps miss, on the first casts
            k = min(a.miss_sample, n)
            head = DataBuffer(ctx, k, ray_t)
            head.local[:] = casts.local[:k]
            head.sync()
            off, rec = d.cast_all(head)
            seen = set()
            for still in stills:
                part = DataBuffer(ctx, k, still_t)
                part.local[:] = still.local[:k]
                part.sync()
                o2, t2 = d.overlaps(part) if shape == "sphere" else d.touching(part)
                seen.update((np.repeat(np.arange(k), np.diff(o2.astype(np.int64))).astype(np.int64) << 32 | t2.astype(np.int64)).tolist())
                part.dispose()
            head.dispose()
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
            case.update({"size": round(float(r), 4), "t_max": round(float(t_max), 4), "records": total, "capacity": capacity,
                         "mean_segment": round(total / n, 2), "longest_segment": int(m.max()), "empty_share": round(float((m == 0).mean()), 4),
                         "count_over_first": round(case["count_only"]["ms"] / case["first_contact"]["ms"], 2),
                         "full_over_count": round(case["full"]["ms"] / case["count_only"]["ms"], 2),
                         "sorted_over_full": round(case["full_sorted"]["ms"] / case["full"]["ms"], 2),
                         "sampled_over_full": round(case["sampled_8"]["ms"] / case["full"]["ms"], 2),
                         "sampled_misses_share": round(missed / max(len(pairs), 1), 4), "miss_sample_contacts": len(pairs)})
            res["cases"]["%s size=%g" % (shape, size)] = case
            print("%s size=%g: done" % (shape, size), file=sys.stderr, flush=True)
            records.dispose()
        for b in [casts, first_out] + stills:
            b.dispose()
    Q.emit(res, a.out)
    for e in events:
        ctx.destroy_event(e)
    offsets.dispose()
    sample_offsets.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
