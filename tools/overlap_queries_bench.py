#!/usr/bin/env python3
"""lbvh_box_overlaps / lbvh_gather_within_distance on the cfg2 mesh (1 M triangles).  Prints one JSON line.

  small_boxes   2^21 boxes, centres uniform in the scene box, half-extent --half per axis: tens of candidates where a surface is met
  self          the mesh's own triangle boxes (the device array lbvh_morton_aabb wrote) as queries: the self broad phase
  radius        the uniform points of tools/point_queries_bench.py set (c) with max_dist2 = --radius^2: the line to read next to
                lbvh_within_distance / lbvh_closest_point_query there (both are timed here too, on the same buffer)
  huge_boxes    64 boxes with half-extents of a quarter of the scene: one lane per box emits hundreds of thousands of
                candidates while the rest of the chip idles — the imbalance.  Timed with --huge-launches launches only.

Before anything is printed `--check` queries of every set are compared with tests/overlap_reference.py (brute force over all
triangles, every segment sorted, word for word), and the offsets of the count-only call with those of count + fill.  Times:
device events around `--launches` back-to-back calls, `--reps` times after `--warmup`; per call = median (min / max beside it).
Node lines and triangle tests: lbvh_ray_stats_target on one more call.  The scan's share: the library's per-kernel event
profile (lbvh_profile_begin / _end) of one count + fill call."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = Q.arguments(launches=100, reps=5, warmup=5)
    ap.add_argument("--huge-launches", type=int, default=2)
    ap.add_argument("--log2-queries", type=int, default=21)
    ap.add_argument("--half", type=float, default=1.5)
    ap.add_argument("--radius", type=float, default=3.0)
    ap.add_argument("--check", type=int, default=24, help="queries per set compared with the brute force")
    a = ap.parse_args()

    import overlap_reference as V
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = 1 << a.log2_queries
    tris = scenes.tiled_torus()
    nt = len(tris)
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[:nt]
    lo, hi = box["min"].copy(), box["max"].copy()
    slo, shi = lo.min(axis=0), hi.max(axis=0)

    rng = np.random.default_rng(17)                       # the draws of tools/point_queries_bench.py, so that `uniform` is its set (b) / (c)
    rng.integers(0, nt, n)
    rng.dirichlet((1, 1, 1), n)
    uniform = rng.uniform(slo, shi, (n, 3)).astype(np.float32)

    def upload(arr):
        b = DataBuffer(ctx, len(arr), arr.dtype)
        b.local[:] = arr
        b.sync()
        return b

    half = np.float32(a.half)
    small = upload(V.make_boxes(uniform - half, uniform + half))
    points = DataBuffer(ctx, n, L.POINT_QUERY)
    points.local["p"], points.local["max_dist2"] = uniform, np.float32(a.radius * a.radius)
    points.sync()
    hrng = np.random.default_rng(18)
    hc = hrng.uniform(slo, shi, (64, 3)).astype(np.float32)
    hh = (0.25 * (shi - slo)).astype(np.float32)
    huge = upload(V.make_boxes(hc - hh, hc + hh))

    sets = {  # name: (function, device pointer of the queries, count, host copy of the queries or None, launches)
        "small_boxes": (N.lib.lbvh_box_overlaps, small.device, n, small.local, a.launches),
        "self": (N.lib.lbvh_box_overlaps, d.container.triangle_aabb.device, nt, V.make_boxes(lo, hi), a.launches),
        "radius": (N.lib.lbvh_gather_within_distance, points.device, n, points.local, a.launches),
        "huge_boxes": (N.lib.lbvh_box_overlaps, huge.device, 64, huge.local, a.huge_launches),
    }
    offsets = DataBuffer(ctx, max(n, nt) + 1, np.uint64)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def total_of(count):
        last = np.zeros(1, dtype=np.uint64)
        N.check(h, N.lib.lbvh_buffer_download(h, last.ctypes.data_as(C.c_void_p), C.c_void_p(offsets.device.value + 8 * count), 8))
        return int(last[0])

    def times(call, launches):                              # no more warm-up calls than launches: the huge boxes
        return Q.timed(ctx, call, None, launches, a.reps, min(a.warmup, launches))

    res = {"workload": "overlap queries on the cfg2 mesh (%d triangles), 2^%d queries (self: one per triangle; huge_boxes: 64)" % (nt, a.log2_queries),
           "launches": a.launches, "huge_launches": a.huge_launches, "reps": a.reps, "half": a.half, "radius": a.radius, "sets": {}}
    for name, (fn, dq, count, host, launches) in sets.items():
        count_only = lambda: fn(h, dq, count, C.byref(s), offsets.device, None, 0)
        N.check(h, count_only())
        m = total_of(count)
        off0 = offsets.get_data()[:count + 1].copy()
        lst = DataBuffer(ctx, max(m, 1), np.uint32)
        fill = lambda: fn(h, dq, count, C.byref(s), offsets.device, lst.device, m)
        N.check(h, fill())
        off = offsets.get_data()[:count + 1].copy()
        got = lst.get_data()
        assert (off == off0).all() and int(off[-1]) == m, "count-only offsets " + name
        # parity on a sample, before any number is printed
        sub = (np.arange(a.check) * (count // max(a.check, 1))).astype(np.int64)
        if fn is N.lib.lbvh_box_overlaps:
            ro, rt = V.box_overlaps(host[sub], lo, hi)
        else:
            ro, rt = V.gather_within_distance(host[sub], ta, tb, tc, lo, hi)
        for j, k in enumerate(sub):
            seg = np.sort(got[int(off[k]):int(off[k + 1])])
            assert (seg == rt[int(ro[j]):int(ro[j + 1])]).all() and len(seg) == int(ro[j + 1] - ro[j]), (name, int(k))
        row = {"queries": count, "M": m, "candidates_per_query": round(m / count, 3), "longest_segment": int(np.diff(off).max()),
               "count_only": times(count_only, launches), "count_and_fill": times(fill, launches)}
        active, lines, tests = Q.counters(ctx, stats, count_only)
        active2, lines2, _ = Q.counters(ctx, stats, fill)
        row.update({"active": active, "node_lines_per_query": round(lines / max(active, 1), 3), "triangle_tests_per_query": round(tests / max(active, 1), 3),
                    "node_lines_count_only": lines, "node_lines_count_and_fill": lines2,
                    "Mcandidates_written_per_s": round(m / (row["count_and_fill"]["ms"] * 1e-3) / 1e6, 1)})
        ctx.profile_begin()
        N.check(h, fill())
        prof = ctx.profile_end()
        scan = sum(ms for k, (_, ms) in prof.items() if "sums" in k or "offsets" in k)
        row["kernel_ms_one_call"] = {k.split("<")[0].strip("( "): round(ms, 4) for k, (_, ms) in prof.items()}
        row["scan_share"] = round(scan / max(sum(ms for _, ms in prof.values()), 1e-9), 4)
        res["sets"][name] = row
        lst.dispose()
    # lbvh_within_distance / lbvh_closest_point_query on the radius set, the same buffer
    flags, rec = DataBuffer(ctx, n, np.uint32), DataBuffer(ctx, n, L.CLOSEST_POINT)
    within = lambda: N.lib.lbvh_within_distance(h, points.device, n, C.byref(s), flags.device)
    closest = lambda: N.lib.lbvh_closest_point_query(h, points.device, n, C.byref(s), rec.device)
    _, w_lines, _ = Q.counters(ctx, stats, within)
    res["radius_yardsticks"] = {"within_distance": {**times(within, a.launches), "node_lines": w_lines},
                                "closest_point_query": {**times(closest, a.launches), "node_lines": Q.counters(ctx, stats, closest)[1]}}
    res["conditions"] = {
        "count_only_never_slower_than_count_and_fill": all(r["count_only"]["ms"] <= r["count_and_fill"]["ms"] for r in res["sets"].values()),
        "distance_count_walk_fetches_no_fewer_lines_than_within_distance": res["sets"]["radius"]["node_lines_count_only"] >= w_lines,
        "fill_walk_repeats_the_count_walk": all(r["node_lines_count_and_fill"] == 2 * r["node_lines_count_only"] for r in res["sets"].values())}
    Q.emit(res, a.out)
    for b in (small, points, huge, offsets, stats, flags, rec):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
