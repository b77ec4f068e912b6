#!/usr/bin/env python3
"""lbvh_triangle_intersections / lbvh_triangle_intersects_any on the cfg2 mesh (1 M triangles), next to the broad phase they extend.
Prints one JSON line.

Queries: 2^20 scene triangles (seeded picks) turned about their centroid by a seeded angle about a seeded axis and scaled by
--scales (default 0.5, 1, 2: three query sizes relative to the scene's own triangles).  Per scale:
  count_only      lbvh_triangle_intersections with capacity 0
  full            count, device-side scan, fill
  any             lbvh_triangle_intersects_any
  box_overlaps    lbvh_box_overlaps (count only and full) on the exact boxes of the same query triangles: the broad phase
  ratio           the three triangle forms' time over the broad phase's of the same form (any: over the count-only broad phase)

Before anything is printed `--check` queries of every scale are compared with tests/triangle_query_reference.py (every segment
sorted, word for word; the flags), and the offsets of the count-only call with those of count + fill.  Times: device events around
`--launches` back-to-back calls, `--reps` times after `--warmup`; per call = median (min / max beside it).  Node lines and triangle
tests: lbvh_ray_stats_target on one more call."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def turned_triangles(ta, tb, tc, count, scale, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(ta), count)
    v = np.stack([ta[k], tb[k], tc[k]], axis=1).astype(np.float64)
    centre = v.mean(axis=1, keepdims=True)
    axis = rng.normal(size=(count, 3))
    axis = (axis / np.linalg.norm(axis, axis=1, keepdims=True))[:, None, :]
    angle = rng.uniform(0.0, 2.0 * np.pi, count)
    co, si = np.cos(angle)[:, None, None], np.sin(angle)[:, None, None]
    r = v - centre
    out = centre + (r * co + np.cross(axis, r) * si + axis * (axis * r).sum(axis=2, keepdims=True) * (1.0 - co)) * scale
    return tuple(out[:, j].astype(np.float32) for j in range(3))


def main():
    ap = Q.arguments(launches=20, reps=5, warmup=3)
    ap.add_argument("--log2-queries", type=int, default=20)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.5, 1.0, 2.0])
    ap.add_argument("--check", type=int, default=24, help="queries per scale compared with the brute force")
    a = ap.parse_args()

    import overlap_reference as V
    import triangle_query_reference as T
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = 1 << a.log2_queries
    tris = scenes.tiled_torus()
    nt = len(tris)
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    ctx = Context(0)
    h, lib = ctx.handle, N.lib
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[:nt]
    lo, hi = box["min"].copy(), box["max"].copy()
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    flags = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    queries = DataBuffer(ctx, n, L.TRI_QUERY)
    boxes = DataBuffer(ctx, n, L.AABB)

    def total_of():
        last = np.zeros(1, dtype=np.uint64)
        N.check(h, lib.lbvh_buffer_download(h, last.ctypes.data_as(C.c_void_p), C.c_void_p(offsets.device.value + 8 * n), 8))
        return int(last[0])

    def times(call):
        return Q.timed(ctx, call, None, a.launches, a.reps, a.warmup)

    res = {"workload": "triangle queries on the cfg2 mesh (%d triangles), 2^%d queries per scale" % (nt, a.log2_queries),
           "launches": a.launches, "reps": a.reps, "scales": {}}
    for scale in a.scales:
        qa, qb, qc = turned_triangles(ta, tb, tc, n, scale, 29)
        queries.local[:] = T.make_queries(qa, qb, qc)
        queries.sync()
        pts = np.stack([qa, qb, qc], axis=1)
        boxes.local[:] = V.make_boxes(pts.min(axis=1), pts.max(axis=1))
        boxes.sync()
        row = {}
        for name, fn, dq in (("triangles", lib.lbvh_triangle_intersections, queries.device), ("box_overlaps", lib.lbvh_box_overlaps, boxes.device)):
            count_only = lambda: fn(h, dq, n, C.byref(s), offsets.device, None, 0)
            N.check(h, count_only())
            m = total_of()
            off0 = offsets.get_data().copy()
            lst = DataBuffer(ctx, max(m, 1), np.uint32)
            fill = lambda: fn(h, dq, n, C.byref(s), offsets.device, lst.device, m)
            N.check(h, fill())
            off = offsets.get_data().copy()
            assert (off == off0).all() and int(off[-1]) == m, "count-only offsets " + name
            if name == "triangles":                                  # parity on a sample, before any number is printed
                got = lst.get_data()
                N.check(h, lib.lbvh_triangle_intersects_any(h, dq, n, C.byref(s), flags.device))
                fl = flags.get_data()
                sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
                ref = T.reference(queries.local[sub], ta, tb, tc, lo, hi)
                for j, k in enumerate(sub):
                    seg = np.sort(got[int(off[k]):int(off[k + 1])])
                    assert len(seg) == int(ref.offsets[j + 1] - ref.offsets[j]) and (seg == ref.tris[int(ref.offsets[j]):int(ref.offsets[j + 1])]).all(), int(k)
                    assert int(fl[k]) == int(ref.flags[j]), int(k)
                assert ((np.diff(off) > 0) == (fl == 1)).all()
            c = Q.counters(ctx, stats, count_only)
            lines, tests = Q.per_active(c)
            row[name] = {"M": m, "candidates_per_query": round(m / n, 3), "longest_segment": int(np.diff(off).max()),
                         "count_only": times(count_only), "full": times(fill), "node_lines_per_query": lines, "triangle_tests_per_query": tests}
            lst.dispose()
        any_call = lambda: lib.lbvh_triangle_intersects_any(h, queries.device, n, C.byref(s), flags.device)
        c = Q.counters(ctx, stats, any_call)
        lines, tests = Q.per_active(c)
        row["triangles"]["any"] = {**times(any_call), "node_lines_per_query": lines, "triangle_tests_per_query": tests}
        t, b = row["triangles"], row["box_overlaps"]
        row["ratio_to_broad_phase"] = {"count_only": round(t["count_only"]["ms"] / b["count_only"]["ms"], 3),
                                       "full": round(t["full"]["ms"] / b["full"]["ms"], 3),
                                       "any_over_count_only_broad_phase": round(t["any"]["ms"] / b["count_only"]["ms"], 3)}
        res["scales"]["%g" % scale] = row
    Q.emit(res, a.out)
    for buf in (offsets, flags, stats, queries, boxes):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
