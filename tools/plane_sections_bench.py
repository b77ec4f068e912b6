#!/usr/bin/env python3
"""lbvh_plane_sections on the cfg2 mesh (1 M triangles) next to the two workarounds it replaces, all timed in the same run.  Prints
one JSON line (profiles/plane_sections/plane_sections.json).

  runs            1 plane through the middle of the mesh, a stack of 64 parallel planes, 4 096 random planes: count only and full
                  (device events), and end to end with the download of the records (wall clock around lbvh_sync)
  workaround_a    the same planes as slab regions {n, d}, {-n, -d}, 4 x {0, 0, 0, 1} through lbvh_region_overlaps_large (count,
                  allocate, fill), the download of the index list, and the triangle-plane narrow phase in numpy on the host: end
                  to end, wall clock, interleaved with this call's end-to-end rounds
  workaround_b    for the single plane: lbvh_triangle_intersection_segments with two query triangles that cover the plane's cut of
                  the scene box (one lane walks each), count only and full, and how many of its records name a triangle that is no
                  candidate of this call, and how many candidates it misses

Before a run is timed its offsets and records are compared with tests/plane_section_reference.py on the first `--check` planes.
Times: device events around `--launches` back-to-back calls, `--reps` times after `--warmup`; per call = median (min / max beside
it).  The wall-clock rounds alternate between the call and workaround (a), `--reps` times each.  There is no pass bar on a time."""
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
    ap = Q.arguments(launches=2, reps=5, warmup=1)
    ap.add_argument("--check", type=int, default=2, help="planes per run compared with the numpy restatement")
    a = ap.parse_args()

    import plane_section_reference as PS
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import host as HO
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    tris = scenes.tiled_torus()
    nt = len(tris)
    va, vb, vc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    ctx = Context(0)
    h, lib = ctx.handle, N.lib
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[:nt]
    lo, hi = box["min"][:, :3].copy(), box["max"][:, :3].copy()
    pts = np.concatenate([lo, hi]).astype(np.float64)
    slo, shi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (slo + shi) * 0.5, float(np.linalg.norm(shi - slo))
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def total_of(buf, count):
        last = np.zeros(1, dtype=np.uint64)
        N.check(h, lib.lbvh_buffer_download(h, last.ctypes.data_as(C.c_void_p), C.c_void_p(buf.device.value + 8 * count), 8))
        return int(last[0])

    def times(call):
        return Q.timed(ctx, call, None, a.launches, a.reps, a.warmup)

    def slab_regions(planes):
        r = np.zeros(len(planes), dtype=L.REGION)
        r["plane"][:, 0, :3], r["plane"][:, 0, 3] = planes["n"], planes["d"]
        r["plane"][:, 1, :3], r["plane"][:, 1, 3] = -planes["n"], -planes["d"]
        r["plane"][:, 2:, 3] = 1.0
        return r

    def host_narrow_phase(planes, off, idx):
        """workaround (a)'s host part: the header's rule 2 and record for every listed (plane, triangle) pair, in numpy"""
        rows = np.repeat(np.arange(len(planes)), np.diff(off).astype(np.int64))
        t = idx.astype(np.int64)
        cand, rec = PS.pair_records(planes[rows], va[t], (vb - va)[t], (vc - va)[t], idx)
        return rec[cand]

    def run(label, planes):
        count = len(planes)
        buf = DataBuffer(ctx, count, L.PLANE)
        buf.local[:] = planes
        buf.sync()
        regions = DataBuffer(ctx, count, L.REGION)
        regions.local[:] = slab_regions(planes)
        regions.sync()
        offsets, offsets2 = DataBuffer(ctx, count + 1, np.uint64), DataBuffer(ctx, count + 1, np.uint64)
        count_only = lambda: lib.lbvh_plane_sections(h, buf.device, count, C.byref(s), offsets.device, None, 0)
        N.check(h, count_only())
        m = total_of(offsets, count)
        seg = DataBuffer(ctx, max(m, 1), L.PLANE_SEGMENT)
        full = lambda: lib.lbvh_plane_sections(h, buf.device, count, C.byref(s), offsets.device, seg.device, m)
        N.check(h, full())
        off, rec = offsets.get_data()[:count + 1].copy(), seg.get_data()[:m].copy()
        ref = PS.reference(planes[:a.check], va, vb, vc, lo, hi)
        last = int(ref.offsets[-1])
        assert (off[:len(ref.offsets)] == ref.offsets).all(), "offsets differ from the restatement"
        assert (PS.record_words(PS.sort_segments(ref.offsets, rec[:last])) == PS.record_words(ref.records)).all(), "records differ"
        c = Q.counters(ctx, stats, count_only)
        row = {"planes": count, "records": m, "task_cap": int(lib.lbvh_debug_region_task_cap_of(0, count)),
               "counters_count_only": {"tasks_not_empty": c.rays, "node_lines": c.node_fetches, "triangle_lines": c.triangle_tests},
               "count_only": times(count_only), "full": times(full)}

        def end_to_end():
            t0 = time.perf_counter()
            N.check(h, count_only())
            total = total_of(offsets, count)
            N.check(h, lib.lbvh_plane_sections(h, buf.device, count, C.byref(s), offsets.device, seg.device, min(total, seg.size)))
            seg.get_data()
            return (time.perf_counter() - t0) * 1e3

        def workaround_a():
            t0 = time.perf_counter()
            o, idx = d.in_regions(regions, L.REGION_TOUCHING, large=True)
            out = host_narrow_phase(planes, o, idx)
            return (time.perf_counter() - t0) * 1e3, len(idx), len(out)

        end_to_end(), workaround_a()
        mine, theirs, listed, kept = [], [], 0, 0
        for _ in range(a.reps):                                          # interleaved rounds
            mine.append(end_to_end())
            ms, listed, kept = workaround_a()
            theirs.append(ms)
        assert kept == m, "the host narrow phase keeps another number of records"
        row["end_to_end_ms"] = Q.summary(mine)
        row["workaround_a"] = {"end_to_end_ms": Q.summary(theirs), "box_candidates_downloaded": listed, "records_kept": kept}
        row["workaround_a_over_this_call"] = round(row["workaround_a"]["end_to_end_ms"]["ms"] / row["end_to_end_ms"]["ms"], 3)
        print(label, row, file=sys.stderr, flush=True)
        for b in (buf, regions, offsets, offsets2, seg):
            b.dispose()
        return row, rec

    rng = np.random.default_rng(41)
    n1 = np.array([[0.3, 0.2, 1.0]])
    one = HO.planes(n1, mid[None])
    levels = np.linspace(slo[2], shi[2], 66)[1:-1]
    stack = HO.planes([0.0, 0.0, 1.0], np.stack([0 * levels + mid[0], 0 * levels + mid[1], levels], axis=1))
    nr = rng.normal(size=(4096, 3))
    many = HO.planes(nr / np.linalg.norm(nr, axis=1, keepdims=True), rng.uniform(slo, shi, (4096, 3)))
    res = {"workload": "lbvh_plane_sections on the cfg2 mesh (%d triangles)" % nt, "launches": a.launches, "reps": a.reps, "runs": {}}
    res["runs"]["one_plane"], one_records = run("one_plane", one)
    res["runs"]["stack_of_64"], _ = run("stack_of_64", stack)
    res["runs"]["random_4096"], _ = run("random_4096", many)

    # workaround (b): two query triangles in the plane that cover its cut of the scene box
    n = n1[0] / np.linalg.norm(n1[0])
    u = np.cross(n, [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    corners = [mid + ext * (su * u + sv * v) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))]
    q = np.zeros(2, dtype=L.TRI_QUERY)
    q["a"], q["b"], q["c"] = [corners[0], corners[0]], [corners[1], corners[2]], [corners[2], corners[3]]
    q["skip"] = L.NULL
    queries = DataBuffer(ctx, 2, L.TRI_QUERY)
    queries.local[:] = q
    queries.sync()
    offsets = DataBuffer(ctx, 3, np.uint64)
    count_b = lambda: lib.lbvh_triangle_intersection_segments(h, queries.device, 2, C.byref(s), offsets.device, None, 0)
    N.check(h, count_b())
    mb = total_of(offsets, 2)
    seg = DataBuffer(ctx, max(mb, 1), L.TRI_SEGMENT)
    full_b = lambda: lib.lbvh_triangle_intersection_segments(h, queries.device, 2, C.byref(s), offsets.device, seg.device, mb)
    N.check(h, full_b())
    theirs, mine = np.unique(seg.get_data()[:mb]["tri"]), np.unique(one_records["tri"])
    res["workaround_b"] = {"records": mb, "count_only": times(count_b), "full": times(full_b),
                           "records_on_triangles_that_are_no_candidates_here": int((~np.isin(seg.get_data()[:mb]["tri"], mine)).sum()),
                           "candidates_here_it_misses": int((~np.isin(mine, theirs)).sum())}
    Q.emit(res, a.out)
    for buf in (queries, offsets, seg, stats):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
