#!/usr/bin/env python3
"""lbvh_region_overlaps_large next to lbvh_region_overlaps on the cfg2 mesh (1 M triangles), both timed in the same run.  Prints one
JSON line (profiles/region_large/region_large.json).

  one_large_frustum   the frustum of tools/region_queries_bench.py that holds about half the mesh, alone: both calls, count only and
                      full, the counters of the large form, and the large form under forced task caps (lbvh_debug_region_task_cap)
  table               counts 1, 16, 256, 4 096, 65 536 of turned boxes holding about 50 %, 5 % and 0.05 % of the mesh: both calls, count
                      only and full, and old / new.  A cell whose lists would exceed --max-candidates words is skipped and says so.
  slot_budget         256 regions of about 5 % under 1 024, 4 096 and 16 384 tasks per region: what slot budgets of 2^18, 2^20 and 2^22
                      would give them

Before a cell is timed the two calls' offsets are compared word for word and their lists after lbvh_sort_index_segments; the first
regions of every size also with tests/region_reference.py.  Times: device events around `--launches` back-to-back calls, `--reps` times
after `--warmup`; per call = median (min / max beside it)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q
from region_queries_bench import look_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = Q.arguments(launches=2, reps=3, warmup=1)
    ap.add_argument("--max-candidates", type=int, default=1 << 28, help="cells with longer lists are skipped")
    ap.add_argument("--check", type=int, default=2, help="regions per size compared with the brute force")
    a = ap.parse_args()

    import region_reference as R
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import host as HO
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    tris = scenes.tiled_torus()
    nt = len(tris)
    ctx = Context(0)
    h, lib = ctx.handle, N.lib
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    box = d.container.triangle_aabb.get_data()[:nt]
    lo, hi = box["min"][:, :3].copy(), box["max"][:, :3].copy()
    pts = np.concatenate([lo, hi]).astype(np.float64)
    slo, shi = pts.min(axis=0), pts.max(axis=0)
    mid, ext = (slo + shi) * 0.5, float(np.linalg.norm(shi - slo))
    n_max = 65536
    regions = DataBuffer(ctx, n_max, L.REGION)
    offsets = DataBuffer(ctx, n_max + 1, np.uint64)
    offsets2 = DataBuffer(ctx, n_max + 1, np.uint64)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    old_fn, new_fn = lib.lbvh_region_overlaps, lib.lbvh_region_overlaps_large

    def total_of(buf, count):
        last = np.zeros(1, dtype=np.uint64)
        N.check(h, lib.lbvh_buffer_download(h, last.ctypes.data_as(C.c_void_p), C.c_void_p(buf.device.value + 8 * count), 8))
        return int(last[0])

    def times(call):
        return Q.timed(ctx, call, None, a.launches, a.reps, a.warmup)

    def cell(count, check_with=None):
        """both calls on the first `count` regions of the buffer: checked against each other, then timed"""
        count_old = lambda: old_fn(h, regions.device, count, L.REGION_TOUCHING, C.byref(s), offsets.device, None, 0)
        count_new = lambda: new_fn(h, regions.device, count, L.REGION_TOUCHING, C.byref(s), offsets2.device, None, 0)
        N.check(h, count_new())
        m = total_of(offsets2, count)
        row = {"M": m, "share_of_the_mesh_per_region": round(m / count / nt, 5),
               "task_cap": int(lib.lbvh_debug_region_task_cap_of(0, count))}
        if m > a.max_candidates:
            row["skipped"] = "lists of %d words exceed --max-candidates" % m
            return row
        N.check(h, count_old())
        assert (offsets.get_data()[:count + 1] == offsets2.get_data()[:count + 1]).all(), "offsets differ"
        lst, lst2 = DataBuffer(ctx, max(m, 1), np.uint32), DataBuffer(ctx, max(m, 1), np.uint32)
        full_old = lambda: old_fn(h, regions.device, count, L.REGION_TOUCHING, C.byref(s), offsets.device, lst.device, m)
        full_new = lambda: new_fn(h, regions.device, count, L.REGION_TOUCHING, C.byref(s), offsets2.device, lst2.device, m)
        N.check(h, full_old())
        N.check(h, full_new())
        HO.sort_index_segments(ctx, offsets, lst, count)
        HO.sort_index_segments(ctx, offsets2, lst2, count)
        got_old, got_new = lst.get_data()[:m], lst2.get_data()[:m]
        assert (got_old == got_new).all(), "sorted lists differ"
        if check_with is not None:
            ro, rt = R.reference(check_with[:count], lo, hi)[R.TOUCHING]
            assert (offsets2.get_data()[:len(ro)] == ro).all() and (got_new[:len(rt)] == rt).all(), "brute force"
        row["count_only"] = {"region_overlaps": times(count_old), "region_overlaps_large": times(count_new)}
        row["full"] = {"region_overlaps": times(full_old), "region_overlaps_large": times(full_new)}
        for form in ("count_only", "full"):
            row[form]["old_over_new"] = round(row[form]["region_overlaps"]["ms"] / row[form]["region_overlaps_large"]["ms"], 3)
        lst.dispose()
        lst2.dispose()
        print(count, row, file=sys.stderr, flush=True)
        return row

    res = {"workload": "lbvh_region_overlaps_large and lbvh_region_overlaps on the cfg2 mesh (%d triangles), TOUCHING" % nt,
           "launches": a.launches, "reps": a.reps}

    # (a) the priced caveat of DESIGN.md §29: the left half of a view that holds the whole mesh
    eye = mid + np.array([0.0, 0.0, 1.0]) * ext
    camera = {"screen_width": 64, "screen_height": 64, "camera_fov": 1.0, "near_plane": 0.01 * ext,
              "camera_to_world": look_at(eye[None], mid[None])[0].astype(np.float32)}
    big = HO.frustum_planes(camera, far=2.0 * ext, rect=(0, 0, 32, 64))
    regions.local[:1] = big
    regions.sync()
    one = cell(1, check_with=big)
    count_new = lambda: new_fn(h, regions.device, 1, L.REGION_TOUCHING, C.byref(s), offsets2.device, None, 0)
    c = Q.counters(ctx, stats, count_new)
    one["counters_count_only"] = {"tasks_not_empty": c.rays, "node_lines": c.node_fetches, "leaf_slots": c.triangle_tests,
                                  "node_lines_per_task": round(c.node_fetches / max(c.rays, 1), 3)}
    one["forced_task_caps_count_only"] = {}
    for cap in (64, 1024, 4096, 16384, 65536):
        N.check(h, lib.lbvh_debug_region_task_cap(h, cap))
        one["forced_task_caps_count_only"][str(cap)] = times(count_new)
    N.check(h, lib.lbvh_debug_region_task_cap(h, 0))
    res["one_large_frustum"] = one

    # (b) turned boxes of three sizes
    rng = np.random.default_rng(41)
    axis = rng.normal(size=(n_max, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = rng.uniform(0.0, 0.5, n_max)
    kx = np.zeros((n_max, 3, 3))
    kx[:, 0, 1], kx[:, 0, 2], kx[:, 1, 0], kx[:, 1, 2], kx[:, 2, 0], kx[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    rot = np.eye(3) + np.sin(angle)[:, None, None] * kx + (1.0 - np.cos(angle))[:, None, None] * (kx @ kx)
    res["table"] = {}
    sets = {}
    for share in (0.5, 0.05, 0.0005):
        half = 0.5 * (shi - slo) * share ** (1.0 / 3.0)
        centre = rng.uniform(slo + 0.8 * half, shi - 0.8 * half, (n_max, 3))
        sets[share] = HO.obb_planes(centre, rot, np.broadcast_to(half, (n_max, 3)))
        regions.local[:] = sets[share]
        regions.sync()
        res["table"]["%g %%" % (100.0 * share)] = {str(count): cell(count, check_with=sets[share][:a.check]) for count in (1, 16, 256, 4096, 65536)}

    # (c) what a smaller slot budget would give 256 regions of 5 %
    regions.local[:] = sets[0.05]
    regions.sync()
    res["slot_budget"] = {}
    for log2_budget, cap in ((18, 1024), (20, 4096), (22, 16384)):
        N.check(h, lib.lbvh_debug_region_task_cap(h, cap))
        row = cell(256)
        res["slot_budget"]["2^%d" % log2_budget] = {"task_cap": cap, "count_only": row["count_only"]["region_overlaps_large"],
                                                    "full": row["full"]["region_overlaps_large"]}
    N.check(h, lib.lbvh_debug_region_task_cap(h, 0))
    Q.emit(res, a.out)
    for buf in (regions, offsets, offsets2, stats):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
