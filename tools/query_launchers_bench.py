#!/usr/bin/env python3
"""The host path of the query launchers: one entry point of each family that shares a launcher, at a size small
enough that the call is bound by the host — 2^12 queries on the cfg2 mesh (1 M triangles).  Prints one JSON line.

  lbvh_box_overlaps, lbvh_triangle_intersections, lbvh_region_overlaps, lbvh_gather_hits   count walk -> scan -> fill walk
  lbvh_sphere_cast, lbvh_closest_point_query                                                one launch

Queries: boxes of half-width --half around random surface points, the same boxes as regions, triangles with edges of that length
at the same points, and the camera rays of a 64 x 64 frame as rays and as spheres of radius --half.  Every CSR call fills: its
list buffer is sized by a counting call before the clock starts.  Times: device events around `--launches` back-to-back calls,
`--reps` times after `--warmup` calls; per call = median over the reps.  Which library is loaded is LBVH_LIB's business: run it
once per library."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = Q.arguments(launches=100, reps=5, warmup=10)
    ap.add_argument("--log2-queries", type=int, default=12)
    ap.add_argument("--half", type=float, default=0.5)
    a = ap.parse_args()

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer, aabb_planes

    n = 1 << a.log2_queries
    tris = scenes.tiled_torus()
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    rng = np.random.default_rng(32)
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    p = (tris["a"][k, :3] * w[:, :1] + tris["b"][k, :3] * w[:, 1:2] + tris["c"][k, :3] * w[:, 2:]).astype(np.float32)
    half = np.float32(a.half)

    def buffer(dtype, **fields):
        b = DataBuffer(ctx, n, dtype)
        for name, value in fields.items():
            b.local[name] = value
        b.sync()
        return b

    side = 1 << (a.log2_queries // 2)
    cam = N.Camera.from_dict(scenes.camera(side, n // side, (0.0, 0.0, 250.0)))
    states = DataBuffer(ctx, n, L.PATH_STATE)
    N.check(h, N.lib.lbvh_path_begin(h, C.byref(cam), states.device))
    st = states.get_data()
    inf = np.float32(np.inf)
    queries = {
        "boxes": buffer(L.AABB, min=p - half, max=p + half),
        "triangles": buffer(L.TRI_QUERY, a=p, skip=L.NULL, b=p + rng.normal(size=(n, 3)).astype(np.float32) * half,
                            c=p + rng.normal(size=(n, 3)).astype(np.float32) * half),
        "regions": buffer(L.REGION, plane=aabb_planes(p - half, p + half)["plane"]),
        "rays": buffer(L.RAY, origin=st["origin"], dir=st["dir"], t_min=np.float32(0.0), t_max=inf),
        "spheres": buffer(L.SPHERE_RAY, origin=st["origin"], dir=st["dir"], radius=half, t_max=inf),
        "points": buffer(L.POINT_QUERY, p=p, max_dist2=inf),
    }
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    hits = DataBuffer(ctx, n, L.HIT)
    closest = DataBuffer(ctx, n, L.CLOSEST_POINT)
    lib = N.lib
    csr = {
        "lbvh_box_overlaps": (np.uint32, lambda o, c: lib.lbvh_box_overlaps(h, queries["boxes"].device, n, C.byref(s), offsets.device, o, c)),
        "lbvh_triangle_intersections": (np.uint32, lambda o, c: lib.lbvh_triangle_intersections(h, queries["triangles"].device, n, C.byref(s),
                                                                                               offsets.device, o, c)),
        "lbvh_region_overlaps": (np.uint32, lambda o, c: lib.lbvh_region_overlaps(h, queries["regions"].device, n, L.REGION_TOUCHING, C.byref(s),
                                                                                 offsets.device, o, c)),
        "lbvh_gather_hits": (L.HIT, lambda o, c: lib.lbvh_gather_hits(h, queries["rays"].device, n, C.byref(s), offsets.device, o, c)),
    }
    calls, totals, lists = {}, {}, []
    for name, (dtype, fn) in csr.items():
        N.check(h, fn(None, 0))
        totals[name] = int(offsets.get_data()[n])
        assert totals[name] > 0, name
        lst = DataBuffer(ctx, totals[name], dtype)
        lists.append(lst)
        calls[name] = lambda fn=fn, lst=lst: fn(lst.device, lst.size)
    calls["lbvh_sphere_cast"] = lambda: lib.lbvh_sphere_cast(h, queries["spheres"].device, n, C.byref(s), hits.device)
    calls["lbvh_closest_point_query"] = lambda: lib.lbvh_closest_point_query(h, queries["points"].device, n, C.byref(s), closest.device)

    res = {"workload": "2^%d queries per call on the cfg2 mesh (1 M triangles), every CSR call filling" % a.log2_queries,
           "library": os.environ.get("LBVH_LIB") or "the tree's own", "launches": a.launches, "reps": a.reps, "warmup": a.warmup,
           "list_entries": totals, "sets": {name: Q.timed(ctx, fn, None, a.launches, a.reps, a.warmup) for name, fn in calls.items()}}
    Q.emit(res, a.out)
    for b in list(queries.values()) + lists + [states, offsets, hits, closest]:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
