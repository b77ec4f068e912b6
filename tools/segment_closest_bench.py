#!/usr/bin/env python3
"""lbvh_segment_closest_point / lbvh_segment_within_distance on the cfg2 mesh (1 M triangles) beside the floor and the workaround.
Prints one JSON line.

`--queries` segments drawn as tools/shape_contacts_bench.py draws its capsules — at points of the surface moved off by up to one
size along a random direction, an axis of two sizes in a random direction — with a search radius of one size, at sizes of 0.5 %,
2 % and 10 % of the scene's extent.  For each size, in the same process on the same segments, in INTERLEAVED rounds (one
repetition of each form after the other, `--reps` rounds: drift of the clock or the device falls on all four alike):
    segment_closest         lbvh_segment_closest_point
    segment_within          lbvh_segment_within_distance
    point_closest           lbvh_closest_point_query at the origins with the same max_dist2: the floor, a walk that grows no box
    capsule_deepest         lbvh_capsule_deepest with radius^2 = max_dist2: the workaround, an overlap walk that prunes nothing
each with the time per call, queries per second, node steps and triangle lines per query (lbvh_ray_stats_target on one more call),
and the ratios segment_closest / point_closest and capsule_deepest / segment_closest.

Before a number of a case is kept its outputs are checked: the flag is 1 exactly where the record's dist2 != MAX_FLOAT, and
`--check` queries against tests/segment_closest_reference.py, every word of the record.
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
FORMS = ("segment_closest", "segment_within", "point_closest", "capsule_deepest")


def main():
    ap = Q.arguments(launches=3, reps=5, warmup=1)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=16, help="queries of each case compared with the reference")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="of the scene's extent")
    a = ap.parse_args()

    import segment_closest_reference as G
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

    rng = np.random.default_rng(1)                                   # the draws of tools/shape_contacts_bench.py, in its order
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n)
    surface = ta[k] * w[:, :1] + tb[k] * w[:, 1:2] + tc[k] * w[:, 2:]
    off = rng.normal(size=(n, 3))
    off *= (rng.uniform(0.0, 1.0, n) / np.linalg.norm(off, axis=1))[:, None]
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)

    seg, pnt, cap = DataBuffer(ctx, n, L.SEGMENT_QUERY), DataBuffer(ctx, n, L.POINT_QUERY), DataBuffer(ctx, n, L.CAPSULE)
    rec, flg = DataBuffer(ctx, n, L.SEGMENT_CLOSEST), DataBuffer(ctx, n, np.uint32)
    near, deep = DataBuffer(ctx, n, L.CLOSEST_POINT), DataBuffer(ctx, n, L.CONTACT)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    lib = N.lib
    forms = {"segment_closest": lambda: lib.lbvh_segment_closest_point(h, seg.device, n, C.byref(s), rec.device),
             "segment_within": lambda: lib.lbvh_segment_within_distance(h, seg.device, n, C.byref(s), flg.device),
             "point_closest": lambda: lib.lbvh_closest_point_query(h, pnt.device, n, C.byref(s), near.device),
             "capsule_deepest": lambda: lib.lbvh_capsule_deepest(h, cap.device, n, C.byref(s), deep.device)}

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d segments within one size of the surface (axis 2 sizes, search radius one size)"
                       % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps, "rounds": "interleaved",
           "checks": "flag == (dist2 != MAX_FLOAT) on every query; the record word for word against the reference on %d queries of each "
                     "case: hold" % a.check,
           "cases": {}}
    words = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for size in a.sizes:
        sz = size * extent
        r = np.float32(sz)
        seg.local["origin"], seg.local["axis"], seg.local["max_dist2"] = surface + off * sz - axis * sz, axis * (2.0 * sz), r * r
        pnt.local["p"], pnt.local["max_dist2"] = seg.local["origin"], r * r
        cap.local["origin"], cap.local["axis"], cap.local["radius"] = seg.local["origin"], seg.local["axis"], r
        for b in (seg, pnt, cap):
            b.sync()
        # ---- checks, before any number of this case is kept
        for name in FORMS:
            N.check(h, forms[name]())
        got, flags = rec.get_data(), flg.get_data()
        assert ((got["dist2"] != L.MAX_FLOAT) == (flags == 1)).all(), "flags, %g" % size
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = G.reference(seg.local[sub], ta, tb, tc, lo, hi)
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
        case = {"size": round(sz, 4), "found": int(flags.sum())}
        for name in FORMS:
            steps, tests = Q.per_active(Q.counters(ctx, stats, forms[name]))
            case[name] = {**Q.summary(per[name], n, "Mqueries_s"), "steps_per_query": steps, "triangle_lines_per_query": tests}
        case["segment_over_point"] = round(case["segment_closest"]["ms"] / case["point_closest"]["ms"], 2)
        case["deepest_over_segment"] = round(case["capsule_deepest"]["ms"] / case["segment_closest"]["ms"], 2)
        case["within_over_closest"] = round(case["segment_within"]["ms"] / case["segment_closest"]["ms"], 2)
        res["cases"]["size=%g" % size] = case
    Q.emit(res, a.out)
    for buf in (seg, pnt, cap, rec, flg, near, deep, stats):
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
