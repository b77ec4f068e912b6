#!/usr/bin/env python3
"""lbvh_capsule_overlaps / lbvh_obb_overlaps on the cfg2 mesh (1 M triangles) against what a caller had before them.  Prints one
JSON line.

`--shapes` shapes stand at points of the surface moved off by up to one size along a random direction: capsules with an axis of two
sizes in a random direction and a radius of half a size, and cubes of half extent one size turned at random, at sizes of 0.5 %, 2 %
and 10 % of the scene's extent.  For each size and shape kind, in the same process on the same shapes:
    count_only, full, any   the new calls in their three forms (full: into a buffer of the counted total, or of --max-list words
                            if that is less: the walk is the same, the words beyond are not written)
    box_overlaps            lbvh_box_overlaps (count-only) on the shapes' own AABBs: the broad-phase floor, and `broad_over_exact`,
                            the factor by which its candidate list is longer
    cast_any                lbvh_capsule_cast_any / lbvh_box_cast_any with an invented dir and t_max = 1e-6: the workaround
each with the time per call, shapes per second, node steps and triangle lines per shape (lbvh_ray_stats_target on one more call).

Before a number of a case is kept its outputs are checked: `--check` shapes against tests/shape_overlap_reference.py (brute force
over all triangles, each segment sorted), the offsets of the full form equal the count-only form's, and the flags of the any form
equal `segment non-empty` on every shape.
Times: device events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls; per call = median over the
reps (min / max beside it: the spread)."""
import ctypes as C
import os
import sys

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (0.005, 0.02, 0.1)


def main():
    ap = Q.arguments(launches=3, reps=5, warmup=1)
    ap.add_argument("--shapes", type=int, default=1 << 20)
    ap.add_argument("--check", type=int, default=16, help="shapes of each case compared with the brute force")
    ap.add_argument("--sizes", type=float, nargs="+", default=list(SIZES), help="of the scene's extent")
    ap.add_argument("--max-list", type=int, default=1 << 30, help="the most words the full form is given")
    a = ap.parse_args()

    import shape_overlap_reference as S
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    n = a.shapes
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
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    turn = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]               # columns: the cube's axes

    bufs = {"capsule": DataBuffer(ctx, n, L.CAPSULE), "obb": DataBuffer(ctx, n, L.OBB)}
    casts = {"capsule": DataBuffer(ctx, n, L.CAPSULE_RAY), "obb": DataBuffer(ctx, n, L.BOX_RAY)}
    aabbs = DataBuffer(ctx, n, L.AABB)
    offsets, offsets2 = DataBuffer(ctx, n + 1, np.uint64), DataBuffer(ctx, n + 1, np.uint64)
    flg, flg2 = DataBuffer(ctx, n, np.uint32), DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    calls = {"capsule": (N.lib.lbvh_capsule_overlaps, N.lib.lbvh_capsule_overlaps_any, N.lib.lbvh_capsule_cast_any),
             "obb": (N.lib.lbvh_obb_overlaps, N.lib.lbvh_obb_overlaps_any, N.lib.lbvh_box_cast_any)}

    def measure(fn):
        steps, tests = Q.per_active(Q.counters(ctx, stats, fn))
        return {**Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mshapes_s"), "steps_per_shape": steps, "triangle_lines_per_shape": tests}

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d shapes within one size of the surface: capsules (axis 2 sizes, radius "
                       "half a size) and cubes (half extent one size) turned at random" % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps,
           "checks": "full form's offsets == count-only form's; any form's flags == segment non-empty on every shape; sorted segments "
                     "word for word against the brute force on %d shapes of each case: hold" % a.check,
           "cases": {}}
    for size in a.sizes:
        sz = size * extent
        centre = surface + off * sz
        for kind in ("capsule", "obb"):
            b, c = bufs[kind], casts[kind]
            if kind == "capsule":
                b.local["origin"], b.local["axis"], b.local["radius"] = centre - axis * sz, axis * (2.0 * sz), np.float32(0.5 * sz)
                blo = np.minimum(b.local["origin"], b.local["origin"] + b.local["axis"]) - b.local["radius"][:, None]
                bhi = np.maximum(b.local["origin"], b.local["origin"] + b.local["axis"]) + b.local["radius"][:, None]
            else:
                axes = (turn * sz).astype(np.float32)
                b.local["centre"], b.local["ax"], b.local["ay"], b.local["az"] = centre, axes[:, :, 0], axes[:, :, 1], axes[:, :, 2]
                g = np.abs(axes).sum(axis=2)
                blo, bhi = b.local["centre"] - g, b.local["centre"] + g
            b.sync()
            for f in b.dtype.names:
                if not f.startswith("_pad"):
                    c.local[f] = b.local[f]
            c.local["dir"], c.local["t_max"] = (0.5, -1.0, 2.0), np.float32(1e-6)
            c.sync()
            aabbs.local["min"][:, :3], aabbs.local["max"][:, :3] = blo, bhi
            aabbs.sync()
            lists, flags, cast_any = calls[kind]
            count_only = lambda: lists(h, b.device, n, C.byref(s), offsets.device, None, 0)
            # ---- checks, before any number of this case is kept
            N.check(h, count_only())
            off_count = offsets.get_data().copy()
            total = int(off_count[n])
            cap = max(min(total, a.max_list), 1)
            out = DataBuffer(ctx, cap, np.uint32)
            full = lambda: lists(h, b.device, n, C.byref(s), offsets2.device, out.device, cap)
            any_form = lambda: flags(h, b.device, n, C.byref(s), flg.device)
            N.check(h, full())
            N.check(h, any_form())
            assert (offsets2.get_data() == off_count).all(), "offsets, %s %g" % (kind, size)
            assert (flg.get_data() == (np.diff(off_count) > 0)).all(), "flags, %s %g" % (kind, size)
            got = out.get_data()
            sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
            ref = S.reference(b.local[sub], ta, tb, tc, lo, hi)
            for j, q in enumerate(sub):
                first, last = int(off_count[q]), int(off_count[q + 1])
                want = ref.tris[int(ref.offsets[j]):int(ref.offsets[j + 1])]
                assert last - first == len(want), "count of shape %d, %s %g" % (q, kind, size)
                if last <= cap:
                    assert (np.sort(got[first:last]) == want).all(), "segment of shape %d, %s %g" % (q, kind, size)
            case = {"size": round(sz, 4), "total": total, "non_empty": int((np.diff(off_count) > 0).sum()), "capacity": cap,
                    "count_only": measure(count_only), "full": measure(full), "any": measure(any_form)}
            N.check(h, N.lib.lbvh_box_overlaps(h, aabbs.device, n, C.byref(s), offsets2.device, None, 0))
            broad = int(offsets2.get_data()[n])
            case["box_overlaps"] = {**measure(lambda: N.lib.lbvh_box_overlaps(h, aabbs.device, n, C.byref(s), offsets2.device, None, 0)), "total": broad}
            case["broad_over_exact"] = round(broad / max(total, 1), 2)
            case["cast_any"] = measure(lambda: cast_any(h, c.device, n, C.byref(s), flg2.device))
            case["cast_any"]["flagged"] = int(flg2.get_data().sum())
            case["count_over_box_overlaps"] = round(case["count_only"]["ms"] / case["box_overlaps"]["ms"], 2)
            case["any_over_cast_any"] = round(case["any"]["ms"] / case["cast_any"]["ms"], 2)
            res["cases"]["%s, size=%g" % (kind, size)] = case
            out.dispose()
    Q.emit(res, a.out)
    for b in list(bufs.values()) + list(casts.values()) + [aabbs, offsets, offsets2, flg, flg2, stats]:
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
