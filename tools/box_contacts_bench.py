#!/usr/bin/env python3
"""lbvh_obb_contacts / lbvh_obb_deepest on the cfg2 mesh (1 M triangles) beside lbvh_obb_overlaps on the same shapes.
Prints one JSON line.

`--shapes` cubes drawn as tools/shape_overlaps_bench.py draws them — at points of the surface moved off by up to one size along a
random direction, a half extent of one size, turned at random — at sizes of 0.5 %, 2 % and 10 % of the scene's extent.  For each
size, in the same process on the same shapes:
    contacts_full, contacts_count_only, deepest      the new calls
    overlaps_full, overlaps_count_only               lbvh_obb_overlaps in its two list forms
each with the time per call, shapes per second, node steps and triangle lines per shape (lbvh_ray_stats_target on one more call),
and the ratios full / overlaps' full, deepest / overlaps' count-only, contacts' count-only / overlaps' count-only.  The last two
are the same kernel; they are measured once more in interleaved rounds with the order swapped from round to round
(count_only_interleaved: the ratio of the medians beside the larger relative spread, max - min over the median).  The full forms write into a buffer of the counted total, or of --max-list records if that is less: the walk is
the same, the records beyond are not written.

Before a number of a case is kept its outputs are checked: the offsets of all four list calls are equal, `--check` shapes against
tests/box_contact_reference.py (brute force over all triangles, each segment sorted by tri, every word of every record, and the deepest
record), and deepest.tri != NULL exactly where the segment is non-empty.
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
    ap.add_argument("--max-list", type=int, default=1 << 27, help="the most records the full forms are given")
    a = ap.parse_args()

    import box_contact_reference as K
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

    rng = np.random.default_rng(1)                                   # the draws of tools/shape_overlaps_bench.py, in its order
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n)
    surface = ta[k] * w[:, :1] + tb[k] * w[:, 1:2] + tc[k] * w[:, 2:]
    off = rng.normal(size=(n, 3))
    off *= (rng.uniform(0.0, 1.0, n) / np.linalg.norm(off, axis=1))[:, None]
    axis = rng.normal(size=(n, 3))                                   # (the capsules' axes: drawn to keep the order)
    turn = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]               # columns: the cube's axes

    b = DataBuffer(ctx, n, L.OBB)
    offs = [DataBuffer(ctx, n + 1, np.uint64) for _ in range(4)]
    deep = DataBuffer(ctx, n, L.BOX_CONTACT)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)
    lib = N.lib

    def measure(fn):
        steps, tests = Q.per_active(Q.counters(ctx, stats, fn))
        return {**Q.timed(ctx, fn, n, a.launches, a.reps, a.warmup, rate="Mshapes_s"), "steps_per_shape": steps, "triangle_lines_per_shape": tests}

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g), %d cubes within one size of the surface (half extent one size) turned at random"
                       % (len(tris), extent, n),
           "launches": a.launches, "reps": a.reps,
           "checks": "the four list calls' offsets are equal; deepest.tri != NULL == segment non-empty on every shape; sorted segments and "
                     "the deepest record word for word against the brute force on %d shapes of each case: hold" % a.check,
           "cases": {}}
    for size in a.sizes:
        sz = size * extent
        centre = surface + off * sz
        axes = (turn * sz).astype(np.float32)
        b.local["centre"], b.local["ax"], b.local["ay"], b.local["az"] = centre, axes[:, :, 0], axes[:, :, 1], axes[:, :, 2]
        b.sync()
        forms = {"contacts_count_only": lambda: lib.lbvh_obb_contacts(h, b.device, n, C.byref(s), offs[0].device, None, 0),
                 "overlaps_count_only": lambda: lib.lbvh_obb_overlaps(h, b.device, n, C.byref(s), offs[1].device, None, 0)}
        # ---- checks, before any number of this case is kept
        N.check(h, forms["contacts_count_only"]())
        off_count = offs[0].get_data().copy()
        total = int(off_count[n])
        cap = max(min(total, a.max_list), 1)
        recs, idx = DataBuffer(ctx, cap, L.BOX_CONTACT), DataBuffer(ctx, cap, np.uint32)
        forms["contacts_full"] = lambda: lib.lbvh_obb_contacts(h, b.device, n, C.byref(s), offs[2].device, recs.device, cap)
        forms["overlaps_full"] = lambda: lib.lbvh_obb_overlaps(h, b.device, n, C.byref(s), offs[3].device, idx.device, cap)
        forms["deepest"] = lambda: lib.lbvh_obb_deepest(h, b.device, n, C.byref(s), deep.device)
        for name in ("overlaps_count_only", "contacts_full", "overlaps_full", "deepest"):
            N.check(h, forms[name]())
        for o in offs[1:]:
            assert (o.get_data() == off_count).all(), "offsets, %g" % size
        got, best = recs.get_data(), deep.get_data()
        assert ((best["tri"] != L.NULL) == (np.diff(off_count) > 0)).all(), "deepest against the segments, %g" % size
        sub = (np.arange(a.check) * (n // max(a.check, 1))).astype(np.int64)
        ref = K.reference(b.local[sub], ta, tb, tc, lo, hi)
        words = lambda x: np.ascontiguousarray(x).view(np.uint32)
        for j, q in enumerate(sub):
            first, last = int(off_count[q]), int(off_count[q + 1])
            want = ref.contacts[int(ref.offsets[j]):int(ref.offsets[j + 1])]
            assert last - first == len(want), "count of shape %d, %g" % (q, size)
            assert (words(best[q:q + 1]) == words(ref.deepest[j:j + 1])).all(), "deepest of shape %d, %g" % (q, size)
            if last <= cap:
                seg = got[first:last]
                assert (words(seg[np.argsort(seg["tri"])]) == words(want)).all(), "segment of shape %d, %g" % (q, size)
        case = {"size": round(sz, 4), "total": total, "non_empty": int((np.diff(off_count) > 0).sum()), "capacity": cap}
        for name in ("contacts_full", "contacts_count_only", "deepest", "overlaps_full", "overlaps_count_only"):
            case[name] = measure(forms[name])
        case["full_over_overlaps_full"] = round(case["contacts_full"]["ms"] / case["overlaps_full"]["ms"], 2)
        case["deepest_over_overlaps_count_only"] = round(case["deepest"]["ms"] / case["overlaps_count_only"]["ms"], 2)
        case["count_only_over_overlaps_count_only"] = round(case["contacts_count_only"]["ms"] / case["overlaps_count_only"]["ms"], 3)
        # the two count-only forms are one kernel: compared in interleaved rounds, the order swapped from round to round, so that
        # what the form measured before leaves behind (clocks, caches) falls on both alike
        events = (ctx.event(), ctx.event())
        pair = {"contacts_count_only": [], "overlaps_count_only": []}
        for r in range(2 * a.reps):
            for name in sorted(pair, reverse=bool(r & 1)):
                pair[name].append(Q.rep(ctx, events, forms[name], a.launches))
        for e in events:
            ctx.destroy_event(e)
        both = {name: Q.summary(per) for name, per in pair.items()}
        ratio = both["contacts_count_only"]["ms"] / both["overlaps_count_only"]["ms"]
        spread = max((v["ms_max"] - v["ms_min"]) / v["ms"] for v in both.values())
        case["count_only_interleaved"] = {**both, "ratio": round(ratio, 4), "spread": round(spread, 4), "within_spread": bool(abs(ratio - 1.0) <= spread)}
        res["cases"]["size=%g" % size] = case
        recs.dispose()
        idx.dispose()
    Q.emit(res, a.out)
    for buf in [b, deep, stats] + offs:
        buf.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
