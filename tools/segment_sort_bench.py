#!/usr/bin/env python3
"""lbvh_sort_hit_segments on the cfg2 mesh (1 M triangles), on the first 2^20 rays of the two sets of tools/gather_hits_bench.py
((a) first-bounce rays, open range; (b) shadow rays, t in (1e-4, 1)).  Prints one JSON line and writes it to
profiles/segment_sort/segment_sort.json.

Per set, in one process and on the same buffers:
  gather_full           lbvh_gather_hits, full form, into a buffer of exactly M records
  gather_then_sort      the same followed by lbvh_sort_hit_segments: the sort works on records in the order of the walk
  sort_alone            lbvh_sort_hit_segments again and again on the list it has already ordered: the same loads, network steps and
                        stores, but no exchange swaps — a lower bound; sort_on_fresh_ms = gather_then_sort - gather_full is the figure
                        for unsorted input
  host_route            what the call replaces: download the records, np.lexsort by (segment, t, tri), upload (host clock)
and one synthetic list: 2^20 segments of 0 .. 3 records with one segment of 2^20 records among them (the header's cost note).

--parent-tree DIR: a checkout of the parent commit with its library built.  Its lbvh_gather_hits (full form) is measured on the
same rays in a child process of this script (--gather-only --tree DIR), `--rounds` times, each time right before this library's
round: the two versions alternate.

Before any time is kept the device-sorted list of each set is compared with the host lexsort on every record, word for word.
Times: device events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls; per call = median over the
repetitions of all rounds (min / max beside it).  Bytes of the wave tier: 16 per query (two 8-byte offsets per lane) plus 32 per
record of a segment of 2 .. 256 records (one load, one store)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

import query_bench as Q
from query_bench import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS = 1 << 20


def main():
    ap = Q.arguments(launches=10, reps=5, warmup=5, out=os.path.join(ROOT, "profiles", "segment_sort", "segment_sort.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=N_RAYS)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its full lbvh_gather_hits is the yardstick")
    ap.add_argument("--gather-only", action="store_true", help="child mode: time the full lbvh_gather_hits on both sets, print JSON")
    ap.add_argument("--tree", default=ROOT, help="where the package and its library are imported from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    W, Ht = a.width, a.height
    n = min(a.rays, W * Ht)
    tris = scenes.tiled_torus()
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))
    first, live, hit, origin, set_buffers = Q.ray_sets(ctx, s, cam, W, Ht)
    buf = lambda o, dr, t_min, t_max: Q.ray_buffer(ctx, o[:n], dr[:n], t_min, t_max[:n])
    sets = {"a": buf(first["origin"], first["dir"], np.float32(1e-3), np.where(live, np.float32(np.inf), np.float32(0.0))),
            "b": buf(origin, (LIGHT - origin).astype(np.float32), np.float32(1e-4), np.where(hit, np.float32(1.0), np.float32(0.0)))}
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    reps_of = lambda fn: Q.reps_of(ctx, fn, a.launches, a.reps, a.warmup)
    words = lambda x: np.ascontiguousarray(x).view(np.uint32)

    calls, fills, info = {}, {}, {}
    for name, rays in sets.items():
        N.check(h, N.lib.lbvh_gather_hits(h, rays.device, n, C.byref(s), offsets.device, None, 0))
        off = offsets.get_data().copy()
        total = int(off[-1])
        fill = DataBuffer(ctx, max(total, 1), L.HIT)
        fills[name] = fill
        gather = (lambda r, f, t: (lambda: N.lib.lbvh_gather_hits(h, r.device, n, C.byref(s), offsets.device, f.device, t)))(rays, fill, total)
        calls[name] = {"gather_full": gather}
        info[name] = (off, total)
    if a.gather_only:
        print(json.dumps({name: {"per": reps_of(calls[name]["gather_full"]), "M": info[name][1]} for name in sets}))
        ctx.close()
        return

    res = {"workload": "cfg2 mesh (%d triangles), the first %d rays of the %dx%d sets: (a) first-bounce rays, open range; (b) shadow rays, "
                       "t in (1e-4, 1)" % (len(tris), n, W, Ht),
           "launches": a.launches, "reps_per_round": a.reps, "rounds": a.rounds,
           "checks": "the device-sorted list == np.lexsort by (segment, t, tri) of the gathered one, every record word for word: hold",
           "sets": {}}
    host_route = {}
    for name, rays in sets.items():
        off, total = info[name]
        fill, gather = fills[name], calls[name]["gather_full"]
        sort = (lambda f, t: (lambda: N.lib.lbvh_sort_hit_segments(h, offsets.device, n, f.device, t)))(fill, total)

        def both(gather=gather, sort=sort):
            st = gather()
            return st if st != 0 else sort()
        # ---- the check, before any number of this set is kept
        N.check(h, gather())
        walk = fill.get_data().copy()
        segment = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        t0 = time.perf_counter()
        got = fill.get_data()
        want = got[np.lexsort((got["tri"], got["t"], segment))]
        fill.local[:] = want
        fill.sync()
        ctx.sync()
        host_route[name] = round((time.perf_counter() - t0) * 1e3, 2)
        fill.local[:] = walk
        fill.sync()
        N.check(h, sort())
        assert (words(fill.get_data()) == words(want)).all(), "device sort == host lexsort, set %s" % name
        m = np.diff(off.astype(np.int64))
        wave = (m >= 2) & (m <= 256)
        calls[name].update({"gather_then_sort": both, "sort_alone": sort})
        res["sets"][name] = {"rays_in_buffer": n, "M": total, "nonempty": int((m > 0).sum()), "segments_of_2_to_256": int(wave.sum()),
                             "longer_segments": int((m > 256).sum()), "most_hits": int(m.max()),
                             "wave_tier_bytes": int(16 * n + 32 * m[wave].sum()), "host_route_ms": host_route[name]}

    per = {name: {k: [] for k in calls[name]} for name in sets}
    parent = {name: [] for name in sets}
    for _ in range(a.rounds):
        if a.parent_tree:
            env = {k: v for k, v in os.environ.items() if k != "LBVH_LIB"}
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--gather-only", "--tree", os.path.abspath(a.parent_tree),
                                    "--launches", str(a.launches), "--reps", str(a.reps), "--warmup", str(a.warmup), "--width", str(W),
                                    "--height", str(Ht), "--rays", str(a.rays)], env=env, check=True, capture_output=True, text=True)
            got = json.loads(child.stdout.strip().splitlines()[-1])
            for name in sets:
                assert got[name]["M"] == info[name][1], "the parent gathers as many records, set %s" % name
                parent[name] += got[name]["per"]
        for name in sets:
            N.check(h, calls[name]["gather_full"]())                   # offsets of this set, and the sort's input in walk order once
            for k, fn in calls[name].items():
                per[name][k] += reps_of(fn)
    for name in sets:
        out = res["sets"][name]
        for k in calls[name]:
            out[k] = Q.summary(per[name][k])
        fresh = round(out["gather_then_sort"]["ms"] - out["gather_full"]["ms"], 4)
        out["sort_on_fresh_ms"] = fresh
        out["sort_share_of_gather_full"] = round(fresh / out["gather_full"]["ms"], 3)
        out["sort_alone_GB_s"] = round(out["wave_tier_bytes"] / (out["sort_alone"]["ms"] * 1e-3) / 1e9, 1)
        out["sort_costs_less_than_one_walk"] = bool(fresh < 0.5 * out["gather_full"]["ms"])
        if parent[name]:
            p = Q.summary(parent[name])
            out["parent_gather_full"] = p
            out["sort_share_of_parent_gather_full"] = round(fresh / p["ms"], 3)
        else:
            out["parent_gather_full"] = "not measured (no --parent-tree)"

    # ---- one segment of 2^20 records among 2^20 short ones
    rng = np.random.default_rng(1)
    lengths = rng.integers(0, 4, 1 << 20).astype(np.uint64)
    lengths[1 << 19] = 1 << 20
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    ob = DataBuffer(ctx, len(off), np.uint64)
    ob.local[:] = off
    ob.sync()
    hb = DataBuffer(ctx, total, L.HIT)
    rec = np.zeros(total, dtype=L.HIT)
    rec["t"] = rng.random(total, dtype=np.float32)
    rec["tri"] = rng.permutation(total).astype(np.uint32)
    segment = np.repeat(np.arange(len(lengths)), lengths.astype(np.int64))
    want = rec[np.lexsort((rec["tri"], rec["t"], segment))]
    long_fn = lambda: N.lib.lbvh_sort_hit_segments(h, ob.device, len(lengths), hb.device, total)
    times = []
    events = (ctx.event(), ctx.event())
    for _ in range(3):
        hb.local[:] = rec
        hb.sync()
        times.append(Q.rep(ctx, events, long_fn, 1))
    assert (words(hb.get_data()) == words(want)).all(), "the synthetic list"
    lengths[1 << 19] = 0                                               # the same list without the long segment
    ob.local[1:] = np.cumsum(lengths)
    ob.sync()
    res["one_long_segment"] = {"segments": len(lengths), "records": total, "long_segment": 1 << 20, "ms": Q.summary(times),
                               "short_segments_alone_ms": Q.summary(reps_of(lambda: N.lib.lbvh_sort_hit_segments(h, ob.device, len(lengths), hb.device, total)))}
    for e in events:
        ctx.destroy_event(e)
    Q.emit(res, a.out)
    for b in set_buffers + [offsets, ob, hb] + list(sets.values()) + list(fills.values()):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
