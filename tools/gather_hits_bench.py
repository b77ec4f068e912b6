#!/usr/bin/env python3
"""lbvh_gather_hits on the cfg2 mesh (1 M triangles), on the first 2^20 rays of the two sets of tools/k_hits_bench.py.  Prints one
JSON line and writes it to profiles/gather_hits/gather_hits.json.

  (a) first-bounce secondary rays (lbvh_path_first_bounce's states as lbvh_ray records; dead paths: inactive rays),
      t_min = 1e-3, t_max = +inf
  (b) shadow rays from every primary hit toward a point light outside the scene box (dir = light - hit point, not normalised;
      t in (1e-4, 1); pixels without a hit: inactive)
On each set, in one process and on the same buffer: the count-only form (capacity 0: one walk and the scan), the full form (count,
scan, fill into a buffer of exactly M records) and, for context, lbvh_count_hits and lbvh_trace_k_closest at k = 32; node lines and
triangle tests per active ray of each (lbvh_ray_stats_target on one more call).

--parent-tree DIR: a checkout of the parent commit with its library built.  Its lbvh_count_hits is measured on the same rays in a
child process of this script (--count-hits-only --tree DIR: the package and the library are imported from DIR), `--rounds` times,
each time right before this library's round: the two versions alternate, as they must when a difference is to be trusted.  The
margin is the parent's own run-to-run spread: max - min over all its repetitions of all rounds.  The verdict compares the count-only form's median with the parent count's median plus that spread.

Before anything is printed the outputs are checked, GPU against GPU on every ray: segment lengths == lbvh_count_hits, the
sorted head of every segment == its row of lbvh_trace_k_closest at k = 32 (record 0: the closest hit); and `--check` rays of each set
against tests/gather_hits_reference.py (brute force over all triangles, word for word after the canonical sort).  Times: device
events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls (the clocks settle there); per call = median
over the repetitions of all rounds (min / max beside it: the spread)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

import query_bench as Q
from query_bench import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_RAYS = 1 << 20


def summary(per, active):
    t = Q.summary(per, active)
    return {"ms": t["ms"], "ms_min": t["ms_min"], "ms_max": t["ms_max"], "reps": len(per), "Mrays_s_active": t["Mrays_s_active"]}


def main():
    ap = Q.arguments(launches=10, reps=5, warmup=5, out=os.path.join(ROOT, "profiles", "gather_hits", "gather_hits.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rays", type=int, default=N_RAYS)
    ap.add_argument("--check", type=int, default=16, help="rays of each set compared with the brute force")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its lbvh_count_hits is the yardstick")
    ap.add_argument("--count-hits-only", action="store_true", help="child mode: time lbvh_count_hits on both sets, print JSON")
    ap.add_argument("--tree", default=ROOT, help="where the package and its library are imported from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer

    W, Ht = a.width, a.height
    n_px = W * Ht
    n = min(a.rays, n_px)
    tris = scenes.tiled_torus()
    ctx = Context(0)
    h = ctx.handle
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()
    cam = N.Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 250.0)))

    # primary hits + first-bounce states, as tools/k_hits_bench.py makes them
    first, live, hit, origin, set_buffers = Q.ray_sets(ctx, s, cam, W, Ht)

    def ray_buffer(origin, direction, t_min, t_max):         # the first n rays of a set
        return Q.ray_buffer(ctx, origin[:n], direction[:n], t_min, t_max[:n])

    sets = {"a": ray_buffer(first["origin"], first["dir"], np.float32(1e-3), np.where(live, np.float32(np.inf), np.float32(0.0))),
            "b": ray_buffer(origin, (LIGHT - origin).astype(np.float32), np.float32(1e-4), np.where(hit, np.float32(1.0), np.float32(0.0)))}
    active = {k: int((b.local["t_min"] < b.local["t_max"]).sum()) for k, b in sets.items()}
    cnt = DataBuffer(ctx, n, np.uint32)

    def reps_of(fn):
        return Q.reps_of(ctx, fn, a.launches, a.reps, a.warmup)

    count_fn = lambda rays: (lambda: N.lib.lbvh_count_hits(h, rays.device, n, C.byref(s), cnt.device))

    if a.count_hits_only:
        out = {}
        for name, rays in sets.items():
            per = reps_of(count_fn(rays))
            out[name] = {"per": per, "count_sum": int(cnt.get_data().astype(np.uint64).sum())}
        print(json.dumps(out))
        ctx.close()
        return

    import gather_hits_reference as G
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    box = d.container.triangle_aabb.get_data()[: len(tris)]
    lo, hi = box["min"].copy(), box["max"].copy()
    offsets = DataBuffer(ctx, n + 1, np.uint64)
    rows = DataBuffer(ctx, n * 32, L.HIT)
    found = DataBuffer(ctx, n, np.uint32)
    stats = DataBuffer(ctx, 1, L.RAY_STATS)

    def work(fn):
        c = Q.counters(ctx, stats, fn)
        lines, tests = Q.per_active(c)
        return {"rays_walked": c.rays, "node_lines_per_ray": lines, "triangle_tests_per_ray": tests}

    words = lambda x: np.ascontiguousarray(x).view(np.uint32)
    res = {"workload": "cfg2 mesh (%d triangles), the first %d rays of the %dx%d sets: (a) first-bounce rays, open range; (b) shadow rays, "
                       "t in (1e-4, 1)" % (len(tris), n, W, Ht),
           "launches": a.launches, "reps_per_round": a.reps, "rounds": a.rounds, "walker": "four-wide (the default) for every call",
           "checks": "for every ray: segment length == lbvh_count_hits, canonical head == lbvh_trace_k_closest at k = 32 (rows and found); "
                     "offsets and canonical segments word for word against the brute force on %d rays of each set: hold" % a.check,
           "sets": {}}
    calls, fills = {}, {}
    for name, rays in sets.items():
        count_only = (lambda r: (lambda: N.lib.lbvh_gather_hits(h, r.device, n, C.byref(s), offsets.device, None, 0)))(rays)
        N.check(h, count_only())
        off = offsets.get_data().copy()
        total = int(off[-1])
        fill = DataBuffer(ctx, max(total, 1), L.HIT)
        fills[name] = fill
        full = (lambda r, f, t: (lambda: N.lib.lbvh_gather_hits(h, r.device, n, C.byref(s), offsets.device, f.device, t)))(rays, fill, total)
        k32 = (lambda r: (lambda: N.lib.lbvh_trace_k_closest(h, r.device, n, 32, C.byref(s), rows.device, found.device)))(rays)
        # ---- checks, before any number of this set is kept
        fill.fill_u32(0x7FC00000)
        N.check(h, full())
        assert (offsets.get_data() == off).all(), "offsets, count-only against full, set %s" % name
        canon = G.canonical(off, fill.get_data())
        N.check(h, count_fn(rays)())
        counts = cnt.get_data().copy()
        m = np.diff(off.astype(np.int64))
        assert (m == counts).all(), "segment length == count_hits, set %s" % name
        N.check(h, k32())
        got, f = rows.get_data().reshape(n, 32), found.get_data()
        assert (f == np.minimum(m, 32)).all(), "found, set %s" % name
        qi, ji = np.nonzero(np.arange(32)[None, :] < m[:, None])
        assert (words(got[qi, ji]) == words(canon[off.astype(np.int64)[qi] + ji])).all(), "canonical head == k = 32 rows, set %s" % name
        act = np.nonzero(rays.local["t_min"] < rays.local["t_max"])[0]
        sub = act[(np.arange(a.check) * (len(act) // max(a.check, 1))).astype(np.int64)]
        ref = G.reference(rays.local[sub], ta, tb, tc, lo, hi)
        assert (np.diff(ref.offsets.astype(np.int64)) == m[sub]).all(), "brute force counts, set %s" % name
        mine = np.concatenate([canon[int(off[q]): int(off[q + 1])] for q in sub]) if len(sub) else canon[:0]
        assert (words(mine) == words(ref.records)).all(), "brute force records, set %s" % name
        calls[name] = {"count_hits": count_fn(rays), "gather_count_only": count_only, "gather_full": full, "trace_k_closest_32": k32}
        res["sets"][name] = {"rays_in_buffer": n, "active_rays": active[name], "M": total,
                             "hits_per_active_ray": round(total / max(active[name], 1), 3), "most_hits": int(m.max()),
                             "count_sum": int(counts.astype(np.uint64).sum())}

    # ---- times: the parent's count (child process) and this library's calls, alternating
    per = {name: {k: [] for k in calls[name]} for name in sets}
    parent = {name: [] for name in sets}
    for _ in range(a.rounds):
        if a.parent_tree:
            env = {k: v for k, v in os.environ.items() if k != "LBVH_LIB"}
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--count-hits-only", "--tree", os.path.abspath(a.parent_tree), "--launches", str(a.launches), "--reps", str(a.reps),
                                    "--warmup", str(a.warmup), "--width", str(W), "--height", str(Ht), "--rays", str(a.rays)],
                                   env=env, check=True, capture_output=True, text=True)
            got = json.loads(child.stdout.strip().splitlines()[-1])
            for name in sets:
                assert got[name]["count_sum"] == res["sets"][name]["count_sum"], "the parent counts the same, set %s" % name
                parent[name] += got[name]["per"]
        for name in sets:
            for k, fn in calls[name].items():
                per[name][k] += reps_of(fn)
    for name in sets:
        out = res["sets"][name]
        for k, fn in calls[name].items():
            out[k] = {**summary(per[name][k], active[name]), **work(fn)}
        co, fu, ch = out["gather_count_only"], out["gather_full"], out["count_hits"]
        out["full_over_count_only"] = {"ms": round(fu["ms"] - co["ms"], 4), "ratio": round(fu["ms"] / co["ms"], 3)}
        out["count_only_vs_count_hits_this_library"] = round(co["ms"] / ch["ms"], 3)
        if parent[name]:
            p = summary(parent[name], active[name])
            spread = round(p["ms_max"] - p["ms_min"], 4)
            out["parent_count_hits"] = p
            out["parent_spread_ms"] = spread
            out["count_only_minus_parent_count_ms"] = round(co["ms"] - p["ms"], 4)
            out["count_only_slower_than_parent_count_by_more_than_the_spread"] = bool(co["ms"] > p["ms"] + spread)
        else:
            out["parent_count_hits"] = "not measured (no --parent-tree)"
    Q.emit(res, a.out)
    for b in set_buffers + [rows, found, cnt, stats, offsets] + list(sets.values()) + list(fills.values()):
        b.dispose()
    d.on_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
