#!/usr/bin/env python3
"""lbvh_sort_record_segments on the cfg2 mesh (1 M triangles) behind its five producers, each with `--queries` queries of `--size`
of the scene's extent drawn about points of the surface (planes: `--planes` random planes through the mesh).  Prints one JSON line
and writes it to profiles/record_sort/record_sort.json.

Per producer, in one process and on the same buffers, in interleaved rounds (every round measures every form once, in this order):
  full                  the producing call, full form, into a buffer of exactly M records
  full_then_sort        the same followed by lbvh_sort_record_segments in the order of the list: the sort works on records in the
                        order of the walk; sort_on_fresh_ms = full_then_sort - full, sort_share = that over full_then_sort (the worth)
  sort_alone            lbvh_sort_record_segments again and again on the list it has already ordered: the same loads, network steps
                        and stores, but no exchange swaps — a lower bound
  floor_hit_sort        lbvh_sort_hit_segments as it stands on the SAME offsets over a 16-byte buffer of M records (the first 16
                        bytes of every record, already ordered the same way): half the bytes through an unchanged kernel;
                        ratio_to_floor = sort_alone / floor_hit_sort
  host_route            what the call replaces: download the records, np.lexsort by (segment, key), upload (host clock)
and one synthetic list (`long_segment`): 2^20 segments of 0 .. 3 records with one segment of 2^20 records among them, as the
16-byte sort records it (the header's cost note); --no-long leaves it out.

--variant LIB: another build of the library (tools/build_variant.sh record_direct -DLBVH_RECORD_SORT_DIRECT: the straightforward
32-byte instantiation of the 16-byte template).  Its full_then_sort and sort_alone are measured on the same queries in a child
process of this script (--child), once per round, right before this library's round: the two builds alternate.  The design claim
is `beats_variant`: the medians differ by more than the spread (max - min) of either side's rounds.

Before any time is kept the device-sorted list of each producer is compared with the host lexsort on every record, word for word.
Times: device events around `--launches` back-to-back calls, `--reps` times after `--warmup` calls (the clocks settle there); per
call = median over the repetitions of all rounds (min / max beside it)."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

import query_bench as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("contacts", "boxcontacts", "triprox", "trisegs", "sections")


def order_key(words8, order):
    """(more significant, less significant) key words of (n, 8) record words: K / D of include/lbvh.h, or word 3"""
    if order == 2:
        return words8[:, 3], np.zeros(len(words8), dtype=np.uint32)
    w = words8[:, 0].copy()
    nan = (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    w[w == np.uint32(0x80000000)] = 0
    k = np.where((w & np.uint32(0x80000000)) != 0, ~w, w | np.uint32(0x80000000))
    if order == 1:
        k = ~k
    return np.where(nan, np.uint32(0xFFFFFFFF), k).astype(np.uint32), words8[:, 1]


def host_sorted(off, words8, order):
    segment = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    high, low = order_key(words8, order)
    return words8[np.lexsort((low, high, segment))]


def main():
    ap = Q.arguments(launches=3, reps=3, warmup=2, out=os.path.join(ROOT, "profiles", "record_sort", "record_sort.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--size", type=float, default=0.005, help="of the scene's extent")
    ap.add_argument("--kinds", nargs="+", default=list(KINDS))
    ap.add_argument("--max-list", type=int, default=1 << 26, help="the most records a list is given")
    ap.add_argument("--variant", default=None, help="a variant build of the library (LBVH_LIB of the child process)")
    ap.add_argument("--child", action="store_true", help="child mode: one round of full_then_sort / sort_alone per producer, JSON on stdout")
    ap.add_argument("--no-long", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)

    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd import scenes
    from unitysimpleraytracing_amd.host import Context, DataBuffer, RaytracingMeshDrawer, planes as host_planes

    n = a.queries
    tris = scenes.tiled_torus()
    ta, tb, tc = (np.ascontiguousarray(tris[k][:, :3], dtype=np.float32) for k in "abc")
    pts = np.concatenate([ta, tb, tc])
    extent = float((pts.max(axis=0) - pts.min(axis=0)).max())
    ctx = Context(0)
    h, lib = ctx.handle, N.lib
    d = RaytracingMeshDrawer(ctx, tris).awake()
    s = d.container.scene()

    rng = np.random.default_rng(1)                                   # the draws of tools/shape_contacts_bench.py, in its order
    k = rng.integers(0, len(tris), n)
    w = rng.dirichlet((1, 1, 1), n)
    surface = ta[k] * w[:, :1] + tb[k] * w[:, 1:2] + tc[k] * w[:, 2:]
    off = rng.normal(size=(n, 3))
    off *= (rng.uniform(0.0, 1.0, n) / np.linalg.norm(off, axis=1))[:, None]
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    sz = a.size * extent
    centre = (surface + off * sz).astype(np.float32)
    corners = [(centre + rng.normal(size=(n, 3)) * (0.5 * sz)).astype(np.float32) for _ in range(3)]

    def capsules(b):
        b.local["origin"], b.local["axis"], b.local["radius"] = centre - axis * sz, axis * (2.0 * sz), np.float32(0.5 * sz)

    def boxes(b):
        b.local["centre"] = centre
        for j, name in enumerate(("ax", "ay", "az")):
            b.local[name] = np.roll(np.eye(3, dtype=np.float32), j, axis=1)[0] * np.float32(0.5 * sz)

    def prox(b):
        b.local["a"], b.local["b"], b.local["c"] = corners
        b.local["max_dist2"], b.local["skip"] = np.float32(sz * sz), L.NULL

    def cuts(b):
        b.local["a"], b.local["b"], b.local["c"] = corners
        b.local["skip"] = L.NULL

    def sections(b):
        nrm = rng.normal(size=(a.planes, 3))
        b.local[:] = host_planes(nrm, rng.uniform(pts.min(axis=0), pts.max(axis=0), (a.planes, 3)))

    producers = {
        "contacts": (L.CAPSULE, L.CONTACT, capsules, lib.lbvh_capsule_contacts, N.SORT_RECORDS_DESCENDING, n),
        "boxcontacts": (L.OBB, L.BOX_CONTACT, boxes, lib.lbvh_obb_contacts, N.SORT_RECORDS_DESCENDING, n),
        "triprox": (L.TRI_DISTANCE_QUERY, L.TRI_CLOSEST, prox, lib.lbvh_triangle_gather_within_distance, N.SORT_RECORDS_ASCENDING, n),
        "trisegs": (L.TRI_QUERY, L.TRI_SEGMENT, cuts, lib.lbvh_triangle_intersection_segments, N.SORT_RECORDS_BY_TRI, n),
        "sections": (L.PLANE, L.PLANE_SEGMENT, sections, lib.lbvh_plane_sections, N.SORT_RECORDS_BY_TRI, a.planes),
    }

    def variant_round(kind):
        """one round of the variant build in a child process -> {kind: {form: [ms, ...]}}"""
        if not a.variant:
            return {}
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--queries", str(n), "--planes", str(a.planes), "--size", str(a.size),
               "--launches", str(a.launches), "--reps", str(a.reps), "--warmup", str(a.warmup), "--max-list", str(a.max_list), "--no-long",
               "--kinds", kind]
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, env={**os.environ, "LBVH_LIB": os.path.abspath(a.variant)}).stdout
        return json.loads(out.strip().splitlines()[-1])

    cases = {}
    for kind in a.kinds:
        q_dtype, r_dtype, fill, call, order, count = producers[kind]
        qb = DataBuffer(ctx, count, q_dtype)
        fill(qb)
        qb.sync()
        ob = DataBuffer(ctx, count + 1, np.uint64)
        N.check(h, call(h, qb.device, count, C.byref(s), ob.device, None, 0))
        offsets = ob.get_data()[: count + 1].copy()
        total = int(offsets[count])
        cap = max(min(total, a.max_list), 1)
        assert total <= a.max_list, "%s: %d records, raise --max-list or lower --size" % (kind, total)
        rb, hb = DataBuffer(ctx, cap, r_dtype), DataBuffer(ctx, cap, L.HIT)
        full = lambda: call(h, qb.device, count, C.byref(s), ob.device, rb.device, cap)
        sort = lambda: lib.lbvh_sort_record_segments(h, ob.device, count, rb.device, cap, order)
        floor = lambda: lib.lbvh_sort_hit_segments(h, ob.device, count, hb.device, cap)
        full_then_sort = lambda: full() or sort()
        # ---- the check, before any number of this producer is kept
        N.check(h, full())
        walk = rb.get_data()[:total].copy().view(np.uint32).reshape(-1, 8)
        N.check(h, sort())
        got = rb.get_data()[:total].copy().view(np.uint32).reshape(-1, 8)
        assert (got == host_sorted(offsets, walk, order)).all(), kind + ": the device order is not the host lexsort's"
        hb.local.view(np.uint32).reshape(-1, 4)[:total] = got[:, :4]
        hb.sync()
        N.check(h, floor())
        if a.child:
            cases[kind] = {"full_then_sort": Q.reps_of(ctx, full_then_sort, a.launches, a.reps, a.warmup),
                           "sort_alone": Q.reps_of(ctx, sort, a.launches, a.reps, a.warmup)}
        else:
            per = {name: [] for name in ("full", "full_then_sort", "sort_alone", "floor_hit_sort")}
            var = {"full_then_sort": [], "sort_alone": []}
            host = []
            for _ in range(a.rounds):
                for name, ms in variant_round(kind).get(kind, {}).items():
                    var[name] += ms
                per["full"] += Q.reps_of(ctx, full, a.launches, a.reps, a.warmup)
                per["full_then_sort"] += Q.reps_of(ctx, full_then_sort, a.launches, a.reps, a.warmup)
                per["sort_alone"] += Q.reps_of(ctx, sort, a.launches, a.reps, a.warmup)
                per["floor_hit_sort"] += Q.reps_of(ctx, floor, a.launches, a.reps, a.warmup)
                N.check(h, full())
                ctx.sync()
                t0 = time.perf_counter()
                words8 = rb.get_data()[:total].view(np.uint32).reshape(-1, 8)
                rb.local.view(np.uint32).reshape(-1, 8)[:total] = host_sorted(offsets, words8, order)
                rb.sync()
                ctx.sync()
                host.append((time.perf_counter() - t0) * 1e3)
            m = np.diff(offsets).astype(np.int64)
            row = {"queries": count, "records": total, "order": int(order), "longest_segment": int(m.max()) if len(m) else 0,
                   "segments_2_to_256": int(((m >= 2) & (m <= 256)).sum()), "segments_above_256": int((m > 256).sum())}
            row.update({name: Q.summary(v) for name, v in per.items()})
            row["host_route"] = Q.summary(host)
            fresh = row["full_then_sort"]["ms"] - row["full"]["ms"]
            row["sort_on_fresh_ms"] = round(fresh, 4)
            row["sort_share_of_full_then_sort"] = round(fresh / row["full_then_sort"]["ms"], 4)
            row["ratio_to_floor"] = round(row["sort_alone"]["ms"] / max(row["floor_hit_sort"]["ms"], 1e-9), 3)
            if a.variant:
                row["variant_direct"] = {name: Q.summary(v) for name, v in var.items()}
                ours, theirs = row["full_then_sort"], row["variant_direct"]["full_then_sort"]
                spread = max(ours["ms_max"] - ours["ms_min"], theirs["ms_max"] - theirs["ms_min"])
                row["beats_variant"] = bool(theirs["ms"] - ours["ms"] > spread)
            cases[kind] = row
        for b in (qb, ob, rb, hb):
            b.dispose()

    if a.child:
        print(json.dumps(cases))
        return

    res = {"workload": "cfg2 mesh (%d triangles, extent %.4g); %d queries of %.3g of the extent about the surface per producer, %d planes"
                       % (len(tris), extent, n, a.size, a.planes),
           "launches": a.launches, "reps": a.reps, "rounds": a.rounds, "variant": os.path.basename(a.variant) if a.variant else None,
           "checks": "the device-sorted list of every producer equals the host lexsort word for word: holds", "cases": cases}

    if not a.no_long:                                                # one segment of 2^20 records among 2^20 short ones
        rng = np.random.default_rng(2)
        lengths = rng.integers(0, 4, 1 << 20)
        lengths[1 << 19] = 1 << 20
        offsets = np.zeros(len(lengths) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lengths.astype(np.uint64))
        total = int(offsets[-1])
        words8 = rng.integers(0, 1 << 32, (total, 8), dtype=np.uint64).astype(np.uint32)
        words8[:, 0] = rng.uniform(0.0, 1.0, total).astype(np.float32).view(np.uint32)
        ob, rb = DataBuffer(ctx, len(offsets), np.uint64), DataBuffer(ctx, total, L.CONTACT)
        ob.local[:] = offsets
        ob.sync()
        per = []
        for _ in range(a.rounds):
            rb.local.view(np.uint32).reshape(-1, 8)[:] = words8
            rb.sync()
            ev = (ctx.event(), ctx.event())
            per.append(Q.rep(ctx, ev, lambda: lib.lbvh_sort_record_segments(h, ob.device, len(lengths), rb.device, total, 0), 1))
            for e in ev:
                ctx.destroy_event(e)
        assert (rb.get_data().view(np.uint32).reshape(-1, 8) == host_sorted(offsets, words8, 0)).all(), "long segment"
        res["long_segment"] = {"segments": len(lengths), "records": total, "longest": 1 << 20, "on_fresh_input": Q.summary(per)}
    Q.emit(res, a.out)


if __name__ == "__main__":
    main()
