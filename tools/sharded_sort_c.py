#!/usr/bin/env python3
"""lbvh_sort_pairs_sharded measured: one call over one context per listed device (a device may repeat: logical ranks on one
GPU — then this is NOT a scaling number, the contexts share that GPU), next to lbvh_sort_pairs of the same N on one context,
checked word for word against it.  Prints one JSON object.

    tools/sharded_sort_c.py <devices...> [--n 16000000] [--replicate] [--keys uniform|cfg4] [--reps 5]

  call_ms         device span of the whole call (HIP events before / after it on every context; slowest context), profiler off
  host_ms         host wall time of the call plus the sync of every context
  stages_ms       per stage, slowest context (a separate run under lbvh_profile_begin: every stage and kernel bracketed by
                  events): local sort, splitter rounds (device-side waits included), exchange, receive sort, broadcast
  kernels_ms      per kernel name, summed over the contexts (same run)
  copy            the range-copy kernel's rate at 8 bytes read + 8 written per moved pair, against the device copy rate
                  (lbvh_copy_bandwidth_probe) — rate_w1: one context, no concurrent kernels; rate_exchange: the W-context
                  exchange with every kernel's bytes over the SUM of the kernels' times (a lower bound when they overlap)
  sort_pairs_ms   lbvh_sort_pairs of the N pairs on one context (the first device)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitysimpleraytracing_amd import _native as N                                          # noqa: E402
from unitysimpleraytracing_amd import scenes                                                # noqa: E402
from unitysimpleraytracing_amd.host import Context, DataBuffer, MeshBufferContainer, MultiGpuSorter   # noqa: E402
from unitysimpleraytracing_amd.sharded_sort import block_of                                 # noqa: E402

STAGES = ("local_sort", "splitters", "exchange", "receive_sort", "broadcast")


def make_keys(kind, n):
    if kind == "uniform":
        return np.random.default_rng(1).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    with Context(0) as ctx:          # cfg4's mesh: 16 M triangles -> Morton codes + capacity pads
        c = MeshBufferContainer(ctx, scenes.tiled_torus(nu=400, nv=160))
        k = c.keys.get_data()[:n].copy()
        c.dispose()
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("devices", type=int, nargs="+")
    ap.add_argument("--n", type=int, default=16_000_000)
    ap.add_argument("--replicate", action="store_true")
    ap.add_argument("--keys", choices=["uniform", "cfg4"], default="uniform")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, W = a.n, len(a.devices)
    keys = make_keys(a.keys, n)
    vals = np.arange(n, dtype=np.uint32)
    sorter = MultiGpuSorter(a.devices)
    ctxs = sorter.contexts
    bounds = [block_of(r, W, n) for r in range(W)]
    ins = [(DataBuffer(c, max(b - a_, 1), np.uint32), DataBuffer(c, max(b - a_, 1), np.uint32)) for c, (a_, b) in zip(ctxs, bounds)]
    outs = [(DataBuffer(c, n, np.uint32), DataBuffer(c, n, np.uint32)) for c in ctxs]

    def restore():                  # the call sorts its inputs in place: every repetition starts from the original blocks
        for (bk, bv), (lo, hi) in zip(ins, bounds):
            bk.local[: hi - lo] = keys[lo:hi]
            bv.local[: hi - lo] = vals[lo:hi]
            bk.sync(); bv.sync()
        sorter.sync()

    def call():
        return sorter.sort_device([b[0].device for b in ins], [b[1].device for b in ins], [hi - lo for lo, hi in bounds],
                                  [o[0].device for o in outs], [o[1].device for o in outs], [n] * W, replicate=a.replicate)

    restore(); call(); sorter.sync()                     # warm-up: scratch, peers, code objects
    call_ms, host_ms = [], []
    ev = [(c.event(), c.event()) for c in ctxs]
    for _ in range(a.reps):
        restore()
        for c, (e0, _) in zip(ctxs, ev):
            c.record(e0)
        t0 = time.perf_counter()
        counts = call()
        for c, (_, e1) in zip(ctxs, ev):
            c.record(e1)
        sorter.sync()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        call_ms.append(max(c.elapsed_ms(e0, e1) for c, (e0, e1) in zip(ctxs, ev)))
    # stages and kernels, profiler on (a run of its own)
    restore()
    for c in ctxs:
        c.profile_begin()
    call()
    rows = [c.profile_end() for c in ctxs]
    stages = {s: max(r.get("sharded:" + s, (0, 0.0))[1] for r in rows) for s in STAGES}
    kernels = {}
    for r in rows:
        for name, (launches, ms) in r.items():
            if not name.startswith("sharded:"):
                l0, m0 = kernels.get(name, (0, 0.0))
                kernels[name] = (l0 + launches, m0 + ms)
    exchange_ms = sum(r.get("sharded:exchange", (0, 0.0))[1] for r in rows)
    # the word-for-word check against lbvh_sort_pairs on one context, and that sort's time
    one = ctxs[0]
    k1, v1 = DataBuffer(one, n, np.uint32), DataBuffer(one, n, np.uint32)
    sp_ms = []
    e0, e1 = ev[0]
    for _ in range(a.reps + 1):
        k1.local[:] = keys
        v1.local[:] = vals
        k1.sync(); v1.sync()
        one.record(e0)
        N.check(one.handle, N.lib.lbvh_sort_pairs(one.handle, k1.device, v1.device, n))
        one.record(e1)
        sp_ms.append(one.elapsed_ms(e0, e1))
    want_k, want_v = k1.get_data().copy(), v1.get_data().copy()
    restore()
    counts = call()
    equal, at = True, 0
    for q, (ok, ov) in enumerate(outs):
        m, lo = (n, 0) if a.replicate else (counts[q], at)
        equal = equal and bool((ok.get_data()[:m] == want_k[lo: lo + m]).all() and (ov.get_data()[:m] == want_v[lo: lo + m]).all())
        at += counts[q]
    equal = equal and at == n
    # copy rates: the device's plain copy (16-byte loads / stores), the range copy alone (W = 1), the W-context exchange
    nbytes = (n * 8) // 16 * 16
    N.check(one.handle, N.lib.lbvh_copy_bandwidth_probe(one.handle, outs[0][0].device, k1.device, nbytes // 2))
    probe = []
    for _ in range(5):
        one.record(e0)
        N.check(one.handle, N.lib.lbvh_copy_bandwidth_probe(one.handle, outs[0][0].device, k1.device, nbytes // 2))
        one.record(e1)
        probe.append(one.elapsed_ms(e0, e1))
    device_copy_gbs = nbytes / min(probe) / 1e6
    w1 = []
    for _ in range(3):
        one.profile_begin()
        st = N.lib.lbvh_sort_pairs_sharded((C.c_void_p * 1)(one.handle.value), 1, (C.c_void_p * 1)(k1.device.value),
                                           (C.c_void_p * 1)(v1.device.value), (C.c_uint32 * 1)(n), (C.c_void_p * 1)(outs[0][0].device.value),
                                           (C.c_void_p * 1)(outs[0][1].device.value), (C.c_uint32 * 1)(n), (C.c_uint32 * 1)(), 0)
        N.check(one.handle, st)
        w1.append(one.profile_end().get("shard_range_copy_kernel", (0, float("nan")))[1])
    print(json.dumps({
        "what": "lbvh_sort_pairs_sharded, %d contexts on devices %s%s" % (W, a.devices,
                " (contexts share one GPU: NOT a scaling number)" if len(set(a.devices)) < W else ""),
        "keys": a.keys, "pairs": n, "replicate": a.replicate, "equal": equal, "slice_counts": counts,
        "call_ms": round(min(call_ms), 3), "call_ms_median": round(float(np.median(call_ms)), 3), "host_ms": round(min(host_ms), 3),
        "stages_ms": {s: round(v, 3) for s, v in stages.items()},
        "kernels_ms": {k: [l, round(m, 3)] for k, (l, m) in sorted(kernels.items(), key=lambda kv: -kv[1][1])},
        "sort_pairs_ms": round(min(sp_ms[1:]), 3),
        "copy": {"device_copy_GBs": round(device_copy_gbs, 1),
                 "rate_w1_GBs": round(16 * n / min(w1) / 1e6, 1), "rate_w1_vs_device": round(16 * n / min(w1) / 1e6 / device_copy_gbs, 3),
                 "rate_exchange_GBs": round(16 * n / exchange_ms / 1e6, 1) if exchange_ms else None,
                 "rate_exchange_vs_device": round(16 * n / exchange_ms / 1e6 / device_copy_gbs, 3) if exchange_ms else None},
    }))
    for pair in ins + outs:
        for b in pair:
            b.dispose()
    k1.dispose(); v1.dispose()
    for c, (e0, e1) in zip(ctxs, ev):
        c.destroy_event(e0); c.destroy_event(e1)
    sorter.close()
    return 0 if equal else 2


if __name__ == "__main__":
    sys.exit(main())
