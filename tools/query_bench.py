"""What the query bench tools (tools/*_bench.py) share: the --launches / --reps / --warmup / --out arguments, device-event timing,
the statistics of one more call, the JSON line with --out, and the two ray sets most of them run on.  Each tool keeps its own
docstring, checks and result layout.  The package is imported inside the functions: a tool puts its tree on sys.path first."""
import argparse
import collections
import ctypes as C
import json
import os

import numpy as np

LIGHT = np.array([0.0, 250.0, 150.0], dtype=np.float32)      # the point light of the shadow rays: outside the scene box


def arguments(launches, reps, warmup, out=None):
    """the parser with the four shared options at the tool's own defaults; the tool adds its size options"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=launches)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--out", default=out, help="also write the JSON here")
    return ap


def _check(ctx, status):
    from unitysimpleraytracing_amd import _native as N
    N.check(ctx.handle, status)


def rep(ctx, events, fn, launches):
    """ms per call: the two device events (ctx.event()) around `launches` back-to-back calls"""
    e0, e1 = events
    ctx.record(e0)
    for _ in range(launches):
        _check(ctx, fn())
    ctx.record(e1)
    return ctx.elapsed_ms(e0, e1) / launches


def summary(per, active=None, rate="Mrays_s_active", digits=1):
    """median, min and max of the repetitions; with `active`, the millions of active queries per second under the key `rate`"""
    per = sorted(per)
    ms = per[len(per) // 2]
    out = {"ms": round(ms, 4), "ms_min": round(per[0], 4), "ms_max": round(per[-1], 4)}
    if active is not None:
        out[rate] = round(active / (ms * 1e-3) / 1e6, digits)
    return out


def reps_of(ctx, fn, launches, reps, warmup):
    """`warmup` calls, then `reps` repetitions: ms per call of each, in the order measured"""
    for _ in range(warmup):
        _check(ctx, fn())
    events = (ctx.event(), ctx.event())
    per = [rep(ctx, events, fn, launches) for _ in range(reps)]
    for e in events:
        ctx.destroy_event(e)
    return per


def timed(ctx, fn, active, launches, reps, warmup, rate="Mrays_s_active", digits=1):
    """summary() of reps_of(): per call = median over the repetitions, min / max beside it"""
    return summary(reps_of(ctx, fn, launches, reps, warmup), active, rate, digits)


Counters = collections.namedtuple("Counters", "rays node_fetches triangle_tests")


def counters(ctx, stats, fn):
    """lbvh_ray_stats_target around one more call of fn -> Counters; stats: a one-record RAY_STATS DataBuffer"""
    from unitysimpleraytracing_amd import _native as N
    stats.fill_u32(0)
    _check(ctx, N.lib.lbvh_ray_stats_target(ctx.handle, stats.device))
    _check(ctx, fn())
    _check(ctx, N.lib.lbvh_ray_stats_target(ctx.handle, None))
    c = stats.get_data()[0]
    return Counters(int(c["rays"]), int(c["node_fetches"]), int(c["triangle_tests"]))


def per_active(c):
    """(node fetches, triangle tests) per walked query, three decimals"""
    r = max(c.rays, 1)
    return round(c.node_fetches / r, 3), round(c.triangle_tests / r, 3)


def emit(res, out):
    """the one JSON line on stdout and, with --out, in that file"""
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def ray_sets(ctx, scene, cam, width, height):
    """The two ray sets of tools/ray_queries_bench.py for one camera, as host arrays -> (first, live, hit, origin, buffers):
      first-bounce rays   `first` (lbvh_path_first_bounce's states), `live` = alive != 0
      shadow rays         from every primary hit (`hit`) toward LIGHT: origin `origin`, dir = LIGHT - origin, not normalised
    `buffers`: what the caller disposes; buffers[0] holds `first` on the device."""
    from unitysimpleraytracing_amd import _native as N
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd.host import DataBuffer
    h, n = ctx.handle, width * height
    states = DataBuffer(ctx, n, L.PATH_STATE)
    prim = DataBuffer(ctx, n, L.HIT)
    hits = DataBuffer(ctx, n, L.HIT)
    N.check(h, N.lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, width, height, C.byref(scene), L.TRACE_FAST, prim.device, None))
    N.check(h, N.lib.lbvh_path_begin(h, C.byref(cam), states.device))
    camera_rays = states.get_data().copy()
    ph = prim.get_data().copy()
    N.check(h, N.lib.lbvh_buffer_upload(h, hits.device, ph.ctypes.data_as(C.c_void_p), ph.nbytes))
    N.check(h, N.lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(scene), states.device, hits.device, 9, 0.7, 1e-3))
    first = states.get_data().copy()
    origin = (camera_rays["origin"] + camera_rays["dir"] * ph["t"][:, None]).astype(np.float32)
    return first, first["alive"] != 0, ph["t"] < L.MAX_FLOAT, origin, [states, prim, hits]


def ray_buffer(ctx, origin, direction, t_min, t_max):
    """lbvh_ray records on the device; t_min / t_max: scalars or one per ray"""
    from unitysimpleraytracing_amd import layouts as L
    from unitysimpleraytracing_amd.host import DataBuffer
    b = DataBuffer(ctx, len(origin), L.RAY)
    b.local["origin"], b.local["dir"], b.local["t_min"], b.local["t_max"] = origin, direction, t_min, t_max
    b.sync()
    return b
