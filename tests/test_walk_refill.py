"""The lane refill of the per-lane walkers, and the overlap scan at scale.

Every per-lane walk of lbvh_path.hip and lbvh_query_*.hip launches min(8192, ceil(count / 64)) one-wave workgroups; a wave owns a run of
ceil(count / waves) consecutive queries and refills a lane from the run when the lane's query is finished.  For every call of
at most 524 288 queries the run is at most 64 and the first hand-out takes all of it: no lane is ever refilled.  Here the refill
runs: lbvh_debug_ray_waves caps the grid so that 1 500 queries make runs of 215 .. 1 501 (part 2), and calls of more than a
million queries make runs of 130 as shipped (part 3).  Part 4 takes the overlap queries' scan over its tile borders, through more
than 1024 tiles and past a running total of 2^32.

The expectations are the numpy brute forces of the *_reference.py helpers and, for lbvh_trace_rays, the C oracle; the query sets
are the mixed generators of each query's own test module, arranged by `arrange` so that a set holds a block of 135 consecutive
inactive queries, an inactive first and last query and, side by side, active queries whose walks differ greatly in length.
Every GPU comparison is word for word on uint32 views."""
import ctypes as C
import os

import numpy as np
import pytest

import k_closest_reference as KC
import k_hits_reference as KH
import oracle as O
import overlap_reference as V
import point_reference as PR
import ray_reference as RR
import sweep_reference as SW
import test_crossings as TC
import test_overlap_queries as TO
import test_sphere_cast as TS
from query_support import (H, library_boxes, mixed_queries, mixed_rays_of, N, pack, padded_boxes, positions,
                           _random_ray_states, stacked_sheets, words)
from unitysimpleraytracing_amd import layouts as L
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
NAN = F(np.nan)
U32 = np.dtype(np.uint32)
ROW_FILL, WORD_FILL = 0x7FC00000, 0xDEADBEEF
GUARD_BYTES = 4096
KMAX = 32
CAPS = [1, 2, 3, 7]
# queries per wave a capped launch must have: four rounds of 64, so that every lane is refilled.  Cap 7 cannot have them on a set of
# 1 500 (ceil(1500 / 7) = 215, three full rounds and a fourth of 23): it is there for its seven uneven runs, and is held to 3 * 64.
MIN_RUN = {1: 4 * 64, 2: 4 * 64, 3: 4 * 64, 7: 3 * 64}
BLOCK = (700, 835)                      # (a): 135 consecutive inactive queries
PLANT = (100, 164)                      # (d): 64 queries, long and short walks in turn
LONG_COUNT = 2 * 8192 * 64 + 8192 + 77  # part 3: 1 056 845 queries, runs of 130 on 8192 waves
PART = 524288                           # ... and the largest call without a refill


def run_of(count, waves):
    """the run of a launch as the kernels compute it: waves = min(cap or 8192, ceil(count / 64))"""
    return max(-(-count // waves), 32)


def waves_of(count, cap=0):
    return min(cap or 8192, -(-count // 64))


# ---- CPU side: the arrangement of a query set --------------------------------------------------------------------------------

def scene_box(a, b, c):
    pts = np.concatenate([a, b, c])
    return pts.min(axis=0).astype(np.float64), pts.max(axis=0).astype(np.float64)


def _deaden_rays(q, idx, box):
    """empty range, NaN t_min, NaN t_max, t_max below t_min"""
    form = np.arange(len(idx)) % 4
    q["t_min"][idx] = np.where(form == 1, NAN, F(0.5))
    q["t_max"][idx] = np.select([form == 0, form == 2, form == 3], [F(0.5), NAN, F(-1.0)], INF).astype(F)


def _deaden_points(q, idx, box):
    """radius 0, negative, NaN; a NaN coordinate"""
    form = np.arange(len(idx)) % 4
    q["max_dist2"][idx] = np.select([form == 0, form == 1, form == 2], [F(0.0), F(-1.0), NAN], INF).astype(F)
    p = q["p"][idx]
    p[form == 3, 1] = NAN
    q["p"][idx] = p


def _deaden_casts(q, idx, box):
    """radius 0 / negative / NaN, t_max <= 0 / NaN, a zero direction, an infinite direction, a NaN origin"""
    form = np.arange(len(idx)) % 8
    q["radius"][idx] = np.select([form == 0, form == 1, form == 2], [F(0.0), F(-0.5), NAN], q["radius"][idx]).astype(F)
    q["t_max"][idx] = np.select([form == 3, form == 4], [F(-1.0), NAN], q["t_max"][idx]).astype(F)
    d, o = q["dir"][idx], q["origin"][idx]
    d[form == 5] = 0.0
    d[form == 6, 0] = INF
    o[form == 7, 2] = NAN
    q["dir"][idx], q["origin"][idx] = d, o


def _deaden_boxes(q, idx, box):
    """inverted on one axis, a NaN bound"""
    form = np.arange(len(idx)) % 4
    lo, hi = q["min"][idx], q["max"][idx]
    for axis in range(3):
        lo[form == axis, axis] = hi[form == axis, axis] + F(1.0)
    hi[form == 3, 0] = NAN
    q["min"][idx], q["max"][idx] = lo, hi


def _deaden_states(q, idx, box):
    q["alive"][idx] = 0


def _deaden_crossing_points(q, idx, box):
    """lbvh_point_crossings has no inactive point; a NaN coordinate is the shortest walk it has: every box missed, parity 0"""
    p = q["p"][idx]
    p[np.arange(len(idx)), np.arange(len(idx)) % 3] = NAN
    q["p"][idx] = p


def _far_and_inside(box, n):
    """n points: even ones on the centre of the scene, odd ones 40 extents away along the diagonal"""
    lo, hi = box
    centre, ext = (lo + hi) / 2.0, (hi - lo).max()
    p = np.tile(centre, (n, 1))
    p[1::2] += 40.0 * ext
    return p.astype(F)


def _plant_rays(q, idx, box):
    """even: through the centre of the scene along its diagonal; odd: from 40 extents away, pointing away from it"""
    q["origin"][idx] = _far_and_inside(box, len(idx))
    q["dir"][idx] = (F(1.0), F(0.75), F(0.5))
    q["t_min"][idx], q["t_max"][idx] = F(0.0), INF


def _plant_points(q, idx, box):
    q["p"][idx] = _far_and_inside(box, len(idx))
    q["max_dist2"][idx] = INF


def _plant_distance(q, idx, box):
    """even: a ball of half the extent at the centre; odd: a ball of a tenth of the extent 40 extents away"""
    ext = (box[1] - box[0]).max()
    q["p"][idx] = _far_and_inside(box, len(idx))
    r = np.where(np.arange(len(idx)) % 2 == 0, 0.5 * ext, 0.1 * ext)
    q["max_dist2"][idx] = (r * r).astype(F)


def _plant_casts(q, idx, box):
    """one active cast of the set aimed at the surface, with a radius of 10 % (even) and 0.5 % (odd) of the extent"""
    ext = (box[1] - box[0]).max()
    act = np.nonzero(SW.active(q) & np.isinf(q["t_max"]))[0]
    q[idx] = q[act[np.arange(len(idx)) % len(act)]]
    q["radius"][idx] = np.where(np.arange(len(idx)) % 2 == 0, 0.1 * ext, 0.005 * ext).astype(F)


def _plant_boxes(q, idx, box):
    """even: a box around the whole scene; odd: a box 40 extents away"""
    lo, hi = box
    ext = (hi - lo).max()
    shift = np.where(np.arange(len(idx)) % 2 == 0, 0.0, 40.0 * ext)[:, None]
    q["min"][idx] = (lo - 1.0 + shift).astype(F)
    q["max"][idx] = (hi + 1.0 + shift).astype(F)


def _plant_states(q, idx, box):
    q["origin"][idx] = _far_and_inside(box, len(idx))
    q["dir"][idx] = (F(0.8), F(0.6), F(0.0))
    q["alive"][idx] = 1


def _outside(p, box):
    lo, hi = box
    ext = (hi - lo).max()
    with np.errstate(invalid="ignore"):
        return ((p < lo - ext) | (p > hi + ext)).any(axis=1)


def _inside(p, box):
    with np.errstate(invalid="ignore"):
        return ((p >= box[0]) & (p <= box[1])).all(axis=1)


# kind -> (inactive forms, planted pairs, active rule, the short walks of (d), the long walks of (d))
KINDS = {
    "rays": (_deaden_rays, _plant_rays, RR.active, lambda q, box: _outside(q["origin"], box), lambda q, box: _inside(q["origin"], box)),
    "points": (_deaden_points, _plant_points, lambda q: PR.active(q) & ~np.isnan(q["p"]).any(axis=1),
               lambda q, box: _inside(q["p"], box), lambda q, box: _outside(q["p"], box)),
    "distance": (_deaden_points, _plant_distance, lambda q: PR.active(q) & ~np.isnan(q["p"]).any(axis=1),
                 lambda q, box: _outside(q["p"], box), lambda q, box: _inside(q["p"], box)),
    "casts": (_deaden_casts, _plant_casts, SW.active,
              lambda q, box: q["radius"] <= F(0.00501 * (box[1] - box[0]).max()), lambda q, box: q["radius"] >= F(0.0999 * (box[1] - box[0]).max())),
    "boxes": (_deaden_boxes, _plant_boxes, V.box_active,
              lambda q, box: _outside(q["min"][:, :3], box), lambda q, box: (q["min"][:, :3] <= box[0]).all(axis=1) & (q["max"][:, :3] >= box[1]).all(axis=1)),
    "states": (_deaden_states, _plant_states, lambda q: q["alive"] != 0,
               lambda q, box: _outside(q["origin"], box), lambda q, box: _inside(q["origin"], box)),
    "crossing_points": (_deaden_crossing_points, _plant_points, lambda q: ~np.isnan(q["p"]).any(axis=1),
                        lambda q, box: _outside(q["p"], box), lambda q, box: _inside(q["p"], box)),
}


def arrange(kind, queries, box):
    """the generator's set with (a) BLOCK, (b) query 0 and (c) the last query made inactive, in every inactive form of the kind in
    turn, and (d) PLANT: long and short walks in turn.  Everything else stays as the generator made it."""
    deaden, plant = KINDS[kind][:2]
    q = queries.copy()
    plant(q, np.arange(*PLANT), box)
    deaden(q, np.concatenate([[0, len(q) - 1], np.arange(*BLOCK)]), box)
    return q


def check_arranged(kind, q, box, caps=CAPS):
    """(a) .. (d) of a set, and that every capped launch has MIN_RUN queries per wave"""
    act = KINDS[kind][2](q)
    short, long_ = KINDS[kind][3](q, box) & act, KINDS[kind][4](q, box) & act
    assert len(q) in (1500, 1501)
    dead = ~act
    runs = np.diff(np.nonzero(np.diff(np.concatenate([[0], dead.astype(np.int8), [0]])))[0])[::2]
    assert runs.max() >= 130                                                          # (a)
    assert dead[0] and dead[-1]                                                       # (b), (c)
    pairs = (short[:-1] & long_[1:]) | (long_[:-1] & short[1:])
    assert pairs.sum() >= 32                                                          # (d)
    assert 0.3 * len(q) < act.sum() < len(q) - 132
    for cap in caps:
        waves = waves_of(len(q), cap)
        assert waves == cap and -(-len(q) // waves) >= MIN_RUN.get(cap, 4 * 64)
    return act


def torus():
    return scenes.tiled_torus(nu=16, nv=10, grid=2)


_SETS = {}


def query_set(name, a, b, c, lo, hi):
    """the arranged set `name` over the triangles a, b, c with the boxes lo, hi (cached per name: the GPU tests pass the library's
    boxes, which equal the padded ones of the CPU tests on these scenes)"""
    if name in _SETS:
        return _SETS[name]
    box = scene_box(a, b, c)
    if name == "rays":
        q = TC.mixed_rays(a, b, c, 1500, 21, lambda r: RR.reference(r, a, b, c, lo, hi).records)[0]
        kind = "rays"
    elif name in ("khits_torus", "khits_sheets"):
        q = mixed_rays_of("sheets" if name == "khits_sheets" else "torus", a, b, c, lo, hi)
        kind = "rays"
    elif name == "points":
        q = mixed_queries(a, b, c, lo, hi, 1501, 22)[0]
        kind = "points"
    elif name == "kclosest":
        q = mixed_queries(a, b, c, lo, hi, 1500, 23)[0]
        kind = "points"
    elif name == "casts":
        q = TS.aimed_casts(a, b, c, 1501, np.random.default_rng(24))
        kind = "casts"
    elif name == "crossing_points":
        q = np.concatenate([TC._point_buffer(a, b, c, np.random.default_rng(s)) for s in (25, 26)])[:1500]
        kind = "crossing_points"
    elif name == "boxes":
        q = TO.box_queries(lo, hi, 1501, 27)
        kind = "boxes"
    elif name == "distance":
        q = TO.distance_queries(lo, hi, 1500, 28)
        kind = "distance"
    else:
        assert name == "states"
        q = _random_ray_states(pack(a, b, c), 1501, 29)
        q["alive"] = (np.random.default_rng(30).random(1501) < 0.5).astype(np.uint32)      # about half the states are dead
        kind = "states"
    q = arrange(kind, q, box)
    _SETS[name] = (kind, q, check_arranged(kind, q, box))
    return _SETS[name]


SET_NAMES = ["rays", "khits_torus", "khits_sheets", "points", "kclosest", "casts", "crossing_points", "boxes", "distance", "states"]


@pytest.mark.parametrize("name", SET_NAMES)
def test_every_arranged_set_holds_the_inactive_block_the_ends_and_the_mixed_neighbours(name):
    a, b, c = stacked_sheets() if name == "khits_sheets" else positions(torus())
    lo, hi = padded_boxes(a, b, c)
    kind, q, act = query_set(name, a, b, c, lo, hi)
    assert not act[BLOCK[0]:BLOCK[1]].any() and act[PLANT[0]:PLANT[1]].all()
    if name == "states":
        assert 0.4 < act.mean() < 0.6


def test_check_arranged_refuses_a_set_without_the_block_or_with_short_runs():
    a, b, c = positions(torus())
    lo, hi = padded_boxes(a, b, c)
    box = scene_box(a, b, c)
    kind, q, _ = query_set("points", a, b, c, lo, hi)
    plain = q.copy()
    plain["max_dist2"][BLOCK[0]:BLOCK[1]:2] = INF
    plain["p"][BLOCK[0]:BLOCK[1]:2] = plain["p"][PLANT[0]]
    with pytest.raises(AssertionError):
        check_arranged(kind, plain, box)
    with pytest.raises(AssertionError):
        check_arranged(kind, q, box, caps=[8])                         # ceil(1501 / 8) = 188 < 256
    for count in (LONG_COUNT,):
        assert waves_of(count) == 8192 and run_of(count, 8192) == 130 and 8192 * 130 > count > 8191 * 130 - 130 * 63


def test_partition_arithmetic_of_the_small_counts():
    """the counts of the partition-edge test reach the floor of 32 per run and the early return of the trailing waves"""
    for count, waves, run, used in [(1, 1, 32, 1), (31, 1, 32, 1), (32, 1, 32, 1), (33, 1, 33, 1), (63, 1, 63, 1), (64, 1, 64, 1),
                                    (65, 2, 33, 2), (127, 2, 64, 2), (129, 3, 43, 3)]:
        assert waves_of(count) == waves and run_of(count, waves) == run
        assert sum(1 for w in range(waves) if w * run < count) == used


# ---- CPU side: the palette of the scan test ------------------------------------------------------------------------------------

SCAN_COUNT = 1024 * 1024 + 3 * 1024 + 5
SCAN_CAPACITY = 1 << 20


def scan_palette(lo, hi):
    """8 boxes over a scene with the triangle boxes lo, hi: 0 the whole scene, 1 / 2 the half below the centre in x / in y, 3 an
    inverted box, 4 a box far outside, 5 / 6 / 7 the octant above the centre, a slab around the centre's z, a small box at the centre"""
    slo, shi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    mid, ext = (slo + shi) / 2.0, shi - slo
    blo, bhi = np.tile(slo - 1.0, (8, 1)), np.tile(shi + 1.0, (8, 1))
    bhi[1, 0] = mid[0]
    bhi[2, 1] = mid[1]
    blo[3], bhi[3] = mid + 1.0, mid - 1.0
    blo[4], bhi[4] = shi + 10.0 * ext, shi + 11.0 * ext
    blo[5] = mid
    blo[6, 2], bhi[6, 2] = mid[2] - 0.05 * ext[2], mid[2] + 0.05 * ext[2]
    blo[7], bhi[7] = mid - 0.1 * ext, mid + 0.1 * ext
    return V.make_boxes(blo.astype(F), bhi.astype(F))


def scan_layout(counts):
    """which palette entry each of the SCAN_COUNT queries is: the halves 1, 2 in turn until they fill the first 2^20 words, then
    the whole scene until the end minus 2000, then 3 .. 7 in turn.  -> (entries, offsets uint64[SCAN_COUNT + 1])"""
    head = 1
    while (counts[1] * ((head + 1) // 2) + counts[2] * (head // 2)) < SCAN_CAPACITY + counts[1]:
        head += 1
    pick = np.zeros(SCAN_COUNT, dtype=np.int64)
    pick[:head] = 1 + np.arange(head) % 2
    pick[-2000:] = 3 + np.arange(2000) % 5
    offsets = np.zeros(SCAN_COUNT + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64)[pick], out=offsets[1:])
    return pick, offsets


def check_scan_layout(pick, offsets, counts):
    """more than 1024 tiles of 1024; the total passes 2^32 before the last 2000 queries; the words below the capacity come from
    entries 1 and 2 only and every query from the pass on is another entry, with a non-empty one among them"""
    assert len(pick) // 1024 + 1 > 1024 + 2
    first_beyond = int(np.searchsorted(offsets, np.uint64(1) << np.uint64(32), side="right")) - 1      # the query whose segment takes the total past 2^32
    assert 0 < first_beyond <= SCAN_COUNT - 2000 and int(offsets[-1]) > (1 << 32)
    below = np.nonzero(offsets[:-1] < SCAN_CAPACITY)[0]
    assert set(pick[below].tolist()) == {1, 2} and int(offsets[below[-1] + 1]) >= SCAN_CAPACITY
    after = pick[first_beyond:]
    assert not (set(after.tolist()) & {1, 2}) and (np.asarray(counts)[after] > 0).sum() > 1000
    assert offsets.dtype == np.uint64 and (np.diff(offsets.astype(np.float64)) >= 0).all()


def test_scan_palette_and_layout():
    pos = np.load(os.path.join(ROOT, "tests", "golden", "cfg1_4096.npz"))["positions"]
    a, b, c = (np.ascontiguousarray(pos[:, k], dtype=F) for k in range(3))
    lo, hi = padded_boxes(a, b, c)
    palette = scan_palette(lo, hi)
    off, tris = V.box_overlaps(palette, lo, hi)
    counts = np.diff(off).astype(np.int64)
    assert counts[0] == 4096 and counts[3] == 0 and counts[4] == 0 and (counts[[1, 2, 5, 6, 7]] > 0).all()
    assert len(set(counts.tolist())) >= 6                                # different candidate sets
    pick, offsets = scan_layout(counts)
    check_scan_layout(pick, offsets, counts)
    # the cumsum is exact in uint64 where float64 or uint32 would not be
    assert int(offsets[-1]) == int(sum(int(counts[k]) * int(n) for k, n in enumerate(np.bincount(pick, minlength=8))))
    assert int(offsets[-1]) != int(offsets[-1].astype(np.uint32))


# ---- GPU side --------------------------------------------------------------------------------------------------------------

class Out:
    """an output of `n` records of `width` items with a guard of 4096 bytes behind them, prefilled before every call"""

    def __init__(self, ctx, dtype, n, width, fill):
        self.dtype, self.n, self.width, self.fill = np.dtype(dtype), n, width, fill
        self.buf = H().DataBuffer(ctx, n * width + GUARD_BYTES // self.dtype.itemsize, dtype)

    def prefill(self):
        self.buf.fill_u32(self.fill, mirror=False)

    def at(self, first):
        return C.c_void_p(self.buf.device.value + first * self.width * self.dtype.itemsize)

    def read(self, written=True):
        """(n, width) records; the guard, and with written=False every word, must still hold the fill"""
        got = self.buf.get_data()
        assert (words(got[self.n * self.width:]) == self.fill).all(), "guard overwritten"
        rec = got[: self.n * self.width].reshape(self.n, self.width).copy()
        if not written:
            assert (words(rec) == self.fill).all()
        return rec

    def dispose(self):
        self.buf.dispose()


class Op:
    """one entry point on one query set: fn(lib, handle, d_in, count, scene, *d_outs) and what each output must hold"""

    def __init__(self, name, set_name, outs, fn, expect, rays_per_active=1, walkers=(1,)):
        self.name, self.set_name, self.outs, self.fn, self.expect = name, set_name, outs, fn, expect
        self.rays_per_active, self.walkers = rays_per_active, walkers


def _upload(ctx, q):
    buf = H().DataBuffer(ctx, len(q), q.dtype)
    buf.local[:] = q
    buf.sync()
    return buf


def issue(ctx, drawer, op, d_in, in_size, outs, first, count):
    s = drawer.container.scene()
    ptrs = [o.at(first) if o is not None else None for o in outs]
    N().check(ctx.handle, op.fn(N().lib, ctx.handle, C.c_void_p(d_in.device.value + first * in_size), count, C.byref(s), *ptrs))


def run(ctx, drawer, op, d_in, q, outs, parts=None):
    """one call over the whole buffer, or one call per part; every output prefilled -> the records"""
    for o in outs:
        if o is not None:
            o.prefill()
    for first, count in (parts or [(0, len(q))]):
        issue(ctx, drawer, op, d_in, q.dtype.itemsize, outs, first, count)
    return [o.read() if o is not None else None for o in outs]


def assert_words(got, want, what):
    gw, ww = words(got).reshape(len(got), -1), words(want).reshape(len(want), -1)
    assert gw.shape == ww.shape, (what, gw.shape, ww.shape)
    bad = np.nonzero((gw != ww).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], want[bad[:3]])


class hooks:
    """the debug hooks of a test, restored on the way out whatever happened"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        return self

    def set(self, waves=0, split=16, walker=1, stats=None):
        h, lib = self.ctx.handle, N().lib
        N().check(h, lib.lbvh_debug_ray_waves(h, waves))
        N().check(h, lib.lbvh_debug_ray_stack_split(h, split))
        N().check(h, lib.lbvh_debug_ray_walker(h, walker))
        N().check(h, lib.lbvh_ray_stats_target(h, stats))

    def __exit__(self, *exc):
        self.set()
        return False


_SCENES = {}


def scene_case(ctx, name):
    """(a, b, c, the library's boxes, drawer, the oracle's build) of "torus" or "sheets"; the derived scene is this one's again"""
    if name not in _SCENES:
        tris = torus() if name == "torus" else pack(*stacked_sheets())
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        a, b, c = positions(tris)
        lo, hi = library_boxes(d)
        plo, phi = padded_boxes(a, b, c)
        assert (words(lo) == words(plo)).all() and (words(hi) == words(phi)).all()      # the CPU tests' sets are these sets
        _SCENES[name] = (a, b, c, lo, hi, d, tris)
    _SCENES[name][5].build_fast_scene()
    return _SCENES[name]


DIRS32 = np.random.default_rng(31).normal(size=(32, 3)).astype(F)
DIRS32[5], DIRS32[6] = (0.0, 0.0, -2.0), (3.0, 0.0, 0.0)
_REFS = {}


def reference_of(key, make):
    if key not in _REFS:
        _REFS[key] = make()
    return _REFS[key]


def _plain(name):
    return lambda lib, h, d_in, count, s, out: getattr(lib, name)(h, d_in, count, s, out)


def _with_k(name, k):
    return lambda lib, h, d_in, count, s, rows, found: getattr(lib, name)(h, d_in, count, k, s, rows, found)


def _crossings(dirs):
    d = np.ascontiguousarray(dirs, dtype=F)
    return lambda lib, h, d_in, count, s, out: lib.lbvh_point_crossings(h, d_in, count, d.ctypes.data_as(C.POINTER(C.c_float)), len(d), s, out)


def _trace_rays(lib, h, d_in, count, s, out):
    return lib.lbvh_trace_rays(h, d_in, count, 1e-3, s, out)


def ops_of(scene, k_values=(1, 5, 32)):
    """every walker entry point but the overlap queries, with the brute force of its own query set"""
    a, b, c, lo, hi, d, tris = scene

    def ref(name, make):
        return reference_of(name, lambda: make(query_set(name, a, b, c, lo, hi)[1]))

    ray = lambda: ref("rays", lambda q: RR.reference(q, a, b, c, lo, hi))
    pts = lambda: ref("points", lambda q: PR.reference(q, a, b, c, lo, hi))
    cast = lambda: ref("casts", lambda q: SW.reference(q, a, b, c, lo, hi))
    knn = lambda: ref("kclosest", lambda q: KC.reference(q, a, b, c, lo, hi, KMAX))
    khit = lambda: ref("khits_torus", lambda q: KH.reference(q, a, b, c, lo, hi, KMAX))
    hit, cp, three = (L.HIT, 1, ROW_FILL), (L.CLOSEST_POINT, 1, ROW_FILL), (0, 1, 2)
    word = (U32, 1, WORD_FILL)
    ops = [
        Op("trace_closest", "rays", [hit], _plain("lbvh_trace_closest"), lambda: [ray().records], walkers=three),
        Op("trace_occluded", "rays", [word], _plain("lbvh_trace_occluded"), lambda: [ray().flags.astype(np.uint32)], walkers=three),
        Op("count_hits", "rays", [word], _plain("lbvh_count_hits"), lambda: [ray().counts.astype(np.uint32)], walkers=three),
        Op("trace_rays", "states", [hit], _trace_rays,
           lambda: [reference_of("states", lambda: O.trace_rays(O.Built(tris, capacity=d.container.capacity, threads=8),
                                                                query_set("states", a, b, c, lo, hi)[1], 1e-3, threads=8))], walkers=three),
        Op("closest_point_query", "points", [cp], _plain("lbvh_closest_point_query"), lambda: [pts().records]),
        Op("within_distance", "points", [word], _plain("lbvh_within_distance"), lambda: [pts().flags.astype(np.uint32)]),
        Op("sphere_cast", "casts", [hit], _plain("lbvh_sphere_cast"), lambda: [cast().records]),
        Op("sphere_cast_any", "casts", [word], _plain("lbvh_sphere_cast_any"), lambda: [cast().flags.astype(np.uint32)]),
    ]
    for k in k_values:
        ops.append(Op(f"k_closest_points[{k}]", "kclosest", [(L.CLOSEST_POINT, k, ROW_FILL), word], _with_k("lbvh_k_closest_points", k),
                      lambda k=k: [KC.truncate(knn(), k).records, KC.truncate(knn(), k).found.astype(np.uint32)]))
        ops.append(Op(f"trace_k_closest[{k}]", "khits_torus", [(L.HIT, k, ROW_FILL), word], _with_k("lbvh_trace_k_closest", k),
                      lambda k=k: [KH.truncate(khit(), k).records, KH.truncate(khit(), k).found.astype(np.uint32)]))
    for n_dirs in (1, 32) if k_values == (1, 5, 32) else (3,):
        dirs = DIRS32[:n_dirs]
        ops.append(Op(f"point_crossings[{n_dirs}]", "crossing_points", [word], _crossings(dirs),
                      lambda dirs=dirs, n_dirs=n_dirs: [reference_of(("crossings", n_dirs), lambda: RR.parity_words(RR.reference(
                          RR.crossing_rays(query_set("crossing_points", a, b, c, lo, hi)[1]["p"], dirs), a, b, c, lo, hi).counts, n_dirs))],
                      rays_per_active=n_dirs))
    return ops


def sheets_ops(scene):
    a, b, c, lo, hi, d, tris = scene
    khit = lambda: reference_of("khits_sheets", lambda: KH.reference(query_set("khits_sheets", a, b, c, lo, hi)[1], a, b, c, lo, hi, KMAX))
    return [Op(f"trace_k_closest[{k}]", "khits_sheets", [(L.HIT, k, ROW_FILL), (U32, 1, WORD_FILL)], _with_k("lbvh_trace_k_closest", k),
               lambda k=k: [KH.truncate(khit(), k).records, KH.truncate(khit(), k).found.astype(np.uint32)]) for k in (1, 5, 32)]


OP_NAMES = ["trace_closest", "trace_occluded", "count_hits", "trace_rays", "closest_point_query", "within_distance", "sphere_cast",
            "sphere_cast_any", "k_closest_points[1]", "trace_k_closest[1]", "k_closest_points[5]", "trace_k_closest[5]",
            "k_closest_points[32]", "trace_k_closest[32]", "point_crossings[1]", "point_crossings[32]", "sheets:trace_k_closest[1]",
            "sheets:trace_k_closest[5]", "sheets:trace_k_closest[32]"]


def expected_rays(op, kind, q, act):
    """what lbvh_ray_stats_target's `rays` must read after one call: every active query walked once (lbvh_point_crossings walks
    every point, a NaN one too, once per direction)"""
    return (len(q) if kind == "crossing_points" else int(act.sum())) * op.rays_per_active


@pytest.mark.gpu
@pytest.mark.parametrize("op_name", OP_NAMES)
def test_refilled_lanes_give_the_brute_force_on_every_wave_cap(ctx, op_name):
    """caps 1, 2, 3, 7 (runs of 1500 .. 215: every lane refilled at least three times) and cap 1 with one stack entry in LDS,
    on every walker the entry point has; the uncapped call first.  Word for word equal to the brute force, hence to each other."""
    sheets = op_name.startswith("sheets:")
    scene = scene_case(ctx, "sheets" if sheets else "torus")
    a, b, c, lo, hi, d, tris = scene
    op = {o.name: o for o in (sheets_ops(scene) if sheets else ops_of(scene))}[op_name.split(":")[-1]]
    kind, q, act = query_set(op.set_name, a, b, c, lo, hi)
    want = op.expect()
    d_in = _upload(ctx, q)
    outs = [Out(ctx, dt, len(q), width, fill) for dt, width, fill in op.outs]
    stats = H().DataBuffer(ctx, 1, L.RAY_STATS)
    with_found = [True, False] if op.name.startswith("k_closest_points") else [True]
    try:
        with hooks(ctx) as hk:
            for walker in op.walkers:
                for cap, split in [(0, 16)] + [(cap, 16) for cap in CAPS] + [(1, 1)]:
                    for found in with_found:
                        what = (op.name, "walker", walker, "cap", cap, "split", split, "found", found)
                        counted = walker != 0                                  # the binary walk has no counting instantiation
                        stats.fill_u32(0)
                        hk.set(waves=cap, split=split, walker=walker, stats=stats.device if counted else None)
                        if cap:
                            assert -(-len(q) // waves_of(len(q), cap)) >= MIN_RUN[cap]
                        if not found:
                            outs[1].prefill()
                        got = run(ctx, d, op, d_in, q, outs if found else [outs[0], None])
                        if not found:
                            outs[1].read(written=False)                        # d_found == NULL: the counts stay as they were
                        for g, w in zip(got, want if found else want[:1]):
                            assert_words(g, w, what)
                        assert N().lib.lbvh_sync(ctx.handle) == 0, what
                        if counted:
                            assert int(stats.get_data()[0]["rays"]) == expected_rays(op, kind, q, act), what
    finally:
        for buf in [d_in, stats] + [o.buf for o in outs]:
            buf.dispose()


def run_overlap(ctx, d, fn, d_in, count, offsets, tris=None, capacity=0, first=0, in_size=32, offsets_at=0):
    s = d.container.scene()
    N().check(ctx.handle, fn(ctx.handle, C.c_void_p(d_in.device.value + first * in_size), count, C.byref(s),
                             C.c_void_p(offsets.device.value + 8 * offsets_at), tris.device if tris is not None else None, capacity))


def overlap_fn(box):
    return N().lib.lbvh_box_overlaps if box else N().lib.lbvh_gather_within_distance


def overlap_reference_of(box, q, a, b, c, lo, hi):
    return V.box_overlaps(q, lo, hi) if box else V.gather_within_distance(q, a, b, c, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [True, False])
def test_refilled_overlap_walks_give_the_brute_force_lists(ctx, box):
    """count-only and count + fill under every cap: exact offsets, segments equal as sorted sets, `rays` = the active queries
    once per walk, guards untouched"""
    a, b, c, lo, hi, d, tris = scene_case(ctx, "torus")
    name = "boxes" if box else "distance"
    kind, q, act = query_set(name, a, b, c, lo, hi)
    ro, rt = reference_of(name, lambda: overlap_reference_of(box, q, a, b, c, lo, hi))
    total = int(ro[-1])
    assert total > 20000 and (np.diff(ro.astype(np.int64)) == 0).sum() > 135
    d_in = _upload(ctx, q)
    offsets = Out(ctx, np.uint64, len(q) + 1, 1, WORD_FILL)
    lists = Out(ctx, U32, total, 1, 0xABABABAB)
    stats = H().DataBuffer(ctx, 1, L.RAY_STATS)
    try:
        with hooks(ctx) as hk:
            for cap, split in [(0, 16)] + [(cap, 16) for cap in CAPS] + [(1, 1)]:
                for fill in (False, True):
                    stats.fill_u32(0)
                    hk.set(waves=cap, split=split, stats=stats.device)
                    offsets.prefill()
                    lists.prefill()
                    run_overlap(ctx, d, overlap_fn(box), d_in, len(q), offsets.buf, lists.buf if fill else None, total if fill else 0,
                                in_size=q.dtype.itemsize)
                    go = offsets.read()[:, 0]
                    assert (go == ro).all(), (cap, split, fill, np.nonzero(go != ro)[0][:10])
                    gt = lists.read(written=fill)[:, 0]
                    if fill:
                        gs = V.sort_segments(go, gt)
                        assert (gs == rt).all(), (cap, split, np.nonzero(gs != rt)[0][:10])
                    assert N().lib.lbvh_sync(ctx.handle) == 0
                    assert int(stats.get_data()[0]["rays"]) == int(act.sum()) * (2 if fill else 1), (cap, split, fill)
    finally:
        for buf in (d_in, stats, offsets.buf, lists.buf):
            buf.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 31, 32, 33, 63, 64, 65, 127, 129])
def test_partition_edges_without_the_hook(ctx, count):
    """the first `count` queries of a point, a k = 5 and a cast set, as shipped: the floor of 32 queries per run, trailing waves
    without a query.  The sets start with an inactive query."""
    scene = scene_case(ctx, "torus")
    a, b, c, lo, hi, d, tris = scene
    ops = {o.name: o for o in ops_of(scene)}
    for name in ("closest_point_query", "k_closest_points[5]", "sphere_cast"):
        op = ops[name]
        kind, q, act = query_set(op.set_name, a, b, c, lo, hi)
        q = q[:count].copy()
        d_in = _upload(ctx, q)
        outs = [Out(ctx, dt, count, width, fill) for dt, width, fill in op.outs]
        try:
            for g, w in zip(run(ctx, d, op, d_in, q, outs), op.expect()):
                assert_words(g, w[:count], (name, count))
            assert N().lib.lbvh_sync(ctx.handle) == 0
        finally:
            for buf in [d_in] + [o.buf for o in outs]:
                buf.dispose()


# ---- part 3: the runs of 130 of a call of more than a million queries, as shipped ---------------------------------------------------

LONG_PARTS = [(0, PART), (PART, PART), (2 * PART, LONG_COUNT - 2 * PART)]
LONG_OPS = ["trace_closest", "trace_occluded", "count_hits", "trace_rays", "closest_point_query", "within_distance", "sphere_cast",
            "sphere_cast_any", "k_closest_points[4]", "trace_k_closest[4]", "point_crossings[3]"]


def long_indices():
    """256 fixed indices: the three queries around the run borders j * 130 of several waves, the last query, and a spread"""
    j = np.array([1, 2, 3, 63, 64, 65, 1000, 4095, 4096, 8000, 8128, 8129], dtype=np.int64)
    edge = np.concatenate([j * 130 - 1, j * 130, j * 130 + 1, [LONG_COUNT - 1, 0]])
    edge = edge[edge < LONG_COUNT]
    rest = np.random.default_rng(32).choice(LONG_COUNT, 256 - len(edge), replace=False)
    return np.unique(np.concatenate([edge, rest]))


def test_long_run_arithmetic():
    assert waves_of(LONG_COUNT) == 8192 and run_of(LONG_COUNT, 8192) == 130
    assert 0 < LONG_COUNT - 8129 * 130 < 130                              # wave 8129 has the short last run, 62 waves none at all
    assert all(count <= PART and run_of(count, waves_of(count)) <= 64 for _, count in LONG_PARTS)      # the parts refill nothing
    assert sum(count for _, count in LONG_PARTS) == LONG_COUNT
    idx = long_indices()
    assert 250 <= len(idx) <= 256 and LONG_COUNT - 1 in idx and {129, 130, 131, 8129 * 130}.issubset(idx.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("op_name", LONG_OPS)
def test_runs_of_130_equal_three_calls_without_refill_and_the_brute_force(ctx, op_name):
    """LONG_COUNT queries, the arranged 1 500 / 1 501 of part 2 repeated, in one call and in three calls of at most 524 288:
    word for word the same, and equal to the brute force at long_indices() (query i is query i mod 1 500 / 1 501 of the set)"""
    scene = scene_case(ctx, "torus")
    a, b, c, lo, hi, d, tris = scene
    op = {o.name: o for o in ops_of(scene, k_values=(4,))}[op_name]
    kind, q0, act0 = query_set(op.set_name, a, b, c, lo, hi)
    q = np.resize(q0, LONG_COUNT)
    act = np.resize(act0, LONG_COUNT)
    want = op.expect()
    d_in = _upload(ctx, q)
    outs = [Out(ctx, dt, LONG_COUNT, width, fill) for dt, width, fill in op.outs]
    stats = H().DataBuffer(ctx, 1, L.RAY_STATS)
    idx = long_indices()
    try:
        with hooks(ctx) as hk:
            stats.fill_u32(0)
            hk.set(stats=stats.device)
            whole = run(ctx, d, op, d_in, q, outs)
            assert N().lib.lbvh_sync(ctx.handle) == 0
            assert int(stats.get_data()[0]["rays"]) == expected_rays(op, kind, q, act)
            hk.set()
            parts = run(ctx, d, op, d_in, q, outs, parts=LONG_PARTS)
            assert N().lib.lbvh_sync(ctx.handle) == 0
        for g, p, w in zip(whole, parts, want):
            assert_words(g, p, (op_name, "one call against three"))
            assert_words(g[idx], w[idx % len(q0)], (op_name, "brute force at the fixed indices"))
    finally:
        for buf in [d_in, stats] + [o.buf for o in outs]:
            buf.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("box", [True, False])
def test_overlap_runs_of_130_equal_three_calls_without_refill_and_the_brute_force(ctx, box):
    a, b, c, lo, hi, d, tris = scene_case(ctx, "torus")
    name = "boxes" if box else "distance"
    kind, q0, act0 = query_set(name, a, b, c, lo, hi)
    ro, rt = reference_of(name, lambda: overlap_reference_of(box, q0, a, b, c, lo, hi))
    n0 = np.diff(ro).astype(np.uint64)
    q = np.resize(q0, LONG_COUNT)
    counts = np.resize(n0, LONG_COUNT)
    want = np.zeros(LONG_COUNT + 1, dtype=np.uint64)
    np.cumsum(counts, out=want[1:])
    total = int(want[-1])
    d_in = _upload(ctx, q)
    offsets = Out(ctx, np.uint64, LONG_COUNT + 1, 1, WORD_FILL)
    lists = Out(ctx, U32, total, 1, 0xABABABAB)
    fn = overlap_fn(box)
    try:
        for fill in (False, True):
            offsets.prefill()
            lists.prefill()
            run_overlap(ctx, d, fn, d_in, LONG_COUNT, offsets.buf, lists.buf if fill else None, total if fill else 0, in_size=q.dtype.itemsize)
            go = offsets.read()[:, 0]
            assert (go == want).all(), (fill, np.nonzero(go != want)[0][:10])
            whole = lists.read(written=fill)[:, 0]
        assert N().lib.lbvh_sync(ctx.handle) == 0
        # three calls, each part's list where the whole call has it
        part_lists = np.empty(total, dtype=np.uint32)
        part_off = H().DataBuffer(ctx, PART + 1, np.uint64)
        part_tris = H().DataBuffer(ctx, int(max(want[f + n] - want[f] for f, n in LONG_PARTS)), np.uint32)
        for first, n in LONG_PARTS:
            base, size = int(want[first]), int(want[first + n] - want[first])
            run_overlap(ctx, d, fn, d_in, n, part_off, part_tris, size, first=first, in_size=q.dtype.itemsize)
            assert (part_off.get_data()[: n + 1] == want[first:first + n + 1] - want[first]).all()
            part_lists[base:base + size] = part_tris.get_data()[:size]
        part_off.dispose()
        part_tris.dispose()
        if not (whole == part_lists).all():                                # the order inside a segment is not part of the contract
            assert (V.sort_segments(want, whole) == V.sort_segments(want, part_lists)).all()
        for i in long_indices():
            seg = np.sort(whole[int(want[i]):int(want[i + 1])])
            k = i % len(q0)
            assert (seg == rt[int(ro[k]):int(ro[k + 1])]).all(), i
    finally:
        for buf in (d_in, offsets.buf, lists.buf):
            buf.dispose()


# ---- part 4: the scan ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("box", [True, False])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 1020, 1023, 1024, 1025, 2047, 2048, 2049, 4097])
def test_scan_tile_borders_and_both_alignments_of_the_offsets(ctx, count, box):
    """offsets[0 .. count] = the exclusive cumsum of the brute-force counts, with d_offsets 16-byte aligned and 8 bytes past that
    (the offsets then leave one 8-byte store at a time); the 8 bytes behind offsets[count] stay as they were"""
    a, b, c, lo, hi, d, tris = scene_case(ctx, "torus")
    name = "boxes" if box else "distance"
    kind, q0, act0 = query_set(name, a, b, c, lo, hi)
    ro, rt = reference_of(name, lambda: overlap_reference_of(box, q0, a, b, c, lo, hi))
    q = np.resize(q0, count)
    want = np.zeros(count + 1, dtype=np.uint64)
    np.cumsum(np.resize(np.diff(ro).astype(np.uint64), count), out=want[1:])
    d_in = _upload(ctx, q)
    offsets = H().DataBuffer(ctx, count + 4, np.uint64)
    assert offsets.device.value % 16 == 0
    try:
        for shift in (0, 1):
            offsets.fill_u32(WORD_FILL, mirror=False)
            run_overlap(ctx, d, overlap_fn(box), d_in, count, offsets, offsets_at=shift, in_size=q.dtype.itemsize)
            got = offsets.get_data().copy()
            assert (got[shift:shift + count + 1] == want).all(), (shift, np.nonzero(got[shift:shift + count + 1] != want)[0][:10])
            assert (words(got[:shift]) == WORD_FILL).all() and (words(got[shift + count + 1:]) == WORD_FILL).all(), shift
        assert N().lib.lbvh_sync(ctx.handle) == 0
    finally:
        d_in.dispose()
        offsets.dispose()


@pytest.mark.gpu
def test_scan_over_more_than_1024_tiles_and_a_total_beyond_two_to_the_32(ctx):
    """SCAN_COUNT box queries from scan_palette over the 4096 triangles of cfg1: 1028 tiles (the carry loop of the tile-sum scan
    runs twice), a total of 4.3e9.  Count-only: every offset.  Then a fill with a capacity of 2^20 words: the segments below it
    are the brute force's, everything from the capacity on is untouched — a position cut to 32 bits would land there or, for
    the queries after the total has passed 2^32, on the first segments with the triangles of another box."""
    pos = np.load(os.path.join(ROOT, "tests", "golden", "cfg1_4096.npz"))["positions"]
    tris = pack(*(np.ascontiguousarray(pos[:, k], dtype=F) for k in range(3)))
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    palette = scan_palette(lo, hi)
    po, pt = V.box_overlaps(palette, lo, hi)
    counts = np.diff(po).astype(np.int64)
    pick, want = scan_layout(counts)
    check_scan_layout(pick, want, counts)
    d_in = _upload(ctx, palette[pick])
    offsets = Out(ctx, np.uint64, SCAN_COUNT + 1, 1, WORD_FILL)
    lists_all = H().DataBuffer(ctx, SCAN_CAPACITY + 3 * 4096, np.uint32)      # ... and 12 288 words behind the capacity
    ev = [ctx.event() for _ in range(3)]
    try:
        offsets.prefill()
        ctx.record(ev[0])
        run_overlap(ctx, d, N().lib.lbvh_box_overlaps, d_in, SCAN_COUNT, offsets.buf)
        ctx.record(ev[1])
        go = offsets.read()[:, 0]
        assert (go == want).all(), np.nonzero(go != want)[0][:10]
        offsets.prefill()
        lists_all.fill_u32(0xABABABAB, mirror=False)
        ctx.record(ev[1])
        run_overlap(ctx, d, N().lib.lbvh_box_overlaps, d_in, SCAN_COUNT, offsets.buf, lists_all, SCAN_CAPACITY)
        ctx.record(ev[2])
        go = offsets.read()[:, 0]
        assert (go == want).all()
        got = lists_all.get_data().copy()
        assert N().lib.lbvh_sync(ctx.handle) == 0
        print(f"scan case: count + fill {ctx.elapsed_ms(ev[1], ev[2]):.1f} ms on the device")
        assert (got[SCAN_CAPACITY:] == 0xABABABAB).all()
        fits = int(np.nonzero(want[1:] <= SCAN_CAPACITY)[0][-1])             # the last query whose segment ends below the capacity
        last = int(want[fits + 1])
        assert fits > 500 and SCAN_CAPACITY - last < 4096
        expect = np.concatenate([pt[int(po[k]):int(po[k + 1])] for k in pick[:fits + 1]])
        assert (V.sort_segments(want[:fits + 2], got[:last]) == expect).all()
    finally:
        for e in ev:
            ctx.destroy_event(e)
        for buf in (d_in, offsets.buf, lists_all):
            buf.dispose()
        d.on_destroy()


@pytest.mark.gpu
def test_the_wave_cap_hook_checks_its_argument(ctx):
    h, lib = ctx.handle, N().lib
    try:
        assert lib.lbvh_debug_ray_waves(h, 8193) == -1 and lib.lbvh_debug_ray_waves(None, 1) == -1
        assert lib.lbvh_debug_ray_waves(h, 8192) == 0 and lib.lbvh_debug_ray_waves(h, 1) == 0
    finally:
        assert lib.lbvh_debug_ray_waves(h, 0) == 0
