"""lbvh_region_overlaps_large: lbvh_region_overlaps for few large regions, every region cut into subtree tasks that are walked one per
lane (include/lbvh.h).  The expectation is the brute force of tests/region_reference.py AND lbvh_region_overlaps on the
same buffers: the offsets word for word, d_tris word for word after lbvh_sort_index_segments.  The region sets, the device buffers and
the mixed regions are those of tests/test_region_queries.py.
  CPU  the surface in every host; the host's task_cap rule for every count; a numpy model of the expansion rule on a random four-wide tree
  L1   parity of both modes on grid_80x80, example_object3, cfg1_4096 under forced task caps 4, 5, 8, 64, 4 096, 65 536 and the default
  L2   a generated grid of 10^5 triangles at the default cap       L3  two calls write the same bytes
  L4   the CSR contract: a capacity inside a task and between two tasks, the sentinel tail, capacity == 0 with NULL d_tris
  L5   the walk's frame: wave caps, the stack limit       L6  rejections, a stale scene, a failed allocation, count == 0, the counters
  L7   the live-path list, the smallest scene       L8  lbvh_driver regions <n> <seed> large"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_reference as V
import region_reference as R
import test_region_queries as Q
from query_support import driver_mesh, H, L, library_boxes, N, positions, words
from unitysimpleraytracing_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MODES = [R.TOUCHING, R.CONTAINED]
CAPS = [4, 5, 8, 64, 4096, 65536, 0]                  # 0: the host's choice
COUNTS = [1, 2, 63, 64, 65, 1500]
SLOTS = 1 << 22
LEAF = 0x80000000
POISON = 0x7FC0DEAD


# ---- CPU: the surface ------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_is_declared_in_every_host():
    h = open(os.path.join(ROOT, "include", "lbvh.h")).read()
    assert re.search(r"#define LBVH_REGION_LARGE_MAX_COUNT\s+65536\b", h)
    assert re.search(r"lbvh_status lbvh_region_overlaps_large\(lbvh_context\* ctx, const lbvh_region\* d_regions, size_t count, uint32_t mode,\s+"
                     r"const lbvh_scene\* h_scene,\s+uint64_t\* d_offsets, uint32_t\* d_tris, uint64_t capacity\);", h)
    bounce = h[h.index("CROSS-CALL STATE"):h.index("lbvh_status lbvh_path_bounce(")]
    assert "lbvh_region_overlaps_large" in bounce
    text = h[h.index("lbvh_region_overlaps for FEW, LARGE regions"):h.index("#define LBVH_REGION_LARGE_MAX_COUNT")]
    for must in ("EQUALS lbvh_region_overlaps' d_offsets", "NOT PART OF THE CONTRACT", "write the same bytes", "No kernel\n *   waits for another workgroup",
                 "count > LBVH_REGION_LARGE_MAX_COUNT", "no _any twin", "node_fetches", "When to use which"):
        assert must in text, must
    dbg = open(os.path.join(ROOT, "include", "lbvh_debug.h")).read()
    assert "lbvh_status lbvh_debug_region_task_cap(lbvh_context* ctx, uint32_t cap);" in dbg
    nat = N()
    res, args = nat.SIGNATURES["lbvh_region_overlaps_large"]
    assert res is C.c_int32 and args == nat.SIGNATURES["lbvh_region_overlaps"][1]
    assert callable(nat.lib.lbvh_region_overlaps_large) and callable(nat.lib.lbvh_debug_region_task_cap)
    assert nat.REGION_LARGE_MAX_COUNT == 65536
    cs = open(os.path.join(ROOT, "bindings", "csharp", "LbvhNative.cs")).read()
    assert re.search(r"public static extern int lbvh_region_overlaps_large\(IntPtr ctx, IntPtr \w+, UIntPtr count, uint mode, ref Scene scene,\s+IntPtr \w+,"
                     r"\s+IntPtr \w+,\s+ulong capacity\);", cs)
    rq = re.sub(r"//[^\n]*", "", open(os.path.join(ROOT, "bindings", "csharp", "RegionQueries.cs")).read())
    assert "lbvh_region_overlaps_large(" in rq and "public void RegionOverlapsLarge(" in rq
    assert "void RegionOverlapsLarge(" in open(os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_host.hpp")).read()
    assert hasattr(H().RaytracingMeshDrawer, "region_overlaps_large")
    assert "large" in H().RaytracingMeshDrawer.in_regions.__code__.co_varnames


# ---- CPU: the host's rule ----------------------------------------------------------------------------------------------------------------

def test_the_task_cap_rule_for_every_count():
    """the largest power of two not above min(65 536, 2^22 / count): at least 64, never more than 2^22 slots; the hook's cap stays
    within the same budget"""
    f = N().lib.lbvh_debug_region_task_cap_of
    for count in range(1, 65537):
        cap = f(0, count)
        assert cap & (cap - 1) == 0 and 64 <= cap <= 65536 and cap * count <= SLOTS, (count, cap)
        assert cap == 65536 or 2 * cap * count > SLOTS, (count, cap)
    assert [f(0, c) for c in (1, 64, 65, 128, 129, 65536)] == [65536, 65536, 32768, 32768, 16384, 64]
    assert f(0, 0) == 0 and f(0, 65537) == 0 and f(8, 65537) == 0
    for count in (1, 2, 63, 64, 65, 1500, 65536):
        for forced in (4, 5, 8, 64, 4096, 65536):
            assert f(forced, count) == min(forced, SLOTS // count)


# ---- CPU: a model of the expansion ---------------------------------------------------------------------------------------------------------

def random_wide_tree(rng, n):
    """-> (nodes, root, lo, hi): nodes[i] = up to four (reference, lo, hi) slots, a reference an inner node's index or LEAF | leaf; every
    slot box the exact min / max union of what lies below it; leaves join at every level, so leaf and inner slots sit side by side"""
    lo = rng.uniform(-10.0, 10.0, (n, 3)).astype(F)
    hi = (lo + rng.uniform(0.0, 3.0, (n, 3)).astype(F)).astype(F)
    order = rng.permutation(n)
    level = [(LEAF | int(i), lo[i], hi[i]) for i in order[:n // 2]]
    rest = [(LEAF | int(i), lo[i], hi[i]) for i in order[n // 2:]]
    nodes = []
    while len(level) > 1 or rest or not nodes:
        take = int(rng.integers(0, len(rest) // 2 + 2))
        level, rest = level + rest[:take], rest[take:]
        level = [level[int(i)] for i in rng.permutation(len(level))]
        nxt, i = [], 0
        while i < len(level):
            group = level[i:i + int(rng.integers(2, 5))]
            i += len(group)
            nodes.append(group)
            nxt.append((len(nodes) - 1, np.min([g[1] for g in group], axis=0), np.max([g[2] for g in group], axis=0)))
        level = nxt
    return nodes, level[0][0], lo, hi


def model_expand(nodes, root, passes, cap):
    """the rule of region_expand_kernel; passes[node][slot] = (the slot passes TOUCHING, a leaf slot is a candidate of the mode)"""
    frontier, rounds = [root], 0
    while True:
        inner = [e for e in frontier if not e & LEAF]
        if not inner or len(frontier) + 3 * len(inner) > cap:
            return frontier, rounds
        out = []
        for e in frontier:
            if e & LEAF:
                out.append(e)
                continue
            for (ref, _, _), (touching, candidate) in zip(nodes[e], passes[e]):
                if touching and (candidate if ref & LEAF else True):
                    out.append(ref)
        assert len(out) <= cap
        frontier, rounds = out, rounds + 1


def model_walk(nodes, node, passes, out):
    for (ref, _, _), (touching, candidate) in zip(nodes[node], passes[node]):
        if not touching:
            continue
        if ref & LEAF:
            if candidate:
                out.append(ref & ~LEAF)
        else:
            model_walk(nodes, ref, passes, out)


def test_model_of_the_expansion_rule_on_a_random_wide_tree():
    """for every cap from 4 to 64 the frontier never exceeds the cap, and the accepted leaves together with the candidates below the
    frontier's subtrees are the brute force's list, each index once"""
    rng = np.random.default_rng(30)
    nodes, root, lo, hi = random_wide_tree(rng, 400)
    centre = rng.uniform(-4.0, 4.0, (4, 3))
    regions = np.concatenate([H().obb_planes(centre, Q._rotations(rng, 4), rng.uniform(3.0, 12.0, (4, 3))),
                              R.make_regions(np.full((1, 6, 4), np.nan)), H().aabb_planes([[-20.0] * 3], [[20.0] * 3])])
    ref = R.reference(regions, lo, hi)
    multi_round = 0
    for q, region in enumerate(regions):
        for mode in MODES:
            passes = []
            for group in nodes:
                P, Nn = R.corner_values(region["plane"][None], np.array([g[1] for g in group])[:, None], np.array([g[2] for g in group])[:, None])
                with np.errstate(invalid="ignore"):
                    t, c = (P >= 0).all(axis=1), (Nn >= 0).all(axis=1)
                passes.append([(bool(t[k]), bool(c[k]) if mode == R.CONTAINED else True) for k in range(len(group))])
            want = R.segments(*ref[mode])[q]
            for cap in range(4, 65):
                frontier, rounds = model_expand(nodes, root, passes, cap)
                assert len(frontier) <= cap
                got = [e & ~LEAF for e in frontier if e & LEAF]
                for e in frontier:
                    if not e & LEAF:
                        model_walk(nodes, e, passes, got)
                assert len(set(got)) == len(got) and sorted(got) == want.tolist(), (q, mode, cap)
                multi_round += rounds > 1
    assert len(ref[R.TOUCHING][1]) > 400 and len(ref[R.CONTAINED][1]) > 50 and multi_round > 100


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------

class Large(Q.Regions):
    """Q.Regions with run() on lbvh_region_overlaps_large"""

    def run(self, mode, tris=None, capacity=None, poison=0xDEADBEEF, expect=0):
        self.offsets.fill_u32(poison)
        s = self.drawer.container.scene()
        cap = 0 if tris is None else (tris.size if capacity is None else capacity)
        rc = N().lib.lbvh_region_overlaps_large(self.ctx.handle, self.regions.device, self.count, mode, C.byref(s), self.offsets.device,
                                                tris.device if tris is not None else None, cap)
        assert rc == expect, (rc, N().lib.lbvh_last_error(self.ctx.handle))
        return self.offsets.get_data().copy()

    def lists(self, mode, large=True):
        return self.drawer.in_regions(self.regions, mode, device_sort=True, large=large)


class task_cap:
    """lbvh_debug_region_task_cap for a block of calls"""

    def __init__(self, ctx, cap):
        self.h, self.cap = ctx.handle, cap

    def __enter__(self):
        N().check(self.h, N().lib.lbvh_debug_region_task_cap(self.h, self.cap))

    def __exit__(self, *exc):
        N().check(self.h, N().lib.lbvh_debug_region_task_cap(self.h, 0))


def special_regions(lo, hi):
    """the whole mesh; a half space through its middle; an empty region; a region with a NaN"""
    slo, shi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    mid, ext = (slo + shi) / 2.0, float((shi - slo).max())
    n = np.array([1.0, 0.3, 0.2])
    half = np.tile(np.append(n, -(n * mid).sum()), (1, 6, 1))
    nan = H().aabb_planes([slo - 1.0], [shi + 1.0])["plane"].copy()
    nan[0, 2, 1] = np.nan
    return np.concatenate([H().aabb_planes([slo - 1.0], [shi + 1.0]), R.make_regions(half),
                           H().aabb_planes([shi + ext], [shi + 2.0 * ext]), R.make_regions(nan)])


_SETS = {}


def region_sets(ctx, name):
    """[(label, regions, {mode: (offsets, tris)} of the brute force, {mode: lists of lbvh_region_overlaps})], once per mesh"""
    a, b, c, lo, hi, regions, kind, ref, d = Q.gpu_case(ctx, name)
    if name not in _SETS:
        special = special_regions(lo, hi)
        sref = R.reference(special, lo, hi)
        whole, half, empty, nan = (np.diff(sref[R.TOUCHING][0]).astype(np.int64))
        assert whole == len(lo) and 0.2 * whole < half < 0.8 * whole and empty == 0 and nan == 0
        assert 0 < int(np.diff(sref[R.CONTAINED][0])[1]) < half
        sets = []
        for k, label in enumerate(("whole", "half", "empty", "nan")):
            sets.append((label, special[k:k + 1], {m: (sref[m][0][k:k + 2] - sref[m][0][k], R.segments(*sref[m])[k]) for m in MODES}))
        for count in COUNTS:
            sets.append((f"mixed{count}", regions[:count], {m: (ref[m][0][:count + 1], ref[m][1][:int(ref[m][0][count])]) for m in MODES}))
        done = []
        for label, regs, want in sets:
            q = Large(ctx, d, regs)
            done.append((label, regs, want, {m: q.lists(m, large=False) for m in MODES}))
            q.dispose()
        _SETS[name] = done
    return d, _SETS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("name", Q.MESHES)
def test_l1_parity_with_the_brute_force_and_with_region_overlaps(ctx, name, cap):
    d, sets = region_sets(ctx, name)
    with task_cap(ctx, cap):
        for label, regs, want, old in sets:
            q = Large(ctx, d, regs)
            for mode in MODES:
                got = q.lists(mode)
                Q.assert_equal_lists(old[mode], want[mode], (name, label, mode, "lbvh_region_overlaps"))
                Q.assert_equal_lists(got, want[mode], (name, cap, label, mode))
                assert (words(got[0]) == words(old[mode][0])).all() and (got[1] == old[mode][1]).all()
                assert (q.run(mode) == want[mode][0]).all()          # the count-only form
            q.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0


@pytest.mark.gpu
def test_l2_a_grid_of_1e5_triangles_at_the_default_cap(ctx):
    """224 x 224 quads: one half space and 16 thin frusta; 17 regions get 65 536 tasks each, far fewer than the triangles inside the
    half space, so the expansion runs several rounds and stops on the cap"""
    tris = scenes.grid_scene(quads=224, half=4.0)
    assert len(tris) == 100352 and N().lib.lbvh_debug_region_task_cap_of(0, 17) == 65536
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    n = np.array([1.0, 0.5, 0.1])
    planes = [np.tile(np.append(n, 2.0), (6, 1))]                    # three quarters of the grid
    rng = np.random.default_rng(21)
    for k in range(16):
        eye = np.array([[rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0), rng.uniform(2.0, 6.0)]])
        target = np.array([[rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 3.0), 0.0]])
        cam = {"screen_width": 64, "screen_height": 64, "camera_fov": 0.5, "near_plane": 0.1, "camera_to_world": Q._look_at(eye, target)[0].astype(F)}
        x0, y0 = rng.integers(0, 48, 2)
        planes.append(H().frustum_planes(cam, far=20.0, rect=(x0, y0, x0 + 16, y0 + 16))["plane"][0])
    regions = R.make_regions(np.array(planes))
    ref = R.reference(regions, lo, hi)
    sizes = np.diff(ref[R.TOUCHING][0]).astype(np.int64)
    assert sizes[0] > 65536 and (sizes[1:] > 0).sum() >= 8 and 0 < int(ref[R.CONTAINED][0][-1]) < int(ref[R.TOUCHING][0][-1])
    q = Large(ctx, d, regions)
    for mode in MODES:
        Q.assert_equal_lists(q.lists(mode), ref[mode], mode)
    assert N().lib.lbvh_sync(ctx.handle) == 0
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 8])
def test_l3_two_calls_write_the_same_bytes(ctx, cap):
    d, sets = region_sets(ctx, "example_object3")
    label, regs, want, old = sets[-1]
    q = Large(ctx, d, regs)
    total = int(want[R.TOUCHING][0][-1])
    bufs = [H().DataBuffer(ctx, total, np.uint32) for _ in range(2)]
    with task_cap(ctx, cap):
        for buf in bufs:
            buf.fill_u32(POISON)
            assert (q.run(R.TOUCHING, buf) == want[R.TOUCHING][0]).all()
    first, second = (buf.get_data().copy() for buf in bufs)
    assert (first == second).all() and (V.sort_segments(want[R.TOUCHING][0], first) == want[R.TOUCHING][1]).all()
    for buf in bufs:
        buf.dispose()
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [4, 65536])
def test_l4_the_csr_contract(ctx, cap):
    """cap 65 536: every task of these regions is one leaf, so a capacity inside a segment falls between two tasks of one region;
    cap 4: at most four tasks per region, so it falls inside a task"""
    d, sets = region_sets(ctx, "cfg1_4096")
    label, regs, want, old = sets[-1]
    assert label == "mixed1500"
    q = Large(ctx, d, regs)
    guard = 4096
    with task_cap(ctx, cap):
        for mode in MODES:
            ro, rt = want[mode]
            total = int(ro[-1])
            assert (q.run(mode, None) == ro).all()                       # capacity == 0, d_tris == NULL
            n = np.diff(ro).astype(np.int64)
            cut = int(np.nonzero((n >= 8) & (ro[:-1] > total // 3))[0][0])
            buf = H().DataBuffer(ctx, total + guard, np.uint32)
            for capacity in (int(ro[cut]) + 1, int(ro[cut]) + int(n[cut]) // 2, int(ro[cut + 1]) - 1, int(ro[cut]), 1):
                buf.fill_u32(0xABABABAB)
                off = q.run(mode, buf, capacity=capacity)
                got = buf.get_data().copy()
                assert (off == ro).all() and int(off[-1]) == total       # d_offsets[count] still says what was needed
                assert (got[capacity:] == 0xABABABAB).all()              # nothing at the capacity or beyond
                fits = int(np.nonzero(ro <= capacity)[0][-1])            # the segments before this offset fit
                last = int(ro[fits])
                assert (V.sort_segments(ro[:fits + 1], got[:last]) == rt[:last]).all()
            buf.fill_u32(0xABABABAB)
            assert (q.run(mode, buf, capacity=total) == ro).all()
            H().sort_index_segments(ctx, q.offsets, buf, q.count)
            got = buf.get_data().copy()
            assert (got[total:] == 0xABABABAB).all() and (got[:total] == rt).all()
            buf.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0
    q.dispose()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 3, 7])
def test_l5_wave_caps_refill_the_lanes(ctx, waves):
    """1 500 regions of 8 task slots on 1, 2, 3 and 7 waves: runs of 12 000 .. 1 715 slots"""
    d, sets = region_sets(ctx, "grid_80x80")
    label, regs, want, old = sets[-1]
    q = Large(ctx, d, regs)
    h, lib = ctx.handle, N().lib
    N().check(h, lib.lbvh_debug_ray_waves(h, waves))
    try:
        with task_cap(ctx, 8):
            got = [q.lists(mode) for mode in MODES]
    finally:
        N().check(h, lib.lbvh_debug_ray_waves(h, 0))
    for mode, lists in zip(MODES, got):
        Q.assert_equal_lists(lists, want[mode], (waves, mode))
    assert lib.lbvh_sync(h) == 0
    q.dispose()


@pytest.mark.gpu
def test_l5_the_stack_limit_is_reported_not_a_short_list():
    """four tasks around the whole mesh with one stack entry in LDS and one in device memory: LBVH_FAULT_RAY_STACK at the next lbvh_sync"""
    tris = Q.scene("cfg1_4096")
    c2 = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(c2, tris).awake()
        lo, hi = library_boxes(d)
        whole = H().aabb_planes(lo.min(axis=0) - F(1.0), hi.max(axis=0) + F(1.0))
        ref = R.reference(whole, lo, hi)
        q = Large(c2, d, whole)
        h, lib = c2.handle, N().lib
        with task_cap(c2, 4):
            Q.assert_equal_lists(q.lists(R.TOUCHING), ref[R.TOUCHING])
            assert lib.lbvh_sync(h) == 0
            N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
            N().check(h, lib.lbvh_debug_ray_stack_limit(h, 1))
            s = d.container.scene()                                   # (no download here: it would report the fault before lbvh_sync does)
            N().check(h, lib.lbvh_region_overlaps_large(h, q.regions.device, 1, R.TOUCHING, C.byref(s), q.offsets.device, None, 0))
            assert lib.lbvh_sync(h) == -3
            assert b"stack" in lib.lbvh_last_error(h)
            N().check(h, lib.lbvh_debug_ray_stack_limit(h, 0))
            N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
            Q.assert_equal_lists(q.lists(R.CONTAINED), ref[R.CONTAINED], "after the stack limit")
        assert lib.lbvh_sync(h) == 0
        q.dispose()
    finally:
        c2.close()


@pytest.mark.gpu
def test_l6_rejections_a_stale_scene_a_failed_allocation_and_the_counters():
    tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
    a, b, c = positions(tris)
    ctx = H().Context(0)
    try:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        lo, hi = library_boxes(d)
        rng = np.random.default_rng(5)
        count = 65537
        k = rng.integers(0, 64, count)
        regions = H().obb_planes(a[k] + rng.normal(size=(count, 3)), Q._rotations(rng, count), rng.uniform(0.5, 6.0, (count, 3)))
        q = Large(ctx, d, regions)
        lst = H().DataBuffer(ctx, 130 * 64 + 1, np.uint32)
        stats = H().DataBuffer(ctx, 1, L().RAY_STATS)
        lib, h, s = N().lib, ctx.handle, d.container.scene()
        call = lib.lbvh_region_overlaps_large
        dq, do, dl = q.regions.device, q.offsets.device, lst.device
        at = lambda buf, n: C.c_void_p(buf.device.value + n)
        bufs = (q.offsets, lst)

        def untouched():
            return all((words(buf.get_data()) == POISON).all() for buf in bufs)

        for buf in bufs:
            buf.fill_u32(POISON)
        assert call(h, dq, 0, 0, C.byref(s), do, dl, 64) == 0                                     # count == 0: a no-op
        for args in ((None, 10, 0, C.byref(s), do, None, 0), (dq, 10, 0, None, do, None, 0), (dq, 10, 0, C.byref(s), None, None, 0),
                     (dq, 10, 2, C.byref(s), do, None, 0), (dq, 10, 0xFFFFFFFF, C.byref(s), do, None, 0),
                     (dq, 10, 1, C.byref(s), do, None, 5), (at(q.regions, 8), 10, 0, C.byref(s), do, None, 0),
                     (dq, 10, 0, C.byref(s), at(q.offsets, 4), None, 0), (dq, 10, 1, C.byref(s), do, at(lst, 2), 8),
                     (dq, 65537, 0, C.byref(s), do, None, 0), (dq, 1 << 32, 0, C.byref(s), do, None, 0)):
            assert call(h, *args) == -1, args
            assert lib.lbvh_last_error(h).startswith(b"lbvh_region_overlaps_large: "), lib.lbvh_last_error(h)
        assert call(None, dq, 10, 0, C.byref(s), do, None, 0) == -1
        for bad in (1, 3, 65537):
            assert lib.lbvh_debug_region_task_cap(h, bad) == -1
        d.container.triangle_data.sync()                               # triangles uploaded without a rebuild: the derived scene is stale
        assert call(h, dq, 130, 0, C.byref(s), do, None, 0) == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(b"lbvh_region_overlaps_large: ") and b"stale" in msg, msg
        assert untouched()
        d.rebuild(fast=True)
        # 65 536 regions are accepted: 64 task slots each, the offsets of lbvh_region_overlaps
        q.count = 65536
        want = Q.Regions.run(q, R.TOUCHING)
        assert int(want[65536]) > 0 and (Large.run(q, R.TOUCHING)[:65537] == want[:65537]).all()
        # a failed growth of the ray scratch or of the task buffer: the error, and the context goes on
        q.count = 130
        ref = R.reference(regions[:130], lo, hi)
        for kth in (1, 2):
            ctx2 = H().Context(0)
            try:
                d2 = H().RaytracingMeshDrawer(ctx2, tris).awake()
                q2 = Large(ctx2, d2, regions[:130])
                assert (Q.Regions.run(q2, R.TOUCHING) == ref[R.TOUCHING][0]).all()       # the wide nodes and a small ray scratch exist
                ctx2.debug_switch(N().DEBUG_SWITCH_FAIL_RESERVE, kth)
                q2.run(R.TOUCHING, expect=-2)
                assert b"LBVH_DEBUG_FAIL_RESERVE" in lib.lbvh_last_error(ctx2.handle)
                Q.assert_equal_lists(q2.lists(R.TOUCHING), ref[R.TOUCHING], kth)
                assert lib.lbvh_sync(ctx2.handle) == 0
            finally:
                ctx2.close()
        # aligned sub-ranges are fine; the plain and the counting instantiation write the same words, and the latter counts
        assert call(h, at(q.regions, 96), 10, 0, C.byref(s), at(q.offsets, 8), at(lst, 4), 8) == 0
        small = Large(ctx, d, regions[:130])
        plain = [small.lists(mode) for mode in MODES]
        stats.fill_u32(0)
        N().check(h, lib.lbvh_ray_stats_target(h, stats.device))
        try:
            with task_cap(ctx, 4):
                counted = [small.lists(mode) for mode in MODES]
        finally:
            N().check(h, lib.lbvh_ray_stats_target(h, None))
        st = stats.get_data()[0]
        for mode, pl, cl in zip(MODES, plain, counted):
            Q.assert_equal_lists(pl, ref[mode], mode)
            assert (pl[0] == cl[0]).all() and (pl[1] == cl[1]).all()
        # per mode a count-only call and a full one: three task walks of at most four tasks per region, two expansions of at least the root
        assert 0 < st["rays"] <= 130 * 4 * 3 * 2 and st["node_fetches"] >= 130 * 2 * 2 and st["triangle_tests"] > 0, st
        for buf in (lst, stats):
            buf.dispose()
        small.dispose()
        q.dispose()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_l7_the_live_path_list_is_dropped(ctx):
    """a path-traced frame with the call issued between the bounces equals the undisturbed frame"""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    cam_d = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam_d, bounces=4)
    img0 = pt.image()
    count = 160 * 96
    st0 = pt.states.get_data()[:count].copy()
    lo, hi = library_boxes(pt.drawer)
    rng = np.random.default_rng(12)
    n = 4 * count                                                    # 61 440 regions, 64 task slots each: the scratch grows in mid-frame
    k = rng.integers(0, len(lo), n)
    q = Large(ctx, pt.drawer, H().obb_planes((lo[k] + hi[k]) * F(0.5), Q._rotations(rng, n), rng.uniform(0.5, 3.0, (n, 3))))
    cam = N().Camera.from_dict(cam_d)
    h, s, lib = ctx.handle, pt.drawer.container.scene(), N().lib

    def large():
        N().check(h, lib.lbvh_region_overlaps_large(h, q.regions.device, n, R.TOUCHING, C.byref(s), q.offsets.device, None, 0))

    N().check(h, lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, 160, 96, C.byref(s), L().TRACE_FAST, pt.hits.device, None))
    large()
    N().check(h, lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), pt.states.device, pt.hits.device, 5, 0.7, 1e-3))
    for bnc in range(1, 4):
        large()
        N().check(h, lib.lbvh_path_bounce(h, C.byref(s), pt.states.device, pt.hits.device, count, bnc, 5, 0.7, 1e-3))
    large()
    N().check(h, lib.lbvh_path_scatter(h, C.byref(s), pt.hits.device, count, 4, 5, 0.7, pt.states.device))
    N().check(h, lib.lbvh_path_resolve(h, pt.states.device, count, pt.image_buf.device))
    assert (words(pt.states.get_data()[:count]) == words(st0)).all()
    assert (pt.image().view(np.uint16) == img0.view(np.uint16)).all()
    assert int(q.offsets.get_data()[n]) > n
    q.dispose()
    pt.drawer.on_destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [0, 4])
def test_l7_the_smallest_scene(ctx, cap):
    """two triangles, the fewest a tree can be built from: the answer of lbvh_region_overlaps"""
    tris = scenes.random_triangles(n=2, seed=3, extent=5.0, edge=2.0)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    lo, hi = library_boxes(d)
    regions = np.concatenate([special_regions(lo, hi), H().aabb_planes(lo[:1], hi[:1]), H().aabb_planes(lo[1:] - F(0.5), hi[1:] + F(0.5))])
    ref = R.reference(regions, lo, hi)
    assert int(ref[R.TOUCHING][0][-1]) >= 5 and int(ref[R.CONTAINED][0][-1]) >= 3
    q = Large(ctx, d, regions)
    with task_cap(ctx, cap):
        for mode in MODES:
            got = q.lists(mode)
            Q.assert_equal_lists(got, ref[mode], mode)
            Q.assert_equal_lists(got, q.lists(mode, large=False), mode)
    q.dispose()
    d.on_destroy()


@pytest.mark.gpu
def test_l8_the_cpp_driver_with_the_large_switch(ctx):
    """`lbvh_driver regions 2000 6 large`: RegionOverlapsLarge of lbvh_host.hpp in both modes, the numbers of the plain form"""
    exe = os.path.join(ROOT, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    count = 2000
    res = json.loads(subprocess.run([exe, "regions", str(count), "6", "large"], check=True, capture_output=True, text=True).stdout)
    tris, pos, lo, hi = driver_mesh(4096)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    ref = R.reference(R.driver_regions(lo, hi, count, seed=6), *library_boxes(d))
    d.on_destroy()
    assert (res["triangles"], res["regions"], res["large"]) == (4096, count, True)
    for mode, key in ((R.TOUCHING, "touching"), (R.CONTAINED, "contained")):
        ro, rt = ref[mode]
        n = np.diff(ro).astype(np.int64)
        weighted = int(((np.arange(len(rt), dtype=np.uint64) + np.uint64(1)) * rt.astype(np.uint64)).sum())
        assert int(ro[-1]) > 0
        assert (res[key]["total"], res[key]["non_empty"], res[key]["flagged"], res[key]["weighted_index_sum"]) == \
            (int(ro[-1]), int((n > 0).sum()), int((n > 0).sum()), weighted), key
    ro, rt = ref[R.TOUCHING]
    first = np.nonzero(np.diff(ro))[0][:3]
    assert res["segments"] == [[int(k)] + rt[int(ro[k]):int(ro[k + 1])].tolist() for k in first]
