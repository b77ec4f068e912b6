"""What the entry points that walk the derived scene one ray or query per lane have in common (lbvh_walk.h, lbvh_walk.hip: begin_walk, the
prologue they share; LBVH_LAUNCH_STATS, the one place that picks the counting or the plain instantiation of a walker;
launch_per_query, the one launch of the point queries and the sphere and capsule casts; csr_query and csr_offsets, the count walk
-> scan -> fill walk of every CSR answer — while each family keeps its own argument checks, whose text a row quotes): one
table, one test, a row per entry point.  The answers themselves are the per-query test files' business; here every comparison
is between two calls of the library, word for word on uint32 views.

Scene: 64 random triangles.  130 queries per call: three waves, the last one partial.  (Which walker built the four-wide nodes after a
rebuild is not visible through include/lbvh_debug.h, so it is not checked here.)"""
import ctypes as C

import numpy as np
import pytest

from query_support import H, L, N, words
from unitysimpleraytracing_amd import scenes

pytestmark = pytest.mark.gpu

COUNT = 130
K = 3
POISON = 0x7FC0DEAD
F = np.float32


def _rays(tris, rng):
    """aimed at points of the triangles from outside their box; every fifth one aimed away"""
    k = rng.integers(0, len(tris), COUNT)
    w = rng.dirichlet((1, 1, 1), COUNT).astype(F)
    target = tris["a"][k, :3] * w[:, :1] + tris["b"][k, :3] * w[:, 1:2] + tris["c"][k, :3] * w[:, 2:]
    d = rng.normal(size=(COUNT, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::5] *= -1.0
    return (target - d * 40.0).astype(F), d.astype(F), target.astype(F)


def _table(tris):
    """name -> (queries, extra arguments between count and the scene, outputs as (dtype, entries, required alignment in bytes),
    lbvh_last_error after a misaligned pointer).  The call is fn(ctx, queries, count, *extra, scene, *outputs), a CSR row's capacity
    last; the extra arguments are lbvh_point_crossings' directions, k, and the region rows' mode.  The message is the text of the
    alignment check of the entry point's family in lbvh_path.hip or lbvh_query_*.hip, as LBVH_REQUIRE reports it ("invalid argument: " and the
    condition) or, for the region rows, under the entry point's own name."""
    lay = L()
    rng = np.random.default_rng(23)
    origin, d, target = _rays(tris, rng)
    rays = np.zeros(COUNT, dtype=lay.RAY)
    rays["origin"], rays["dir"], rays["t_min"], rays["t_max"] = origin, d, 0.0, np.inf
    casts = np.zeros(COUNT, dtype=lay.SPHERE_RAY)
    casts["origin"], casts["dir"], casts["radius"], casts["t_max"] = origin, d, 0.4, np.inf
    capsules = np.zeros(COUNT, dtype=lay.CAPSULE_RAY)
    capsules["origin"], capsules["dir"], capsules["radius"], capsules["t_max"] = origin, d, 0.4, np.inf
    capsules["axis"] = rng.normal(size=(COUNT, 3)).astype(F)
    points = np.zeros(COUNT, dtype=lay.POINT_QUERY)
    points["p"] = target + rng.normal(size=(COUNT, 3)).astype(F)
    points["max_dist2"] = 9.0
    boxes = np.zeros(COUNT, dtype=lay.AABB)
    boxes["min"], boxes["max"] = points["p"] - F(2.0), points["p"] + F(2.0)
    regions = H().aabb_planes(boxes["min"], boxes["max"])
    tri_queries = np.zeros(COUNT, dtype=lay.TRI_QUERY)
    tri_queries["a"], tri_queries["skip"] = points["p"], lay.NULL
    tri_queries["b"] = points["p"] + rng.normal(size=(COUNT, 3)).astype(F) * F(3.0)
    tri_queries["c"] = points["p"] + rng.normal(size=(COUNT, 3)).astype(F) * F(3.0)
    dirs = np.array([[1, 0, 0], [0.3, 1, 0.2], [0.1, -0.2, 1]], dtype=F)
    u32, u64 = np.dtype(np.uint32), np.dtype(np.uint64)
    hit, cp = (lay.HIT, COUNT, 16), (lay.CLOSEST_POINT, COUNT, 16)
    flag = (u32, COUNT, 4)
    csr = [(u64, COUNT + 1, 8), (u32, COUNT * len(tris), 4)]
    csr_hits = [(u64, COUNT + 1, 8), (lay.HIT, COUNT * len(tris), 16)]
    touching = (lay.REGION_TOUCHING,)
    bad = "invalid argument: "
    out_any = " && ((uintptr_t)d_out & (ANY ? 3 : 15)) == 0"
    found = " && ((uintptr_t)d_found & 3) == 0"
    lists = "((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0"
    region_lists = "((uintptr_t)d_regions & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0"
    flags = " && ((uintptr_t)d_flags & 3) == 0"
    plain_rays = bad + "((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_out & (Q != kClosest ? 3 : 15)) == 0"
    return {
        "lbvh_trace_closest": (rays, (), [hit], plain_rays),
        "lbvh_trace_occluded": (rays, (), [flag], plain_rays),
        "lbvh_count_hits": (rays, (), [flag], plain_rays),
        "lbvh_closest_point_query": (points, (), [cp], bad + "((uintptr_t)d_queries & 15) == 0" + out_any),
        "lbvh_within_distance": (points, (), [flag], bad + "((uintptr_t)d_queries & 15) == 0" + out_any),
        "lbvh_sphere_cast": (casts, (), [hit], bad + "((uintptr_t)d_casts & 15) == 0" + out_any),
        "lbvh_sphere_cast_any": (casts, (), [flag], bad + "((uintptr_t)d_casts & 15) == 0" + out_any),
        "lbvh_k_closest_points": (points, (K,), [(lay.CLOSEST_POINT, COUNT * K, 16), flag],
                                  bad + "((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_out & 15) == 0" + found),
        "lbvh_trace_k_closest": (rays, (K,), [(lay.HIT, COUNT * K, 16), flag],
                                 bad + "((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_hits & 15) == 0" + found),
        "lbvh_box_overlaps": (boxes, (), csr, bad + lists),
        "lbvh_gather_within_distance": (points, (), csr, bad + lists),
        "lbvh_point_crossings": (points, (dirs.ctypes.data_as(C.POINTER(C.c_float)), len(dirs)), [flag],
                                 bad + "((uintptr_t)d_points & 15) == 0 && ((uintptr_t)d_parity & 3) == 0"),
        "lbvh_gather_hits": (rays, (), csr_hits,
                             bad + "((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_hits & 15) == 0"),
        "lbvh_triangle_intersections": (tri_queries, (), csr, bad + lists + flags),
        "lbvh_triangle_intersects_any": (tri_queries, (), [flag], bad + lists + flags),
        "lbvh_region_overlaps": (regions, touching, csr, "lbvh_region_overlaps: " + bad + region_lists + flags),
        "lbvh_region_overlaps_any": (regions, touching, [flag], "lbvh_region_overlaps_any: " + bad + region_lists + flags),
        # 130 regions: at or below LBVH_REGION_LARGE_MAX_COUNT (65 536), so the table's count stands.  The host gives each 16 384
        # task slots (the largest power of two not above 2^22 / 130): 2 129 920 slots, 33 280 waves of them on the 8 192 launched
        "lbvh_region_overlaps_large": (regions, touching, csr, "lbvh_region_overlaps_large: " + bad + region_lists),
        "lbvh_capsule_cast": (capsules, (), [hit], bad + "((uintptr_t)d_casts & 15) == 0" + out_any),
        "lbvh_capsule_cast_any": (capsules, (), [flag], bad + "((uintptr_t)d_casts & 15) == 0" + out_any),
    }, rays, dirs


PLAIN_RAYS = ("lbvh_trace_closest", "lbvh_trace_occluded", "lbvh_count_hits")
ENTRY_POINTS = PLAIN_RAYS + ("lbvh_closest_point_query", "lbvh_within_distance", "lbvh_sphere_cast", "lbvh_sphere_cast_any",
                             "lbvh_k_closest_points", "lbvh_trace_k_closest", "lbvh_box_overlaps", "lbvh_gather_within_distance",
                             "lbvh_point_crossings", "lbvh_gather_hits", "lbvh_triangle_intersections", "lbvh_triangle_intersects_any",
                             "lbvh_region_overlaps", "lbvh_region_overlaps_any", "lbvh_capsule_cast", "lbvh_capsule_cast_any",
                             "lbvh_region_overlaps_large")                   # (last: its task slots grow the ray scratch)


class Bench:
    """a context of its own (its ray scratch has never grown, its debug settings are this file's), the scene, and what
    lbvh_trace_rays answers for the table's rays before any query has run"""

    def __init__(self):
        self.ctx = H().Context(0)
        self.tris = scenes.random_triangles(n=64, seed=8, extent=10.0, edge=6.0)
        self.drawer = H().RaytracingMeshDrawer(self.ctx, self.tris).awake()
        self.table, rays, self.dirs = _table(self.tris)
        st = np.zeros(COUNT, dtype=L().PATH_STATE)
        st["origin"], st["dir"], st["alive"] = rays["origin"], rays["dir"], 1
        st["alive"][7::9] = 0
        self.states = H().DataBuffer(self.ctx, COUNT, L().PATH_STATE)
        self.states.local[:] = st
        self.states.sync()
        self.path_hits = H().DataBuffer(self.ctx, COUNT, L().HIT)
        self.stats = H().DataBuffer(self.ctx, 1, L().RAY_STATS)
        self.expected_path_hits = self.trace_rays()
        assert 20 < (self.expected_path_hits["t"] < L().MAX_FLOAT).sum() < COUNT

    def trace_rays(self):
        s = self.drawer.container.scene()
        self.path_hits.fill_u32(POISON)
        N().check(self.ctx.handle, N().lib.lbvh_trace_rays(self.ctx.handle, self.states.device, COUNT, 0.0, C.byref(s), self.path_hits.device))
        return self.path_hits.get_data().copy()

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_point_keeps_the_shared_contract(bench, name):
    nat, h, lib = N(), bench.ctx.handle, N().lib
    fn = getattr(lib, name)
    queries, extra, outs, misaligned = bench.table[name]
    csr = outs[0][0] == np.uint64
    qb = H().DataBuffer(bench.ctx, COUNT + 1, queries.dtype)
    qb.local[:COUNT] = queries
    qb.sync()
    bufs = [H().DataBuffer(bench.ctx, entries + 1, dtype) for dtype, entries, _ in outs]
    s = bench.drawer.container.scene()
    at = lambda buf, k: C.c_void_p(buf.device.value + k)

    def call(count=COUNT, q=None, out0=None):
        ptrs = [out0 if out0 is not None else bufs[0].device] + [b.device for b in bufs[1:]]
        if csr:
            ptrs.append(bufs[1].size - 1)                                  # the capacity
        return fn(h, q if q is not None else qb.device, count, *extra, C.byref(s), *ptrs)

    def poison():
        for b in bufs:
            b.fill_u32(POISON)

    def untouched():
        return all((words(b.get_data()) == POISON).all() for b in bufs)

    def answer():
        poison()
        nat.check(h, call())
        got = [words(b.get_data()).copy() for b in bufs]
        if csr:                                                            # the list as far as the last offset says
            total = int(bufs[0].local[COUNT])
            assert 0 < total <= bufs[1].size - 1
            got[1] = got[1][:total * (outs[1][0].itemsize // 4)]
        return got

    def same(a, b):
        return len(a) == len(b) and all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))

    try:
        # count == 0 is a no-op; a misaligned query or output pointer is refused with the family's own message; nothing is
        # written by either
        poison()
        assert call(count=0) == 0
        assert call(q=at(qb, 4)) == -1
        assert lib.lbvh_last_error(h) == misaligned.encode()
        assert call(out0=at(bufs[0], 4 if outs[0][2] > 4 else 2)) == -1
        assert lib.lbvh_last_error(h) == misaligned.encode()
        assert untouched()
        # triangles uploaded without a rebuild: the derived scene is stale, and the message names this entry point
        bench.drawer.container.triangle_data.sync()
        assert call() == -1
        msg = lib.lbvh_last_error(h)
        assert msg.startswith(name.encode() + b": ") and b"stale" in msg, msg
        assert untouched()
        bench.drawer.rebuild(fast=True)                                    # (the four-wide nodes are made again by the next walk)
        # the plain instantiation: the statistics target cleared, a poisoned statistics block stays as it is
        bench.stats.fill_u32(POISON)
        plain = answer()
        assert (words(bench.stats.get_data()) == POISON).all()
        assert any((w != POISON).any() for w in plain)
        # the call dropped the live-ray list: lbvh_trace_rays makes its own again
        assert (words(bench.trace_rays()) == words(bench.expected_path_hits)).all()
        # the counting instantiation: the same words, and it counted
        bench.stats.fill_u32(0)
        nat.check(h, lib.lbvh_ray_stats_target(h, bench.stats.device))
        try:
            counted = answer()
        finally:
            nat.check(h, lib.lbvh_ray_stats_target(h, None))
        st = bench.stats.get_data()[0]
        assert same(counted, plain)
        assert st["rays"] > 0 and st["node_fetches"] > 0 and st["triangle_tests"] > 0, st
        # plain rays over the binary nodes: the four-wide walk's words, also as the first walk after a rebuild
        if name in PLAIN_RAYS:
            bench.drawer.rebuild(fast=True)
            nat.check(h, lib.lbvh_debug_ray_walker(h, 0))
            try:
                binary = answer()
            finally:
                nat.check(h, lib.lbvh_debug_ray_walker(h, 1))
            assert same(binary, plain)
            assert (words(bench.trace_rays()) == words(bench.expected_path_hits)).all()
    finally:
        nat.check(h, lib.lbvh_ray_stats_target(h, None))
        nat.check(h, lib.lbvh_debug_ray_walker(h, 1))
        for b in [qb] + bufs:
            b.dispose()
