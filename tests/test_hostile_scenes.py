"""The ray, point and overlap queries against their brute-force references on the scenes of tests/hostile_scenes.py: two and three
triangles, one Morton cell, every triangle stored eight times, triangles outside the scene box, degenerate and needle triangles, a
coplanar fan.  Per scene one ray set (about 600 rays of query_support.mix_ranges + 100 aimed through vertices, edge midpoints and
along edges), one point set (about 600 of query_support.mixed_queries + 100 exactly at vertices and centroids) and one box set
(random, zero-extent, whole-scene, inverted and NaN boxes); the references are computed once per scene.

CPU (unmarked): what the references alone must meet so that no comparison is vacuous, and the fp32 references against float64
evaluations of the same definitions on these scenes.
GPU: every entry point below == its reference fed the library's own boxes, word for word (CSR segments after sorting), at the
default stack split and once more with the LDS part of the stack cut to one entry:
    lbvh_trace_closest / lbvh_trace_occluded / lbvh_count_hits     ray_reference
    lbvh_point_crossings                                           ray_reference.crossing_rays + parity_words
    lbvh_trace_k_closest, k = 1, 3, 32                             k_hits_reference
    lbvh_gather_hits                                               gather_hits_reference
    lbvh_closest_point_query / lbvh_within_distance                point_reference
    lbvh_k_closest_points, k = 1, 3, 32                            k_closest_reference
    lbvh_gather_within_distance / lbvh_box_overlaps                overlap_reference
The region family (regions, large regions, plane sections) is held to its brute force on the same scenes in
tests/test_hostile_regions.py; the swept shapes, the contacts and the triangle and segment families are not covered yet."""
import numpy as np
import pytest

import gather_hits_reference as G
import hostile_scenes as HS
import k_closest_reference as KC
import k_hits_reference as KH
import oracle as O
import overlap_reference as V
import point_reference as PR
import ray_reference as RR
from query_support import (aimed_rays, H, KMAX, L, library_boxes, make_queries, make_rays, mix_ranges, mixed_queries, N,
                           padded_boxes, positions, row_words, scene_rays, words)

F = np.float32
INF = F(np.inf)
KS = (1, 3, KMAX)
N_MIXED, N_AIMED = 600, 100


# ---- the query sets ----------------------------------------------------------------------------------------------------------

def hittable(name, n):
    """the triangles a ray can meet: all but the points and collinear triples of `slivers`"""
    return np.nonzero(HS.sliver_kinds() >= HS.NEEDLE)[0] if name == "slivers" else np.arange(n)


def pow2_below(x):
    return 2.0 ** np.floor(np.log2(x))


def aimed_ray_set(name, a, b, c, rng, count=N_AIMED):
    """Rays with t_min = 0 through vertices (4 in 10), through edge midpoints (3 in 10) and along edges (3 in 10) of the triangles a
    ray can meet; on `slivers` a third of them go through needle centroids instead.  Directions: small dyadic vectors (k / 8), a
    tenth of them along an axis; the target lies at t = s, a power of two, so on dyadic scenes (`fan`) origin, t and the tie are
    exact.  t_max: +inf, s (strict: the target does not count) or the float above s."""
    sel = hittable(name, len(a))
    verts = np.stack([a, b, c])
    k = sel[rng.integers(0, len(sel), count)]
    corner = rng.integers(0, 3, count)
    v0, v1 = verts[corner, k], verts[(corner + 1) % 3, k]
    mode = rng.choice(3, count, p=[0.4, 0.3, 0.3])                  # 0 vertex, 1 edge midpoint, 2 along the edge
    d = rng.integers(-8, 9, (count, 3)).astype(np.float64)
    d[(d == 0).all(axis=1)] = (0.0, 0.0, -8.0)
    axis = rng.random(count) < 0.1
    d[axis] = np.eye(3)[rng.integers(0, 3, axis.sum())] * rng.choice([-8.0, 8.0], axis.sum())[:, None]
    d = (d / 8.0).astype(F)
    pts = np.concatenate([a, b, c])
    extent = float((pts.max(axis=0) - pts.min(axis=0)).max())
    s = (pow2_below(extent) * 2.0 ** -rng.integers(0, 3, count)).astype(F)
    target = np.where((mode == 1)[:, None], (v0 + v1) * F(0.5), v0)
    if name == "slivers":
        needle = np.nonzero(HS.sliver_kinds() == HS.NEEDLE)[0]
        third = np.nonzero(rng.random(count) < 0.33)[0]
        kn = needle[rng.integers(0, len(needle), len(third))]
        target[third] = (a[kn] + b[kn] + c[kn]) / F(3.0)
        mode[third] = 0
    along = mode == 2
    d[along] = (v1 - v0)[along]
    s[along] = F(0.5)
    origin = (target - s[:, None] * d).astype(F)
    pick = rng.choice(3, count, p=[0.7, 0.15, 0.15])
    t_max = np.where(pick == 0, INF, np.where(pick == 1, s, np.nextafter(s, INF))).astype(F)
    return make_rays(origin, d, F(0.0), t_max)


def ray_set(name, a, b, c, lo, hi):
    """-> (rays, aimed mask): half of the mixed rays start in the scene's box (scene_rays), half come from outside at surface points
    of the triangles a ray can meet (aimed_rays); their ranges are mix_ranges'; the aimed set is spread among them"""
    rng = np.random.default_rng(100 + len(a))
    sel = hittable(name, len(a))
    if name == "slivers":                                  # three needles in four left to the aimed set: a hit on one is a coin toss in fp32
        kind = HS.sliver_kinds()[sel]
        sel = np.concatenate([sel[kind == HS.ORDINARY], sel[kind == HS.NEEDLE][::4]])
    half = N_MIXED // 2
    o1, d1 = scene_rays(a, b, c, half, rng)
    o2, d2 = aimed_rays(a[sel], b[sel], c[sel], N_MIXED - half, rng, along_z=0.3)[:2]
    mixed = mix_ranges(np.concatenate([o1, o2]), np.concatenate([d1, d2]), rng, lambda r: KH.reference(r, a, b, c, lo, hi, KMAX))
    rays = np.concatenate([mixed, aimed_ray_set(name, a, b, c, rng)])
    aimed = np.arange(len(rays)) >= N_MIXED
    order = rng.permutation(len(rays))
    return rays[order], aimed[order]


def point_set(name, a, b, c, lo, hi):
    """-> (queries, aimed mask): mixed_queries, plus points exactly at vertices (7 in 10) and at centroids (on `copies`: of the
    originals) with radii +inf, the scene's typical nearest distance, or 1e-30"""
    rng = np.random.default_rng(200 + len(a))
    mixed, unb = mixed_queries(a, b, c, lo, hi, N_MIXED, 300 + len(a))
    k = rng.integers(0, len(a), N_AIMED)
    p = np.stack([a, b, c])[rng.integers(0, 3, N_AIMED), k]
    cen = rng.random(N_AIMED) < 0.3
    p[cen] = ((a[k] + b[k] + c[k]) / F(3.0))[cen]
    d = unb.records["dist2"]
    typical = F(np.median(d[d > 0]))
    r2 = rng.choice(np.array([np.inf, np.inf, typical, 1e-30], dtype=F), N_AIMED)
    queries = np.concatenate([mixed, make_queries(p.astype(F), r2)])
    aimed = np.arange(len(queries)) >= N_MIXED
    order = rng.permutation(len(queries))
    return queries[order], aimed[order]


def box_set(a, b, c, lo, hi):
    """about 600 boxes: 400 random ones (centres in the scene box grown by a tenth, half-extents up to a quarter of it), 100 of
    zero extent at vertices, 40 of zero extent anywhere, 20 that hold the whole scene, 20 inverted and 20 with a NaN bound"""
    rng = np.random.default_rng(400 + len(a))
    slo, shi = lo.min(axis=0).astype(np.float64), hi.max(axis=0).astype(np.float64)
    ext = shi - slo
    centre = rng.uniform(slo - 0.1 * ext, shi + 0.1 * ext, (400, 3))
    half = rng.uniform(0.0, 0.25 * ext, (400, 3))
    vert = np.stack([a, b, c])[rng.integers(0, 3, 100), rng.integers(0, len(a), 100)].astype(np.float64)
    anywhere = rng.uniform(slo, shi, (40, 3))
    grow = rng.uniform(0.0, 1.0, (20, 1)) * ext
    inv = rng.uniform(slo, shi, (20, 3))
    nan_lo = rng.uniform(slo, shi, (20, 3))
    nan_hi = nan_lo + 0.5 * ext
    nan_lo[:10, 1] = np.nan
    nan_hi[10:, 2] = np.nan
    bmin = np.concatenate([centre - half, vert, anywhere, slo - grow, inv + 0.25 * ext, nan_lo])
    bmax = np.concatenate([centre + half, vert, anywhere, shi + grow, inv, nan_hi])
    order = rng.permutation(len(bmin))
    return V.make_boxes(bmin[order].astype(F), bmax[order].astype(F))


class Case:
    """one scene, its three query sets and every reference, from the given triangle boxes"""

    def __init__(self, name, lo, hi):
        self.name, self.tris = name, HS.scene(name)
        self.a, self.b, self.c = a, b, c = positions(self.tris)
        self.lo, self.hi = lo, hi
        self.rays, self.aimed_rays = ray_set(name, a, b, c, lo, hi)
        self.points, self.aimed_points = point_set(name, a, b, c, lo, hi)
        self.boxes = box_set(a, b, c, lo, hi)
        self.dirs = H().DEFAULT_DIRS
        self.ray = RR.reference(self.rays, a, b, c, lo, hi)
        self.khits = KH.reference(self.rays, a, b, c, lo, hi, KMAX)
        self.gather = G.reference(self.rays, a, b, c, lo, hi)
        # crossings: from the points and from the rays' origins (the points of `fan` lie in its plane and cross nothing)
        self.cross_points = make_queries(np.concatenate([self.points["p"], self.rays["origin"]]), INF)
        self.crossings = RR.reference(RR.crossing_rays(self.cross_points["p"], self.dirs), a, b, c, lo, hi).counts
        self.parity = RR.parity_words(self.crossings, len(self.dirs))
        self.point = PR.reference(self.points, a, b, c, lo, hi)
        self.kpoints = KC.reference(self.points, a, b, c, lo, hi, KMAX)
        self.within = V.gather_within_distance(self.points, a, b, c, lo, hi)
        self.overlap = V.box_overlaps(self.boxes, lo, hi)


_CASES = {}


def case_of(name, boxes=None):
    """the Case from the Morton stage's boxes as padded_boxes restates them (CPU), or from the library's own (GPU): the same
    object when they are the same words"""
    lo, hi = boxes if boxes is not None else padded_boxes(*positions(HS.scene(name)))
    key = (name, lo.tobytes(), hi.tobytes())
    if key not in _CASES:
        _CASES[key] = Case(name, lo, hi)
    return _CASES[key]


# ---- CPU: the scenes are what they claim to be ------------------------------------------------------------------------------

def morton_components(tris):
    """the oracle's Morton code of every triangle, taken apart into its three 10-bit components"""
    keys = O.morton_aabb(tris)[0][: len(tris)].astype(np.uint64)
    out = np.zeros((len(tris), 3), dtype=np.int64)
    for axis, shift in enumerate((2, 1, 0)):
        for bit in range(10):
            out[:, axis] |= (((keys >> np.uint64(3 * bit + shift)) & np.uint64(1)) << np.uint64(bit)).astype(np.int64)
    return keys, out


def test_scene_shapes():
    sizes = {name: len(HS.scene(name)) for name in HS.NAMES}
    assert sizes == dict(pair=2, triple=3, one_cell=257, copies=320, outside=200, slivers=256, fan=64)
    for name in HS.NAMES:
        t = HS.scene(name)
        assert t.dtype == L().TRIANGLE and np.isfinite(np.concatenate(positions(t))).all()
        assert (words(t) == words(HS.scene(name))).all()                      # fixed seeds
    # one_cell: exactly one Morton code; edges of about 2^-6, the 0.001 pad is comparable
    t = HS.scene("one_cell")
    keys, _ = morton_components(t)
    assert len(np.unique(keys)) == 1
    a, b, c = positions(t)
    edge = np.linalg.norm(b - a, axis=1)
    assert 2.0 ** -8 < np.median(edge) < 2.0 ** -5 and 0.001 > np.median(edge) / 32
    # outside: at least 60 triangles have a clamped component (0 or 1023 with the box's centre beyond the scene box on that axis)
    t = HS.scene("outside")
    _, comp = morton_components(t)
    lo, hi = padded_boxes(*positions(t))
    centre = (lo + hi) * F(0.5)
    clamped = ((comp == 0) & (centre < -125.0)) | ((comp == 1023) & (centre >= 125.0))
    print(f"outside: {int(clamped.any(axis=1).sum())} triangles with a clamped component")
    assert clamped.any(axis=1).sum() >= 60
    assert (np.abs(centre[0::2]) < 125.0).all() and np.abs(centre).max() > 350.0
    # copies: 40 groups of 8 identical records at scattered indices
    t, g = HS.scene("copies"), HS.copies_groups()
    for k in range(40):
        idx = np.nonzero(g == k)[0]
        assert len(idx) == 8 and (words(t[idx]).reshape(8, -1) == words(t[idx[:1]]).reshape(1, -1)).all() and not (np.diff(idx) == 1).all()
    # slivers: a quarter each, interleaved; the needles' aspect (long edge over height, float64 on the fp32 vertices)
    a, b, c = (x.astype(np.float64) for x in positions(HS.scene("slivers")))
    kind = HS.sliver_kinds()
    assert (np.bincount(kind) == 64).all() and (kind[:4] == [HS.POINT, HS.COLLINEAR, HS.NEEDLE, HS.ORDINARY]).all()
    assert ((a == b) & (a == c)).all(axis=1)[kind == HS.POINT].all()
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    assert (area2[kind == HS.COLLINEAR] == 0).all() and (np.linalg.norm(b - a, axis=1)[kind == HS.COLLINEAR] > 0).all()
    k = kind == HS.NEEDLE
    long_ = np.linalg.norm(b - a, axis=1)[k]
    assert (long_ / (area2[k] / long_)).min() >= 1e5
    assert (area2[kind == HS.ORDINARY] > 0.01).all()
    # fan: coplanar, one shared vertex, the second half the first mirrored
    a, b, c = positions(HS.scene("fan"))
    assert (a == HS.FAN_VERTEX).all() and (b[:, 2] == a[:, 2]).all() and (c[:, 2] == a[:, 2]).all()
    assert ((b[32:] - a[32:]) == (b[:32] - a[:32]) * np.array([-1, 1, 1], dtype=F)).all()


# ---- CPU: non-vacuity, on the references alone ------------------------------------------------------------------------------

def bounded(queries):
    return PR.active(queries) & (queries["max_dist2"] < PR.MAX_FLOAT)


@pytest.mark.parametrize("name", HS.NAMES)
def test_the_references_are_not_vacuous(name):
    """The floors: at least 25 % of the active rays have a candidate; at least 25 % of the active bounded point queries have one
    and at least 10 % have none; and what is asserted per scene below.  Reached (active rays with a candidate; bounded point
    queries with a candidate):
      pair      43 %; 58 %            triple   35 %; 53 %            one_cell 59 %; 57 %            outside  37 %; 58 %
      copies    45 %; 56 %; 266 rays hit, every tie count a multiple of 8, every winner the lowest index of its group of 8
      fan       38 %; 56 %; 68 rays with ties >= 4, the most 64
      slivers   48 %; 62 %; 55 candidates on needles, none on a point or collinear triangle; 188 point winners are points or
                collinear triples"""
    cs = case_of(name)
    rays, ref = cs.rays, cs.ray
    assert len(rays) == N_MIXED + N_AIMED and len(cs.points) == N_MIXED + N_AIMED and 550 <= len(cs.boxes) <= 700
    act = RR.active(rays)
    has = ref.counts[act] > 0
    qb = bounded(cs.points)
    found = cs.point.flags[qb] == 1
    n_over = np.diff(cs.overlap[0]).astype(np.int64)
    n_within = np.diff(cs.within[0]).astype(np.int64)
    print(f"{name}: {int(act.sum())} active rays, {100 * has.mean():.0f} % with a candidate, most candidates {int(ref.counts.max())}, "
          f"most ties {int(ref.ties.max())}; {int(qb.sum())} bounded point queries, {100 * found.mean():.0f} % with a candidate; "
          f"boxes: {100 * (n_over > 0).mean():.0f} % non-empty, longest {int(n_over.max())}; within: longest {int(n_within.max())}")
    assert act.sum() >= 500 and (~act).sum() >= 50
    assert has.mean() >= 0.25
    assert qb.sum() >= 150 and found.mean() >= 0.25 and (~found).mean() >= 0.10
    # ranges at a candidate and one float to either side of it are in the set, and so are exact zero-extent and whole-scene boxes
    t_open = KH.reference(make_rays(rays["origin"], rays["dir"], rays["t_min"], INF), cs.a, cs.b, cs.c, cs.lo, cs.hi, KMAX).records["t"]
    assert ((rays["t_max"][:, None] == t_open) & (t_open < RR.MAX_FLOAT)).any(axis=1).sum() >= 20
    assert (n_over == len(cs.tris)).sum() >= 20 and (n_over > 0).mean() >= 0.25
    zero = (cs.boxes["min"][:, :3] == cs.boxes["max"][:, :3]).all(axis=1)
    assert zero.sum() >= 140 and (n_over[zero] > 0).sum() >= 100 and (~V.box_active(cs.boxes)).sum() >= 40
    assert (n_within == len(cs.tris)).sum() >= 50 or name == "slivers"          # an unbounded radius holds every triangle
    # the k-th place is contested: rows cut at 1 and 3 inside longer candidate lists
    assert (cs.khits.candidates > 3).sum() >= 50 or name not in ("one_cell", "copies", "fan")
    assert (cs.kpoints.candidates > 3).sum() >= 100 or len(cs.tris) <= 3
    # crossings: some rays cross something (`fan`, a plate: 59); `copies` crosses everything eight times, `fan` mostly twice
    assert (cs.crossings > 0).sum() >= 50 and (cs.crossings == 0).sum() >= 100
    assert ((cs.parity != 0).sum() == 0) if name == "copies" else ((cs.parity != 0).sum() >= 100) or name == "fan"
    if name == "copies":
        hit = ref.counts > 0
        assert hit.sum() >= 150 and (ref.ties[hit] % 8 == 0).all() and (ref.counts % 8 == 0).all()
        g = HS.copies_groups()
        first = np.array([np.nonzero(g == k)[0][0] for k in range(40)])
        won = cs.point.flags == 1
        assert won.sum() >= 300 and (cs.point.records["tri"][won] == first[g[cs.point.records["tri"][won]]]).all()
        assert (ref.records["tri"][hit] == first[g[ref.records["tri"][hit]]]).all()
        assert (cs.kpoints.candidates % 8 == 0).all() and (n_within % 8 == 0).all() and (n_over % 8 == 0).all()
        print(f"copies: {int(hit.sum())} rays hit, {int(won.sum())} points have a winner")
    if name == "fan":
        print(f"fan: {int((ref.ties >= 4).sum())} rays with ties >= 4")
        assert (ref.ties >= 4).sum() >= 30 and ref.ties.max() == 64
    if name == "slivers":
        kind = HS.sliver_kinds()
        on = kind[cs.gather.records["tri"]]
        winners = kind[cs.point.records["tri"][cs.point.flags == 1]]
        print(f"slivers: candidates per kind {np.bincount(on, minlength=4).tolist()}, point winners per kind {np.bincount(winners, minlength=4).tolist()}")
        assert (on == HS.NEEDLE).sum() >= 1 and (on <= HS.COLLINEAR).sum() == 0
        assert (winners <= HS.COLLINEAR).sum() >= 20


# ---- CPU: the fp32 references against float64 on these scenes -----------------------------------------------------------------

def closest_hit64(rays, a, b, c, lo, hi):
    """(t, tri) of the closest candidate of every ray (tri = -1: none), the candidate rule of include/lbvh.h in float64 on the same
    fp32 inputs: own-box slab test with entry e, Moeller-Trumbore with its rejections, t >= e, t_min < t < min(t_max, MAX_FLOAT).
    Written with vector algebra, not ray_reference's scalar steps."""
    d64 = np.float64
    o, d = rays["origin"].astype(d64)[:, None, :], rays["dir"].astype(d64)[:, None, :]
    e1, e2 = (b - a).astype(d64)[None], (c - a).astype(d64)[None]               # the edges are the fp32 differences in both
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t1, t2 = (lo.astype(d64)[None] - o) * inv, (hi.astype(d64)[None] - o) * inv
        entry = np.fmin(t1, t2).max(axis=2)
        leave = np.fmax(t1, t2).min(axis=2)
        passes = (leave > entry) & (leave > 0)
        p = np.cross(d, e2)
        det = (e1 * p).sum(axis=2)
        s = o - a.astype(d64)[None]
        u = (s * p).sum(axis=2) / det
        q = np.cross(s, e1)
        v = (d * q).sum(axis=2) / det
        t = (e2 * q).sum(axis=2) / det
        miss = (np.abs(det) < d64(F(1e-8))) | (u < 0) | (u > 1) | (v < 0) | (u + v > 1)
        big = np.minimum(rays["t_max"], RR.MAX_FLOAT).astype(d64)
        cand = ~miss & passes & ~(t < entry) & (t > rays["t_min"].astype(d64)[:, None]) & (t < big[:, None])
    key = np.where(cand, t, np.inf)
    k = key.argmin(axis=1)
    rows = np.arange(len(rays))
    return key[rows, k], np.where(cand[rows, k], k, -1)


# float64 agreement: the bound of test_point_queries.py, 64 * 2^-24 * extent, where the scene stays below it; where it does not,
# 4 x the worst error measured here (units of 2^-24 * extent), see the docstring of the test
T_BOUND = dict(pair=4 * 138, triple=64, one_cell=4 * 152, copies=4 * 129, outside=4 * 117, slivers=4 * 845086, fan=64)
D_BOUND = dict(pair=64, triple=64, one_cell=64, copies=64, outside=64, slivers=4 * 256608, fan=64)


@pytest.mark.parametrize("name", HS.NAMES)
def test_references_agree_with_their_float64_evaluation(name):
    """On the non-degenerate triangles of the scene (all but the points and collinear triples of `slivers`), with the scene's own
    point set and its ray set opened to (0, +inf):
      distance   |sqrt(d32) - sqrt(d64)| <= D_BOUND * 2^-24 * extent, d = point_reference.nearest_dist2 in either precision
      closest t  |t32 - t64| * |dir| <= T_BOUND * 2^-24 * extent (the same form, relative to extent / |dir|, on t) on every ray
                 whose winner is the same triangle in both; a ray whose winner differs (a hit on an edge in one precision and
                 beside it in the other, or two hits within rounding) is excluded, and at most 2 % of the rays may be
    extent = the largest side of the scene's box.  The rays are the 600 mixed ones: the aimed ones go through vertices and along
    edges on purpose, where hit or miss is a matter of rounding (with them 15 .. 26 of 700 rays change their winner, on `fan` none).
    Measured worst errors in units of 2^-24 * extent, and rays excluded of 600:
      scene      extent    distance    closest t    excluded
      pair        44.36        1.56       137.74           0
      triple      60.18        1.33        48.11           0
      one_cell   0.0630        0.53       151.79           0
      copies      59.87        1.94       128.84           0
      outside     850.4        7.64       116.19           0
      slivers     39.96    256607.6     845085.3           7
      fan          8.00       13.08        10.36           0
    The distances stay below the 64 units of test_point_queries.py everywhere but on `slivers`; t passes them on grazing rays
    (Moeller-Trumbore divides by a determinant that cancels) on four scenes, and the needles of `slivers` lose every digit: there
    fp32 puts the nearest point of a needle up to 0.6 units from where float64 puts it.  A bound above 64 is 4 x the measured
    value, rounded up."""
    cs = case_of(name)
    sel = hittable(name, len(cs.tris))
    a, b, c, lo, hi = cs.a[sel], cs.b[sel], cs.c[sel], cs.lo[sel], cs.hi[sel]
    extent = float((cs.hi.max(axis=0) - cs.lo.min(axis=0)).max())
    unit = 2.0 ** -24 * extent
    pts = cs.points["p"]
    d32 = PR.nearest_dist2(pts, a, b, c, np.float32)
    d64 = PR.nearest_dist2(pts, a, b, c, np.float64)
    d_err = np.abs(np.sqrt(d32.astype(np.float64)) - np.sqrt(d64)).max() / unit
    mixed = cs.rays[~cs.aimed_rays]
    rays = make_rays(mixed["origin"], mixed["dir"], F(0.0), INF)
    ref = RR.reference(rays, a, b, c, lo, hi)
    t64, k64 = closest_hit64(rays, a, b, c, lo, hi)
    k32 = np.where(ref.flags == 1, ref.records["tri"].astype(np.int64), -1)
    same = (k32 == k64) & (k32 >= 0)
    differs = k32 != k64
    scale = np.linalg.norm(rays["dir"].astype(np.float64), axis=1)
    t_err = (np.abs(ref.records["t"].astype(np.float64) - t64) * scale)[same].max() / unit
    print(f"{name}: extent {extent:.4g}; distance worst {d_err:.2f} units of 2^-24 * extent; closest t worst {t_err:.2f} units on "
          f"{int(same.sum())} rays, {int(differs.sum())} of {len(rays)} excluded (another winner)")
    assert same.sum() >= 150
    assert differs.sum() <= 0.02 * len(rays)
    assert d_err <= D_BOUND[name]
    assert t_err <= T_BOUND[name]


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Device:
    """device buffers of one Case and one method per entry point, each returning host copies"""

    def __init__(self, ctx, drawer, cs):
        lay = L()
        self.ctx, self.drawer = ctx, drawer
        self.n_rays, self.n_points = len(cs.rays), len(cs.points)
        self.buffers = []
        self.rays = self._upload(cs.rays, lay.RAY)
        self.points = self._upload(cs.points, lay.POINT_QUERY)
        self.cross_points = self._upload(cs.cross_points, lay.POINT_QUERY)
        self.boxes = self._upload(cs.boxes, lay.AABB)
        self.hits = self._new(self.n_rays * KMAX, lay.HIT)
        self.near = self._new(self.n_points * KMAX, lay.CLOSEST_POINT)
        self.flags = self._new(self.n_rays + self.n_points, np.uint32)

    def _new(self, size, dtype):
        self.buffers.append(H().DataBuffer(self.ctx, size, dtype))
        return self.buffers[-1]

    def _upload(self, data, dtype):
        buf = self._new(len(data), dtype)
        buf.local[:] = data
        buf.sync()
        return buf

    def _flags(self, call, queries, n):
        self.flags.fill_u32(0xDEADBEEF)
        call(queries, self.flags)
        return self.flags.get_data()[:n].copy()

    def closest(self):
        self.hits.fill_u32(0x7FC00000)
        self.drawer.trace_closest(self.rays, self.hits)
        return self.hits.get_data()[: self.n_rays].copy()

    def occluded(self):
        return self._flags(self.drawer.trace_occluded, self.rays, self.n_rays)

    def counts(self):
        return self._flags(self.drawer.count_hits, self.rays, self.n_rays)

    def crossings(self, dirs):
        return self._flags(lambda q, out: self.drawer.point_crossings(q, out, dirs), self.cross_points, self.cross_points.size)

    def k_hits(self, k):
        self.hits.fill_u32(0x7FC00000)
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.trace_k_closest(self.rays, k, self.hits, self.flags)
        got = self.hits.get_data().copy()
        assert (words(got[self.n_rays * k:]) == 0x7FC00000).all()
        return got[: self.n_rays * k].reshape(self.n_rays, k), self.flags.get_data()[: self.n_rays].copy()

    def gathered(self, device_sort):
        return self.drawer.all_hits(self.rays, device_sort=device_sort)

    def nearest(self):
        self.near.fill_u32(0x7FC00000)
        self.drawer.closest_points(self.points, self.near)
        return self.near.get_data()[: self.n_points].copy()

    def within(self):
        return self._flags(self.drawer.within_distance, self.points, self.n_points)

    def k_nearest(self, k):
        self.near.fill_u32(0x7FC00000)
        self.flags.fill_u32(0xDEADBEEF)
        self.drawer.k_closest_points(self.points, k, self.near, self.flags)
        got = self.near.get_data().copy()
        assert (words(got[self.n_points * k:]) == 0x7FC00000).all()
        return got[: self.n_points * k].reshape(self.n_points, k), self.flags.get_data()[: self.n_points].copy()

    def lists(self, queries, device_sort):
        return self.drawer.overlaps(queries, device_sort=device_sort)

    def dispose(self):
        for b in self.buffers:
            b.dispose()


def same_records(got, want, queries, what):
    bad = np.nonzero((words(got).reshape(len(want), -1) != words(want).reshape(len(want), -1)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:3]], want[bad[:3]], queries[bad[:3]])


def same_words(got, want, queries, what):
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:5]], want[bad[:5]], queries[bad[:3]])


def same_rows(got, found, ref, queries, what):
    bad = np.nonzero((row_words(got) != row_words(ref.records)).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], got[bad[:2]], ref.records[bad[:2]], queries[bad[:2]])
    same_words(found, ref.found, queries, what)


def same_lists(got, ref, queries, what):
    (go, gt), (ro, rt) = got, ref
    same_words(go, ro, queries, what)
    assert len(gt) == len(rt) == int(ro[-1]), what
    bad = np.nonzero(V.sort_segments(go, gt) != rt)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10])


def check_rays(dev, cs, what):
    same_records(dev.closest(), cs.ray.records, cs.rays, (what, "lbvh_trace_closest"))
    same_words(dev.occluded(), cs.ray.flags, cs.rays, (what, "lbvh_trace_occluded"))
    same_words(dev.counts(), cs.ray.counts, cs.rays, (what, "lbvh_count_hits"))


def check_crossings(dev, cs, what):
    same_words(dev.crossings(cs.dirs), cs.parity, cs.cross_points, (what, "lbvh_point_crossings"))


def check_k_hits(dev, cs, what, ks=KS):
    for k in ks:
        got, found = dev.k_hits(k)
        same_rows(got, found, KH.truncate(cs.khits, k), cs.rays, (what, "lbvh_trace_k_closest", k))


def check_gathered(dev, cs, what, device_sorts=(False, True)):
    for device_sort in device_sorts:                       # as the walk left the segments, and after lbvh_sort_hit_segments
        off, rec = dev.gathered(device_sort)
        same_words(off, cs.gather.offsets, cs.rays, (what, "lbvh_gather_hits offsets"))
        assert len(rec) == int(cs.gather.offsets[-1])
        got = rec if device_sort else G.canonical(off, rec)
        bad = np.nonzero((words(got).reshape(-1, 4) != words(cs.gather.records).reshape(-1, 4)).any(axis=1))[0]
        assert len(bad) == 0, (what, "lbvh_gather_hits", device_sort, len(bad), bad[:10], got[bad[:3]], cs.gather.records[bad[:3]])


def check_points(dev, cs, what):
    same_records(dev.nearest(), cs.point.records, cs.points, (what, "lbvh_closest_point_query"))
    same_words(dev.within(), cs.point.flags, cs.points, (what, "lbvh_within_distance"))


def check_k_nearest(dev, cs, what, ks=KS):
    for k in ks:
        got, found = dev.k_nearest(k)
        same_rows(got, found, KC.truncate(cs.kpoints, k), cs.points, (what, "lbvh_k_closest_points", k))


def check_overlaps(dev, cs, what, device_sorts=(False, True)):
    for device_sort in device_sorts:
        same_lists(dev.lists(dev.points, device_sort), cs.within, cs.points, (what, "lbvh_gather_within_distance", device_sort))
        same_lists(dev.lists(dev.boxes, device_sort), cs.overlap, cs.boxes, (what, "lbvh_box_overlaps", device_sort))


_DRAWERS = {}


def device_case(ctx, name):
    """(Case from the library's own boxes, Device): one drawer per scene, built once; one context keeps one derived traversal
    scene, so it is derived again for the test that asks"""
    if name not in _DRAWERS:
        tris = HS.scene(name)
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        _DRAWERS[name] = (d, case_of(name, library_boxes(d)))
    d, cs = _DRAWERS[name]
    d.build_fast_scene()
    return cs, Device(ctx, d, cs)


def finish(ctx, dev):
    dev.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0              # no fault word: no stack entry was dropped


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_closest_occluded_and_count_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_rays(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_crossing_parities_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_crossings(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_first_k_hits_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_k_hits(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_gathered_hits_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_gathered(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_closest_point_and_within_distance_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_points(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_k_nearest_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_k_nearest(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_overlap_lists_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_overlaps(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_every_entry_point_with_one_lds_stack_entry(ctx, name):
    """lbvh_debug_ray_stack_split(ctx, 1): all but one waiting sibling goes to the device-memory part of the stack.  The same
    words — on `one_cell` and `copies` (heavily overlapping boxes: the deepest stacks) as everywhere."""
    cs, dev = device_case(ctx, name)
    lib, h = N().lib, ctx.handle
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        what = (name, "stack split 1")
        check_rays(dev, cs, what)
        check_crossings(dev, cs, what)
        check_k_hits(dev, cs, what, ks=(3,))
        check_gathered(dev, cs, what, device_sorts=(False,))
        check_points(dev, cs, what)
        check_k_nearest(dev, cs, what, ks=(3,))
        check_overlaps(dev, cs, what, device_sorts=(False,))
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    finish(ctx, dev)
