"""The region family (lbvh_region_overlaps, lbvh_region_overlaps_any, lbvh_region_overlaps_large, lbvh_plane_sections) against its
brute-force restatements — tests/region_reference.py and tests/plane_section_reference.py, word for word — on the seven scenes of
tests/hostile_scenes.py.  Per scene one region set and one plane set; the references are computed once per scene.
  regions  600 of test_region_queries.mixed_regions (all eight kinds, seed 17) + the aimed ones of aimed_regions below (67 .. 103):
           the exact union box, that box one float smaller on each face, zero-volume boxes at stored vertices, triangles' own boxes,
           and per scene what the scene is hostile with
  planes   test_plane_sections.special_planes (77) + 400 of random_planes + the 59 or 60 of aimed_planes below, each with d from
           fp32_through, so that pv is exactly 0 at the vertex (or along the edge) it is aimed at

CPU (unmarked): what the references alone must meet so that no comparison is vacuous; the section reference against float64 on the
random planes (plane_section_reference.float64_check: K = 64, at most 1 % of the ends under the cosine floor); the region reference
against the header's P and N evaluated in float64 on the same fp32 words.
GPU: every entry point == its reference fed the library's own boxes, on poisoned output buffers, ending with lbvh_sync == 0:
    lbvh_region_overlaps        both modes: the offsets, d_tris after a host sort and after lbvh_sort_index_segments
    lbvh_region_overlaps_any    both modes: the flags, the words behind them untouched
    lbvh_region_overlaps_large  both modes under task caps 4, 64 and the default: the brute force, lbvh_region_overlaps' offsets,
                                two calls write the same bytes
    lbvh_plane_sections         task caps 4, 64 and the default: offsets and records (NaNs folded, sorted by tri), the record invariants
    all of them once more with the LDS part of the stack cut to one entry
    aabb_planes(box) in TOUCHING mode == lbvh_box_overlaps of the same box, for every aimed box: the tie to the family that
    tests/test_hostile_scenes.py holds (n = +-1 and 0: hi - q.lo >= 0 is q.lo <= hi for every pair of finite floats)"""
import numpy as np
import pytest

import hostile_scenes as HS
import overlap_reference as V
import plane_section_reference as PS
import region_reference as R
import test_plane_sections as PL
import test_region_queries as Q
from query_support import H, L, library_boxes, N, padded_boxes, positions, words

F = np.float32
INF = F(np.inf)
MODES = [R.TOUCHING, R.CONTAINED]
CAPS = [4, 64, 0]                                     # lbvh_debug_region_task_cap; 0: the host's choice
N_MIXED, N_RANDOM = 600, 400
N_VERTEX, N_OWN = 30, 30
UNION, SHRUNK, VERTEX, OWN, SCENE_BOX, SCENE_OBB = 8, 9, 10, 11, 12, 13          # the aimed kinds, after mixed_regions' 0 .. 7
POISON, GUARD = 0x7FC0DEAD, 64
INNER = 141.0                  # `outside`: no triangle with its centre inside +-125 reaches here (vertices within +-140, the pad)


# ---- the region sets ---------------------------------------------------------------------------------------------------------

def stratified(name, n, count, rng):
    """`count` triangle indices; on `slivers` a quarter of each kind: points and collinear triples are among them"""
    if name != "slivers":
        return rng.integers(0, n, count)
    kind = HS.sliver_kinds()
    return np.concatenate([rng.choice(np.nonzero(kind == k)[0], (count + 3 - k) // 4) for k in range(4)])


def scene_boxes(name, a, lo, hi, rng):
    """-> (qlo, qhi): the boxes aimed at what the scene is hostile with
    outside   per axis and side four boxes that begin at +-141 or beyond and reach past the last triangle, and twelve far triangles'
              own boxes cut at +-141: only triangles with a centre beyond +-125 can be inside
    one_cell  24 boxes with every face on a multiple of 2^-6 (half of them: of 2^-5) from the cube's corner, a third of them of zero
              thickness on one axis, and the cube of side 2^-4 itself
    fan       24 slabs about z = 2 (z ranges: exactly 2; 2 +- 2^-10; the boxes' top face alone; from the float above it; up to the
              boxes' bottom face; up to the float below it; [2, 3]; [1, 2]) over the whole fan, one quadrant and a random rectangle;
              the four quadrant boxes with a vertical edge through FAN_VERTEX"""
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    qlo, qhi = [], []
    if name == "outside":
        for axis in range(3):
            for sign in (1.0, -1.0):
                for part in range(4):
                    l, h = slo - F(1.0), shi + F(1.0)
                    other = [k for k in range(3) if k != axis]
                    if part in (1, 2):                               # the lower / upper half of another axis
                        (h if part == 1 else l)[other[part - 1]] = F(0.0)
                    start = F(INNER + (40.0 if part == 3 else 0.0))
                    if sign > 0:
                        l[axis] = start
                    else:
                        h[axis] = -start
                    qlo.append(l)
                    qhi.append(h)
        centre = (lo + hi) * F(0.5)
        reach = np.maximum(hi, -lo)
        far = np.nonzero((np.abs(centre) >= 125.0).any(axis=1) & (reach.max(axis=1) > INNER + 1.0))[0]
        for j in rng.choice(far, 12, replace=False):
            l, h = lo[j].copy(), hi[j].copy()
            axis = int(np.argmax(reach[j]))
            if h[axis] >= -l[axis]:
                l[axis] = max(l[axis], F(INNER))
            else:
                h[axis] = min(h[axis], F(-INNER))
            qlo.append(l)
            qhi.append(h)
    if name == "one_cell":
        corner = HS.ONE_CELL_CORNER
        i0 = rng.integers(0, 4, (24, 3))
        i1 = i0 + rng.integers(1, 5 - i0)
        i0[12:] = 2 * rng.integers(0, 2, (12, 3))                    # the second half on multiples of 2^-5: some hold whole triangles
        i1[12:] = i0[12:] + 2 * rng.integers(1, 3 - i0[12:] // 2)
        flat = np.arange(0, 24, 3)
        axis = rng.integers(0, 3, len(flat))
        i1[flat, axis] = i0[flat, axis]
        qlo += list((corner + i0 * 2.0 ** -6).astype(F)) + [corner.astype(F)]
        qhi += list((corner + i1 * 2.0 ** -6).astype(F)) + [(corner + 2.0 ** -4).astype(F)]
    if name == "fan":
        v = HS.FAN_VERTEX
        top, bottom = hi[0, 2], lo[0, 2]
        assert (hi[:, 2] == top).all() and (lo[:, 2] == bottom).all()
        zs = [(2.0, 2.0), (2.0 - 2.0 ** -10, 2.0 + 2.0 ** -10), (top, top), (np.nextafter(top, INF), 3.0), (1.0, bottom),
              (1.0, np.nextafter(bottom, -INF)), (2.0, 3.0), (1.0, 2.0)]
        for z0, z1 in zs:
            r0 = v[:2] + rng.integers(-40, 24, 2) / 8.0
            for (x0, y0), (x1, y1) in ((slo[:2], shi[:2]), (v[:2], v[:2] + F(4.0)), (r0, r0 + rng.integers(1, 32, 2) / 8.0)):
                qlo.append(np.array([x0, y0, z0], dtype=F))
                qhi.append(np.array([x1, y1, z1], dtype=F))
        for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            other = v[:2] + np.array([sx, sy], dtype=F) * F(3.0)
            qlo.append(np.append(np.minimum(v[:2], other), F(1.0)).astype(F))
            qhi.append(np.append(np.maximum(v[:2], other), F(3.0)).astype(F))
    return np.array(qlo, dtype=F).reshape(-1, 3), np.array(qhi, dtype=F).reshape(-1, 3)


def aimed_regions(name, a, b, c, lo, hi, rng):
    """-> (regions, kinds, qlo, qhi): built with the host's aabb_planes / obb_planes; qlo / qhi hold the box of every region made by
    aabb_planes and NaN for the others
    UNION      the exact union of the triangles' boxes          SHRUNK   that box one float smaller on one face, each of the six
    VERTEX     30 zero-volume boxes at stored vertices          OWN      30 boxes equal to one triangle's own box (`copies`: eight
               triangles' at once; `slivers`: a quarter each of points, collinear triples, needles and ordinary ones)
    SCENE_BOX  scene_boxes above                                 SCENE_OBB  `fan`: eight turned boxes with an edge through FAN_VERTEX"""
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    qlo, qhi, kinds = [slo], [shi], [UNION]
    for axis in range(3):
        up, down = slo.copy(), shi.copy()
        up[axis], down[axis] = np.nextafter(slo[axis], INF), np.nextafter(shi[axis], -INF)
        qlo += [up, slo]
        qhi += [shi, down]
        kinds += [SHRUNK, SHRUNK]
    k = stratified(name, len(a), N_VERTEX, rng)
    vert = np.stack([a, b, c])[rng.integers(0, 3, len(k)), k]
    k = stratified(name, len(a), N_OWN, rng)
    slo_, shi_ = scene_boxes(name, a, lo, hi, rng)
    qlo = np.concatenate([np.array(qlo), vert, lo[k], slo_]).astype(F)
    qhi = np.concatenate([np.array(qhi), vert, hi[k], shi_]).astype(F)
    kinds = np.array(kinds + [VERTEX] * len(vert) + [OWN] * len(k) + [SCENE_BOX] * len(slo_))
    regions = H().aabb_planes(qlo, qhi)
    if name == "fan":                                      # the edge where the faces +axis 0 and +axis 1 meet passes through the vertex
        rot = Q._rotations(rng, 8)
        half = rng.uniform(0.5, 6.0, (8, 3))
        centre = HS.FAN_VERTEX.astype(np.float64) - half[:, :1] * rot[:, 0] - half[:, 1:2] * rot[:, 1] + rng.uniform(-1.0, 1.0, (8, 1)) * rot[:, 2]
        regions = np.concatenate([regions, H().obb_planes(centre, rot, half)])
        kinds = np.concatenate([kinds, [SCENE_OBB] * 8])
        nan = np.full((8, 3), np.nan, dtype=F)
        qlo, qhi = np.concatenate([qlo, nan]), np.concatenate([qhi, nan])
    return regions, kinds, qlo, qhi


def region_set(name, a, b, c, lo, hi):
    """-> (regions, kinds, qlo, qhi): the mixed regions (kinds 0 .. 7) and the aimed ones, spread among them"""
    rng = np.random.default_rng(500 + len(a))
    mixed, kind, _ = Q.mixed_regions(a, b, c, lo, hi, count=N_MIXED, seed=17)
    aimed, akind, qlo, qhi = aimed_regions(name, a, b, c, lo, hi, rng)
    nan = np.full((N_MIXED, 3), np.nan, dtype=F)
    order = rng.permutation(N_MIXED + len(aimed))
    return (np.concatenate([mixed, aimed])[order], np.concatenate([kind, akind])[order], np.concatenate([nan, qlo])[order],
            np.concatenate([nan, qhi])[order])


# ---- the plane sets ----------------------------------------------------------------------------------------------------------

def tilts(rng, count):
    n = rng.normal(size=(count, 3))
    return (n * rng.uniform(0.25, 4.0, (count, 1)) / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def aimed_planes(name, a, b, c, rng):
    """-> (planes, labels); d = fp32_through(n, p): pv(p) == 0 exactly (a vertex b or c only where the line a + (b - a) gives it back)
    fan      "hub": 40 through FAN_VERTEX at random tilts; "flat": z = 2 itself, three ways (every s is 0: no candidate);
             "spoke": 16 upright planes that contain a shared edge (n = (e.y, -e.x, 0) for the edge e: exact)
    slivers  "point": 20 through the stored vertex of point triangles; "needle": 20 that contain the long edge of a needle as fp32
             has it (n = e x r rounded once; s is 0 at a, rounding noise at b); "line": 10 that contain a collinear triple (n = e x
             axis: exact, every s is 0) and "end": 10 through its end a alone
    others   "vertex": 60 through stored vertices at random tilts, two thirds through a (exact), the rest through b or c; on
             `copies` each is shared by eight triangles"""
    e1 = b - a
    if name == "fan":
        spoke = rng.integers(0, len(a), 16)
        n = np.concatenate([tilts(rng, 40), np.array([[0, 0, 1], [0, 0, -1], [0, 0, 4]], dtype=F),
                            np.stack([e1[spoke, 1], -e1[spoke, 0], np.zeros(16, dtype=F)], axis=1)])
        p = np.tile(HS.FAN_VERTEX, (len(n), 1))
        labels = ["hub"] * 40 + ["flat"] * 3 + ["spoke"] * 16
    elif name == "slivers":
        kind = HS.sliver_kinds()
        pick = lambda k, count: rng.choice(np.nonzero(kind == k)[0], count, replace=False)
        pt, nd, ln, en = pick(HS.POINT, 20), pick(HS.NEEDLE, 20), pick(HS.COLLINEAR, 10), pick(HS.COLLINEAR, 10)
        across = np.cross(e1[nd].astype(np.float64), rng.normal(size=(20, 3)))
        axis = np.eye(3)[np.argmin(np.abs(e1[ln]), axis=1)]          # (not along e: the cross product is not zero)
        n = np.concatenate([tilts(rng, 20), (across / np.linalg.norm(across, axis=1, keepdims=True)).astype(F),
                            np.cross(e1[ln].astype(np.float64), axis).astype(F), tilts(rng, 10)])
        p = np.concatenate([a[pt], a[nd], a[ln], a[en]])
        labels = ["point"] * 20 + ["needle"] * 20 + ["line"] * 10 + ["end"] * 10
    else:
        k = rng.integers(0, len(a), 60)
        corner = np.where(np.arange(60) < 40, 0, rng.integers(1, 3, 60))
        n, p, labels = tilts(rng, 60), np.stack([a, b, c])[corner, k], ["vertex"] * 60
    n, p = n.astype(F), p.astype(F)
    return PS.make_planes(n, PL.fp32_through(n, p)), np.array(labels)


def plane_set(name, a, b, c):
    """-> (planes, labels): special, then random, then aimed"""
    rng = np.random.default_rng(600 + len(a))
    special, rnd = PL.special_planes(a, b, c), PL.random_planes(a, b, c, N_RANDOM)
    aimed, labels = aimed_planes(name, a, b, c, rng)
    return np.concatenate([special, rnd, aimed]), np.concatenate([["special"] * len(special), ["random"] * len(rnd), labels])


class Case:
    """one scene, its region and plane sets and both references, from the given triangle boxes"""

    def __init__(self, name, lo, hi):
        self.name, self.tris = name, HS.scene(name)
        self.a, self.b, self.c = a, b, c = positions(self.tris)
        self.lo, self.hi = lo, hi
        self.regions, self.kind, self.qlo, self.qhi = region_set(name, a, b, c, lo, hi)
        self.region_ref = R.reference(self.regions, lo, hi)
        self.box_rows = np.nonzero(np.isfinite(self.qlo).all(axis=1))[0]
        self.boxes = V.make_boxes(self.qlo[self.box_rows], self.qhi[self.box_rows])
        self.planes, self.plane_labels = plane_set(name, a, b, c)
        self.sections = PS.reference(self.planes, a, b, c, lo, hi)

    def sizes(self, mode):
        return np.diff(self.region_ref[mode][0]).astype(np.int64)

    def section_sizes(self):
        return np.diff(self.sections.offsets).astype(np.int64)

    def sections_of(self, label):
        """the reference Result of the planes with this label alone (they are consecutive), and those planes"""
        rows = np.nonzero(self.plane_labels == label)[0]
        first, last = int(rows[0]), int(rows[-1]) + 1
        assert (np.diff(rows) == 1).all()
        keep = (self.sections.rows >= first) & (self.sections.rows < last)
        off = self.sections.offsets[first:last + 1] - self.sections.offsets[first]
        return PS.Result(off, self.sections.records[keep], self.sections.rows[keep] - first), self.planes[first:last]


_CASES = {}


def case_of(name, boxes=None):
    """the Case from the Morton stage's boxes as padded_boxes restates them (CPU), or from the library's own (GPU): the same
    object when they are the same words"""
    lo, hi = boxes if boxes is not None else padded_boxes(*positions(HS.scene(name)))
    key = (name, lo.tobytes(), hi.tobytes())
    if key not in _CASES:
        _CASES[key] = Case(name, lo, hi)
    return _CASES[key]


# ---- CPU: non-vacuity, on the references alone ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", HS.NAMES)
def test_the_references_are_not_vacuous(name):
    """The floors, per scene: TOUCHING non-empty for at least a third of the regions, CONTAINED for at least a tenth, at least a
    tenth empty (those of test_region_queries.check_not_vacuous); a region with 0 < CONTAINED < TOUCHING; every kind of
    mixed_regions at least 15 times; at least 20 regions that hold the whole scene; at least half the planes cut something; and
    what is asserted per scene below.  Reached (TOUCHING / CONTAINED non-empty, empty; regions with 0 < C < T; whole-scene regions;
    the rarest mixed kind; planes that cut; records):
      pair      83 % / 36 %, 17 %; 110; 479; 28; 85 %;    730
      triple    80 % / 36 %, 20 %; 159; 386; 26; 89 %;    865
      one_cell  82 % / 56 %, 18 %; 346; 135; 28; 96 %; 32 687
      copies    82 % / 52 %, 18 %; 300;  78; 25; 93 %; 31 656; every segment length a multiple of 8
      outside   83 % / 60 %, 17 %; 349;  29; 18; 96 %;  4 646; 216 regions whose TOUCHING list holds out-of-box triangles alone
      slivers   82 % / 67 %, 18 %; 417;  67; 34; 94 %; 15 965: none on a point, 6 177 on collinear triples, 4 812 on needles
      fan       77 % / 44 %, 23 %; 247; 362; 25; 93 %; 12 580; z = 2 cuts nothing, three times; each of the 40 planes through
                FAN_VERTEX has 34 records (the longest segment of the scene), each of the 16 along a shared edge 32"""
    cs = case_of(name)
    n = len(cs.tris)
    t, c = cs.sizes(R.TOUCHING), cs.sizes(R.CONTAINED)
    cut = cs.section_sizes()
    counts = np.bincount(cs.kind, minlength=14)
    print(f"{name}: {len(cs.regions)} regions, TOUCHING {100 * (t > 0).mean():.0f} % non-empty, CONTAINED {100 * (c > 0).mean():.0f} %, "
          f"empty {100 * (t == 0).mean():.0f} %, 0 < C < T in {int(((c > 0) & (c < t)).sum())}, whole scene {int((t == n).sum())}, "
          f"kinds {counts.tolist()}; {len(cs.planes)} planes, {100 * (cut > 0).mean():.0f} % cut, {len(cs.sections.records)} records, "
          f"longest segment {int(cut.max())}")
    assert 60 <= len(cs.regions) - N_MIXED <= 110 and 50 <= (cs.plane_labels != "special").sum() - N_RANDOM <= 70 and len(cs.planes) < 600
    assert (t > 0).mean() >= 1.0 / 3.0 and (c > 0).mean() >= 0.1 and (t == 0).mean() >= 0.1
    assert (c <= t).all() and ((c > 0) & (c < t)).any()
    assert (counts[:8] >= 15).all() and counts[UNION] == 1 and counts[SHRUNK] == 6 and counts[VERTEX] == N_VERTEX and counts[OWN] == N_OWN
    assert (t == n).sum() >= 20
    assert (cut > 0).mean() >= 0.5
    # the aimed regions do what they are aimed at: the union box holds everything in both modes; one float less on a face still
    # touches everything and no longer contains all; a triangle's own box contains it; a stored vertex is inside its triangle's box
    assert t[cs.kind == UNION] == n and c[cs.kind == UNION] == n
    assert (t[cs.kind == SHRUNK] == n).all() and (c[cs.kind == SHRUNK] < n).all()
    assert (c[cs.kind == OWN] >= 1).all() and (t[cs.kind == VERTEX] >= 1).all()
    PL.check_records(cs.sections.records)
    # aimed planes: s is exactly 0 at the vertex aimed at (vertex a of a triangle, as the triangle line holds it)
    aimed = np.nonzero(~np.isin(cs.plane_labels, ("special", "random", "vertex")))[0]
    on = (PS.pv(cs.planes[aimed][:, None], cs.a[None]) == 0).any(axis=1)
    assert on.all(), (name, cs.plane_labels[aimed][~on])
    if name == "copies":
        assert (t % 8 == 0).all() and (c % 8 == 0).all() and (cut % 8 == 0).all()
        assert (t[cs.kind == OWN] >= 8).all() and (cut[cs.plane_labels == "vertex"] >= 8).sum() >= 30
    if name == "slivers":
        kind = HS.sliver_kinds()
        named = np.bincount(kind[cs.sections.records["tri"]], minlength=4)
        print(f"slivers: records per kind {named.tolist()}")
        assert named[HS.POINT] == 0 and named[HS.COLLINEAR] >= 1000 and named[HS.NEEDLE] >= 1000
        # own boxes of points and collinear triples are in the region set, and a plane that contains a collinear triple cuts it nowhere
        own = cs.box_rows[cs.kind[cs.box_rows] == OWN]
        flat = (cs.qhi[own] - cs.qlo[own] < F(0.0021)).all(axis=1)                 # a point's box: the pad alone
        assert flat.sum() >= 5
        for k in np.nonzero(cs.plane_labels == "line")[0]:
            seg = cs.sections.records["tri"][int(cs.sections.offsets[k]):int(cs.sections.offsets[k + 1])]
            s = PS.pv(cs.planes[k], np.stack([cs.a, cs.b, cs.c], axis=1))                      # [triangles, 3 vertices]
            whole = np.nonzero((s == 0).all(axis=1) & (kind == HS.COLLINEAR))[0]
            assert len(whole) >= 1 and not np.isin(whole, seg).any()
    if name == "fan":
        flat = np.nonzero(cs.plane_labels == "flat")[0]
        hub = cut[cs.plane_labels == "hub"]
        print(f"fan: z = 2 cuts {cut[flat].tolist()}, planes through FAN_VERTEX cut {int(hub.min())} .. {int(hub.max())}, "
              f"spokes {int(cut[cs.plane_labels == 'spoke'].min())} .. {int(cut[cs.plane_labels == 'spoke'].max())}")
        assert (cut[flat] == 0).all() and (hub >= 2).sum() >= 10
        assert (t[cs.kind == SCENE_OBB] > 0).sum() >= 4
    if name == "outside":
        centre = (cs.lo + cs.hi) * F(0.5)
        far = (np.abs(centre) >= 125.0).any(axis=1)
        assert (far == (np.arange(n) % 2 == 1)).all()
        off, tris = cs.region_ref[R.TOUCHING]
        only = np.array([t[k] > 0 and far[tris[int(off[k]):int(off[k + 1])]].all() for k in range(len(t))])
        print(f"outside: {int(only.sum())} regions whose TOUCHING list holds out-of-box triangles alone")
        assert only.sum() >= 20 and only[cs.kind == SCENE_BOX].sum() >= 20
    if name == "one_cell":
        scene = cs.box_rows[cs.kind[cs.box_rows] == SCENE_BOX]
        steps = (cs.qlo[scene].astype(np.float64) - HS.ONE_CELL_CORNER) * 64.0
        assert (steps == np.round(steps)).all() and (t[scene] > 0).sum() >= 20 and ((c[scene] > 0) & (c[scene] < t[scene])).sum() >= 5


# ---- CPU: the section reference against float64 ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", HS.NAMES)
def test_the_section_reference_agrees_with_float64_on_the_random_planes(name):
    """plane_section_reference.float64_check on the 400 random planes: every end within the module's derived bound (ratio <= 1 with
    K = 64) and at most 1 % of the ends left out under its |cos| floor.  Reached (worst ratio; ends left out of all):
      pair 0.019, 0 of 1 098       triple 0.019, 0 of 1 276        one_cell 0.022, 43 of 47 814      copies 0.013, 40 of 46 192
      outside 0.011, 7 of 6 428    slivers 0.010, 11 of 20 928     fan 0.015, 80 of 19 212"""
    cs = case_of(name)
    ref, planes = cs.sections_of("random")
    assert len(planes) == N_RANDOM and int(ref.offsets[-1]) == len(ref.records)
    ratio, out = PS.float64_check(planes, cs.a, cs.b, cs.c, ref)
    print(f"{name}: {len(ref.records)} records on the random planes, worst ratio {ratio.max():.3f}, {int(out.sum())} of {out.size} ends left out")
    assert len(ref.records) >= 300
    assert out.mean() <= 0.01
    assert (ratio <= 1.0).all()


# ---- CPU: the region reference against float64 -----------------------------------------------------------------------------

def corner_values64(planes, lo, hi):
    """the header's P and N in float64 on the same fp32 words: planes [regions, 6, 4], boxes [triangles, 3] -> [regions, 6, triangles]"""
    n, d = planes[:, :, None, :3].astype(np.float64), planes[:, :, None, 3].astype(np.float64)
    lo, hi = lo.astype(np.float64)[None, None], hi.astype(np.float64)[None, None]
    with np.errstate(all="ignore"):
        pos = n >= 0.0
        far, near = np.where(pos, hi, lo), np.where(pos, lo, hi)
        return (n * far).sum(axis=3) + d, (n * near).sum(axis=3) + d


@pytest.mark.parametrize("name", HS.NAMES)
def test_the_region_reference_agrees_with_float64(name):
    """P and N of include/lbvh.h are three products and three sums, each rounded once: a term passes through at most four roundings, so
    fp32 and float64 differ by at most 4 * 2^-24 * (|n|_1 * extent + |d|), extent = the largest absolute box coordinate of the scene.
    On every region of the set (the aimed ones included) the verdict P >= 0, N >= 0 of the fp32 restatement may differ from the
    float64 one only where the float64 value lies in that band; a plane with a non-finite word gives the same verdict in both.
    The share of (region, triangle) pairs with any of their twelve values in the band is at most 1 % on the mixed regions without
    kind 5 (faces placed exactly on a box face) — the aimed regions are left out of the SHARE for the same reason: they put faces
    exactly on box faces on purpose.  Reached (share in the band; verdicts that differ inside it):
      pair 0.000 %, 0     triple 0.000 %, 0     one_cell 0.300 %, 10    copies 0.000 %, 0     outside 0.001 %, 0
      slivers 0.000 %, 0  fan 0.000 %, 0
    (with kind 5 and the aimed regions counted too: 6.7 %, 5.0 %, 0.4 %, 0.4 %, 0.1 %, 0.1 %, 9.5 %)"""
    cs = case_of(name)
    planes = cs.regions["plane"]
    P32, N32 = R.corner_values(planes[:, :, None, :], cs.lo[None, None], cs.hi[None, None])
    P64, N64 = corner_values64(planes, cs.lo, cs.hi)
    extent = float(max(np.abs(cs.lo).max(), np.abs(cs.hi).max()))
    with np.errstate(all="ignore"):
        band = 4.0 * 2.0 ** -24 * (np.abs(planes[..., :3].astype(np.float64)).sum(axis=2) * extent + np.abs(planes[..., 3].astype(np.float64)))
    finite = np.isfinite(planes).all(axis=2)                                        # [regions, 6]
    differ, inside = 0, np.zeros(P64.shape[::2], dtype=bool)
    for v32, v64 in ((P32, P64), (N32, N64)):
        with np.errstate(invalid="ignore"):
            d = (v32 >= 0) != (v64 >= 0)
            near = np.abs(v64) <= band[:, :, None]
        assert not (d & ~finite[:, :, None]).any()
        assert not (d & ~near).any(), (name, np.argwhere(d & ~near)[:5])
        differ += int(d.sum())
        inside |= (near & finite[:, :, None]).any(axis=1)
    counted = (cs.kind < 8) & (cs.kind != 5)
    share = inside[counted].mean()
    print(f"{name}: extent {extent:.4g}; {100 * share:.3f} % of {int(counted.sum())} x {len(cs.tris)} pairs in the band "
          f"({100 * inside.mean():.3f} % with kind 5 and the aimed regions); {differ} verdicts differ, all inside it")
    assert counted.sum() >= 500
    assert share <= 0.01


# ---- GPU -------------------------------------------------------------------------------------------------------------------

class Device:
    """device buffers of one Case with GUARD entries behind each output, and one method per entry point, each on poisoned outputs
    and returning host copies"""

    def __init__(self, ctx, drawer, cs):
        lay = L()
        self.ctx, self.drawer, self.cs = ctx, drawer, cs
        self.buffers = []
        self.regions = self._upload(cs.regions, lay.REGION)
        self.planes = self._upload(cs.planes, lay.PLANE)
        self.boxes = self._upload(cs.boxes, lay.AABB)
        self.box_regions = self._upload(cs.regions[cs.box_rows], lay.REGION)
        most = max(len(cs.regions), len(cs.planes))
        self.offsets = self._new(most + 1 + GUARD, np.uint64)
        self.flags = self._new(len(cs.regions) + GUARD, np.uint32)
        self.tris = [self._new(int(cs.region_ref[R.TOUCHING][0][-1]) + GUARD, np.uint32) for _ in range(2)]
        self.segments = self._new(len(cs.sections.records) + GUARD, lay.PLANE_SEGMENT)

    def _new(self, size, dtype):
        self.buffers.append(H().DataBuffer(self.ctx, size, dtype))
        return self.buffers[-1]

    def _upload(self, data, dtype):
        buf = self._new(len(data), dtype)
        buf.local[:] = data
        buf.sync()
        return buf

    def _offsets(self, count):
        got = self.offsets.get_data().copy()
        assert (words(got[count + 1:]) == POISON).all()
        return got[:count + 1]

    def lists(self, mode, large=False, device_sort=False, which=0):
        """-> (offsets, d_tris up to the total as the call left them — or as lbvh_sort_index_segments did); the tail keeps the poison"""
        buf, count = self.tris[which], self.regions.size
        self.offsets.fill_u32(POISON)
        buf.fill_u32(POISON)
        (self.drawer.region_overlaps_large if large else self.drawer.region_overlaps)(self.regions, mode, self.offsets, buf)
        if device_sort:
            H().sort_index_segments(self.ctx, self.offsets, buf, count)
        off = self._offsets(count)
        got = buf.get_data().copy()
        total = int(off[-1])
        assert total <= buf.size - GUARD and (got[total:] == POISON).all()
        return off, got[:total]

    def any(self, mode):
        self.flags.fill_u32(POISON)
        self.drawer.region_overlaps_any(self.regions, mode, self.flags)
        got = self.flags.get_data().copy()
        assert (got[self.regions.size:] == POISON).all()
        return got[:self.regions.size]

    def sections(self):
        """-> (offsets, records as the call left them); the tail keeps the poison"""
        count = self.planes.size
        self.offsets.fill_u32(POISON)
        self.segments.fill_u32(POISON)
        self.drawer.plane_sections(self.planes, self.offsets, self.segments)
        off = self._offsets(count)
        got = self.segments.get_data().copy()
        total = int(off[-1])
        assert total <= self.segments.size - GUARD and (words(got[total:]) == POISON).all()
        return off, got[:total]

    def dispose(self):
        for b in self.buffers:
            b.dispose()


def same_lists(got, ref, what, sort=True):
    (go, gt), (ro, rt) = got, ref
    bad = np.nonzero(go != ro)[0]
    assert len(bad) == 0, (what, "offsets", len(bad), bad[:10], go[bad[:5]], ro[bad[:5]])
    assert len(gt) == len(rt) == int(ro[-1]), (what, len(gt), len(rt))
    bad = np.nonzero((V.sort_segments(go, gt) if sort else gt) != rt)[0]
    assert len(bad) == 0, (what, len(bad), bad[:10], gt[bad[:10]], rt[bad[:10]])


def check_lists(dev, cs, what, device_sorts=(False, True)):
    for mode in MODES:
        for device_sort in device_sorts:                   # sorted on the host, and by lbvh_sort_index_segments
            got = dev.lists(mode, device_sort=device_sort)
            same_lists(got, cs.region_ref[mode], (what, "lbvh_region_overlaps", mode, device_sort), sort=not device_sort)


def check_any(dev, cs, what):
    for mode in MODES:
        want = (cs.sizes(mode) > 0).astype(np.uint32)
        bad = np.nonzero(dev.any(mode) != want)[0]
        assert len(bad) == 0, (what, "lbvh_region_overlaps_any", mode, len(bad), bad[:10], cs.kind[bad[:10]])


def check_large(dev, cs, what, caps=CAPS):
    lib, h = N().lib, dev.ctx.handle
    plain = {mode: dev.lists(mode)[0] for mode in MODES}
    for cap in caps:
        N().check(h, lib.lbvh_debug_region_task_cap(h, cap))
        try:
            for mode in MODES:
                first = dev.lists(mode, large=True, which=0)
                second = dev.lists(mode, large=True, which=1)
                same_lists(first, cs.region_ref[mode], (what, "lbvh_region_overlaps_large", cap, mode))
                assert (words(first[0]) == words(plain[mode])).all(), (what, cap, mode, "the offsets of lbvh_region_overlaps")
                assert (first[0] == second[0]).all() and (first[1] == second[1]).all(), (what, cap, mode, "two calls, other bytes")
        finally:
            N().check(h, lib.lbvh_debug_region_task_cap(h, 0))


def check_sections(dev, cs, what, caps=CAPS):
    lib, h = N().lib, dev.ctx.handle
    ref = cs.sections
    for cap in caps:
        N().check(h, lib.lbvh_debug_region_task_cap(h, cap))
        try:
            off, rec = dev.sections()
        finally:
            N().check(h, lib.lbvh_debug_region_task_cap(h, 0))
        bad = np.nonzero(off != ref.offsets)[0]
        assert len(bad) == 0, (what, "lbvh_plane_sections offsets", cap, len(bad), bad[:10], cs.plane_labels[bad[:10]])
        assert len(rec) == len(ref.records)
        got = PS.sort_segments(off, rec)
        bad = np.nonzero((PS.record_words(got) != PS.record_words(ref.records)).any(axis=1))[0]
        assert len(bad) == 0, (what, "lbvh_plane_sections", cap, len(bad), bad[:10], got[bad[:3]], ref.records[bad[:3]],
                               cs.plane_labels[ref.rows[bad[:3]]])
        PL.check_records(rec)


def check_boxes(dev, cs, what):
    """aabb_planes(box), TOUCHING == lbvh_box_overlaps of the same box == both brute forces"""
    boff, btris = dev.drawer.overlaps(dev.boxes, device_sort=True)
    roff, rtris = dev.drawer.in_regions(dev.box_regions, R.TOUCHING, device_sort=True)
    want = V.box_overlaps(cs.boxes, cs.lo, cs.hi)
    same_lists((boff, btris), want, (what, "lbvh_box_overlaps"), sort=False)
    same_lists((roff, rtris), want, (what, "aabb_planes against lbvh_box_overlaps"), sort=False)
    sub = R.reference(cs.regions[cs.box_rows], cs.lo, cs.hi)[R.TOUCHING]
    same_lists((roff, rtris), sub, (what, "aabb_planes against the region reference"), sort=False)
    assert int(want[0][-1]) > len(cs.boxes) // 2


_DRAWERS = {}


def device_case(ctx, name):
    """(Case from the library's own boxes, Device): one drawer per scene, built once; one context keeps one derived traversal
    scene, so it is derived again for the test that asks"""
    if name not in _DRAWERS:
        d = H().RaytracingMeshDrawer(ctx, HS.scene(name)).awake()
        _DRAWERS[name] = (d, case_of(name, library_boxes(d)))
    d, cs = _DRAWERS[name]
    d.build_fast_scene()
    return cs, Device(ctx, d, cs)


def finish(ctx, dev):
    dev.dispose()
    assert N().lib.lbvh_sync(ctx.handle) == 0              # no fault word: no stack entry was dropped


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_region_lists_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_lists(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_region_flags_equal_the_brute_force(ctx, name):
    cs, dev = device_case(ctx, name)
    check_any(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_large_region_lists_equal_the_brute_force_under_every_task_cap(ctx, name):
    """`one_cell`, `copies` and `outside` are where the expansion into subtree tasks meets a tree split by index alone, eight equal
    leaves in a row and long leaf runs at the ends of the curve"""
    cs, dev = device_case(ctx, name)
    check_large(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_plane_sections_equal_the_restatement_under_every_task_cap(ctx, name):
    cs, dev = device_case(ctx, name)
    check_sections(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_axis_aligned_regions_equal_box_overlaps(ctx, name):
    cs, dev = device_case(ctx, name)
    check_boxes(dev, cs, name)
    finish(ctx, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("name", HS.NAMES)
def test_every_entry_point_with_one_lds_stack_entry(ctx, name):
    """lbvh_debug_ray_stack_split(ctx, 1): all but one waiting sibling goes to the device-memory part of the stack.  The same words."""
    cs, dev = device_case(ctx, name)
    lib, h = N().lib, ctx.handle
    N().check(h, lib.lbvh_debug_ray_stack_split(h, 1))
    try:
        what = (name, "stack split 1")
        check_lists(dev, cs, what, device_sorts=(False,))
        check_any(dev, cs, what)
        check_large(dev, cs, what, caps=(4, 0))
        check_sections(dev, cs, what, caps=(4, 0))
    finally:
        N().check(h, lib.lbvh_debug_ray_stack_split(h, 16))
    finish(ctx, dev)
