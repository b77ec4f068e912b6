"""CPU restatement of the box casts of include/lbvh.h (lbvh_box_cast, lbvh_box_cast_any): numpy float32, one rounded operation per
step, brute force over every (cast, triangle) pair — no tree.  A helper module, not a test file.  The slab test is
ray_reference.box_entry, imported, not written again; what is here is the header's own text: the thirteen axes in their order, the
interval of each, the entry / exit rule, the grown box, the accept rule, the tie rule.

    box_time(o, d, bx, by, bz, a, e1, e2)  -> (t, axis): the time with one scene triangle (+inf: none) and the axis that gave it
    grown_entry(casts, lo, hi)             (passes, entry) of every cast's ray against every box grown by g
    reference(casts, a, b, c, box_lo, box_hi) -> Result(records, flags, ties, valid, rejected)
    nearest(casts, a, b, c)                the least time below T over all triangles with no box rule, its triangle and axis
    driver_casts(lo, hi, count, seed, half_extent, t_max)   the casts `lbvh_driver boxcast` generates

`reference` takes the triangles' positions and their OWN boxes (the library's scene.triangle_aabb).  Every pair gets the slab test
of the grown box; the time is evaluated for the pairs that pass it, and for all pairs when `count_rule` asks for the accept rule's
statistics.  The kernel leaves its loop over the axes early; this module never does (the header's rule is over all thirteen)."""
from collections import namedtuple

import numpy as np

import ray_reference as RR
from unitysimpleraytracing_amd.layouts import BOX_AXIS_START, BOX_HIT, BOX_RAY, MAX_FLOAT

F = np.float32
MISS = np.array([(MAX_FLOAT, 0, 0, 0)], dtype=BOX_HIT)[0]

Result = namedtuple("Result", "records flags ties valid rejected")


def make_casts(centre, direction, ax, ay, az, t_max=F(np.inf)):
    c = np.zeros(len(centre), dtype=BOX_RAY)
    c["centre"], c["dir"], c["ax"], c["ay"], c["az"], c["t_max"] = centre, direction, ax, ay, az, t_max
    return c


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], axis=-1)


def active(casts):
    with np.errstate(all="ignore"):
        d = casts["dir"].astype(F)
        det = _dot(casts["ax"], _cross(casts["ay"], casts["az"]))
        return (casts["t_max"] > 0) & ~np.isnan(casts["centre"]).any(axis=1) & np.isfinite(d).all(axis=1) & (_dot(d, d) > 0) & \
            np.isfinite(casts["ax"]).all(axis=1) & np.isfinite(casts["ay"]).all(axis=1) & np.isfinite(casts["az"]).all(axis=1) & \
            np.isfinite(det) & (det != 0)


def limit(casts):
    """T = min(t_max, LBVH_MAX_FLOAT)"""
    return np.minimum(casts["t_max"], MAX_FLOAT)


def axes_of(bx, by, bz, e1, e2):
    """[(P_j, Q_j) for j = 0 .. 12]: L_j = cross(P_j, Q_j)"""
    with np.errstate(all="ignore"):
        edges = (e1, e2, e2 - e1)
    return [(e1, e2), (by, bz), (bz, bx), (bx, by)] + [(b, e) for b in (bx, by, bz) for e in edges]


def box_time(o, d, bx, by, bz, a, e1, e2):
    """rows of pairs, every argument (n, 3) float32 -> (t, axis)"""
    for x in (o, d, bx, by, bz, a, e1, e2):
        assert x.dtype == F
    n = len(o)
    enter = np.zeros(n, dtype=F)
    leave = np.full(n, np.inf, dtype=F)
    axis = np.full(n, BOX_AXIS_START, dtype=np.int64)
    none = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        m = a - o
        for j, (p, q) in enumerate(axes_of(bx, by, bz, e1, e2)):
            line = _cross(p, q)
            p0 = _dot(m, line)
            p1 = p0 + _dot(e1, line)
            p2 = p0 + _dot(e2, line)
            lo = np.fmin(p0, np.fmin(p1, p2))
            hi = np.fmax(p0, np.fmax(p1, p2))
            rb = (np.abs(_dot(bx, line)) + np.abs(_dot(by, line))) + np.abs(_dot(bz, line))
            v = _dot(d, line)
            pos, neg = v > 0, v < 0
            under, over = lo - rb, hi + rb
            tin = np.where(pos, under, over) / v
            tout = np.where(pos, over, under) / v
            moving = pos | neg
            none |= ~moving & ~((lo <= rb) & (-rb <= hi))
            later = moving & (tin > enter)
            enter = np.where(later, tin, enter)
            axis = np.where(later, j, axis)
            leave = np.where(moving & (tout < leave), tout, leave)
        t = np.where(~none & (enter <= leave), enter, F(np.inf))
    assert t.dtype == F and not np.isnan(t).any()
    return t, axis


def grown_entry(casts, lo, hi):
    """(passes, entry), each (casts, triangles): the walkers' slab test against lo - g, hi + g, g = (|ax| + |ay|) + |az|"""
    with np.errstate(all="ignore"):
        inv = F(1) / casts["dir"].astype(F)
        g = ((np.abs(casts["ax"]) + np.abs(casts["ay"])) + np.abs(casts["az"]))[:, None, :]
        return RR.box_entry(casts["centre"][:, None, :], inv[:, None, :], lo[None] - g, hi[None] + g)


def _pairs(sub, qi, ti, a, e1, e2):
    return box_time(sub["centre"][qi], sub["dir"][qi], sub["ax"][qi], sub["ay"][qi], sub["az"][qi], a[ti], e1[ti], e2[ti])


def reference(casts, a, b, c, box_lo, box_hi, casts_per_chunk=256, count_rule=False):
    """Brute force in float32.  casts: BOX_RAY array; a, b, c: (T, 3) positions; box_lo, box_hi: (T, 3) the triangles' own boxes.
    records: the candidate with the least t, ties to the lower index, or the miss record; flags: 1 where a candidate exists; ties:
    how many candidates share the least t.
    count_rule: also evaluate the pairs that fail the grown-box test; valid = the (active cast, triangle) pairs with a time in
    [0, T), rejected = those of them that miss the grown box or have t < entry."""
    assert casts.dtype == BOX_RAY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    lo, hi = np.ascontiguousarray(box_lo, dtype=F), np.ascontiguousarray(box_hi, dtype=F)
    e1, e2 = b - a, c - a
    n = len(casts)
    records = np.empty(n, dtype=BOX_HIT)
    records[:] = MISS
    flags = np.zeros(n, dtype=np.uint32)
    ties = np.zeros(n, dtype=np.uint32)
    valid = rejected = 0
    act = active(casts)
    big = limit(casts)
    for first in range(0, n, casts_per_chunk):
        sel = np.nonzero(act[first:first + casts_per_chunk])[0] + first
        if len(sel) == 0:
            continue
        sub = casts[sel]
        passes, entry = grown_entry(sub, lo, hi)
        qi, ti = np.nonzero(np.ones_like(passes) if count_rule else passes)
        t, axis = _pairs(sub, qi, ti, a, e1, e2)
        with np.errstate(invalid="ignore"):
            timed = t < big[sel][qi]
            cand = timed & passes[qi, ti] & ~(t < entry[qi, ti])
        valid += int(timed.sum())
        rejected += int((timed & ~cand).sum())
        key = np.full(passes.shape, F(np.inf))
        key[qi[cand], ti[cand]] = t[cand]
        pair = np.full(passes.shape, -1, dtype=np.int64)
        pair[qi, ti] = np.arange(len(qi))
        k = key.argmin(axis=1)                                 # the first (lowest-index) minimum
        rows = np.arange(len(sel))
        has = np.isfinite(key[rows, k])
        hit, kh = sel[has], k[has]
        th = key[rows, k][has]
        records["t"][hit], records["tri"][hit], records["axis"][hit] = th, kh, axis[pair[rows, k][has]]
        flags[hit] = 1
        ties[hit] = (key[has] == th[:, None]).sum(axis=1)
    return Result(records, flags, ties, valid, rejected)


def nearest(casts, a, b, c, casts_per_chunk=32):
    """(t, tri, axis): the least time below T over all triangles in float32 with no box rule, the lowest index on a tie; t = +inf
    where there is none"""
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    e1, e2 = b - a, c - a
    n, nt = len(casts), len(a)
    out = np.full(n, np.inf, dtype=F)
    tri = np.zeros(n, dtype=np.int64)
    axis_out = np.zeros(n, dtype=np.int64)
    act = active(casts)
    big = limit(casts)
    for first in range(0, n, casts_per_chunk):
        sel = np.nonzero(act[first:first + casts_per_chunk])[0] + first
        if len(sel) == 0:
            continue
        qi, ti = np.repeat(np.arange(len(sel)), nt), np.tile(np.arange(nt), len(sel))
        t, axis = _pairs(casts[sel], qi, ti, a, e1, e2)
        t = np.where(t < big[sel][qi], t, F(np.inf)).reshape(len(sel), nt)
        k = t.argmin(axis=1)
        out[sel], tri[sel], axis_out[sel] = t[np.arange(len(sel)), k], k, axis.reshape(len(sel), nt)[np.arange(len(sel)), k]
    return out, tri, axis_out


# ---- the casts of `lbvh_driver boxcast [seed] [half_extent] [t_max] [n_casts]`: SplitMix64, every draw a scalar fp32 operation in
# the C++ order

def driver_casts(lo, hi, count, seed=3, half_extent=1.5, t_max=2.0):
    """per cast and axis k: the centre around the mesh's box and the target inside it (as query_support.driver_rays), then component
    k of ax, ay, az: half_extent on the diagonal plus uniform in [-half_extent / 2, half_extent / 2]"""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    half = F(half_extent)
    casts = np.zeros(count, dtype=BOX_RAY)
    for i in range(count):
        for k in range(3):
            grow = F(0.25) * F(hi[k] - lo[k])
            casts["centre"][i, k] = uni(F(lo[k] - grow), F(hi[k] + grow))
            casts["dir"][i, k] = F(uni(lo[k], hi[k]) - casts["centre"][i, k])
            for j, name in enumerate(("ax", "ay", "az")):
                casts[name][i, k] = F((half if j == k else F(0)) + uni(F(-0.5) * half, F(0.5) * half))
    casts["t_max"] = F(t_max)
    return casts
