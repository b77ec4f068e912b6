"""CPU restatement of the capsule casts of include/lbvh.h (lbvh_capsule_cast, lbvh_capsule_cast_any): numpy float32, one rounded
operation per step, brute force over every (cast, triangle) pair — no tree.  A helper module, not a test file.  Nothing of the
arithmetic is written again here: the time against one derived triangle is sweep_reference.contact_time, the barycentrics are
point_reference.point_triangle, the pierce is triangle_query_reference.pierce (its t, which that function does not return, is
ray_reference.ray_triangle's: the same operations, test_capsule_cast.py checks that the two agree).  What is here is the header's
own text: the derived triangles, the order of j, the pierce rule, the grown box, the accept rule, the tie rule, s and (u, v).

    derived(a, e1, e2, h)                  the eight (a_j, e1_j, e2_j) of the header
    capsule_time(o, d, r, h, a, e1, e2)    -> (t, which, t_p): the time with one scene triangle (+inf: none), the derived triangle
                                           that gave it (8: the pierce) and the pierce's parameter
    contact(o, d, t, h, a, e1, e2, which, t_p)  -> (s, u, v) of a taken candidate
    grown_entry(casts, lo, hi)             (passes, entry) of every cast's ray against every box grown by the axis and the radius
    reference(casts, a, b, c, box_lo, box_hi) -> Result(records, flags, ties, valid, rejected, which, s)
    nearest(casts, a, b, c)                the least time below T over all triangles with no box rule, its triangle, j and s
    driver_casts(lo, hi, count, seed, radius, height)   the casts `lbvh_driver capsule` generates

`reference` takes the triangles' positions and their OWN boxes (the library's scene.triangle_aabb).  Every pair gets the slab test
of the grown box; the time is evaluated for the pairs that pass it, and for all pairs when `count_rule` asks for the accept rule's
statistics."""
from collections import namedtuple

import numpy as np

import point_reference as P
import ray_reference as RR
import sweep_reference as S
import triangle_query_reference as TQ
from unitysimpleraytracing_amd.layouts import CAPSULE_RAY, HIT, MAX_FLOAT

F = np.float32
MISS = S.MISS
PIERCE = 8

Result = namedtuple("Result", "records flags ties valid rejected which s")


def make_casts(origin, direction, radius, axis, t_max=F(np.inf)):
    c = np.zeros(len(origin), dtype=CAPSULE_RAY)
    c["origin"], c["dir"], c["radius"], c["axis"], c["t_max"] = origin, direction, radius, axis, t_max
    return c


def as_spheres(casts, radius=None):
    """the lbvh_sphere_ray records of the same origins and directions"""
    s = np.zeros(len(casts), dtype=S.SPHERE_RAY)
    s["origin"], s["dir"], s["t_max"] = casts["origin"], casts["dir"], casts["t_max"]
    s["radius"] = casts["radius"] if radius is None else radius
    return s


def active(casts):
    return S.active(as_spheres(casts)) & np.isfinite(casts["axis"]).all(axis=1)


def limit(casts):
    return np.minimum(casts["t_max"], MAX_FLOAT)


def derived(a, e1, e2, h):
    """[(a_j, e1_j, e2_j) for j = 0 .. 7]: every vertex and every difference one fp32 operation per component"""
    with np.errstate(all="ignore"):
        A, B, C = a, a + e1, a + e2
        A_, B_, C_ = A - h, B - h, C - h
        corners = [(A_, B_, C_), (A, B, A_), (B_, A_, B), (B, C, B_), (C_, B_, C), (C, A, C_), (A_, C_, A)]
        return [(a, e1, e2)] + [(p, q - p, r - p) for p, q, r in corners]


def capsule_time(o, d, r, h, a, e1, e2):
    """rows of pairs: o, d, h, a, e1, e2 (n, 3), r (n,) float32"""
    t = np.full(len(o), np.inf, dtype=F)
    which = np.zeros(len(o), dtype=np.int64)
    for j, (pj, e1j, e2j) in enumerate(derived(a, e1, e2, h)):
        tj = S.contact_time(o, d, r, pj, e1j, e2j)
        better = tj < t                                      # strictly less, as fp32 values: False for NaN and for -0 against +0
        t = np.where(better, tj, t)
        which = np.where(better, j, which)
    through = TQ.pierce(o, h, a, e1, e2) & ~(t == F(0))
    t_p = RR.ray_triangle(o, h, a, e1, e2)[0]
    t = np.where(through, F(0), t)
    which = np.where(through, PIERCE, which)
    assert t.dtype == F
    return t, which, np.where(through, t_p, F(0)).astype(F)


def contact(o, d, t, h, a, e1, e2, which, t_p):
    """(s, u, v): s from the barycentrics of c(t) on the winning derived triangle, (u, v) of c(t) + h*s on the scene triangle"""
    with np.errstate(all="ignore"):
        c = o + d * t[:, None]
        s = np.where(which == PIERCE, t_p, np.where(which == 1, F(1), F(0))).astype(F)
        for j, (pj, e1j, e2j) in enumerate(derived(a, e1, e2, h)):
            if j < 2:
                continue
            _, _, v1 = P.point_triangle(c, pj, e1j, e2j)
            s = np.where(which == j, F(1) - v1 if j & 1 else v1, s)
        x = c + h * s[:, None]
    _, u, v = P.point_triangle(x, a, e1, e2)
    return s, u, v


def grown_entry(casts, lo, hi):
    """(passes, entry), each (casts, triangles): the walkers' slab test against (lo - max(h, 0)) - r, (hi - min(h, 0)) + r"""
    with np.errstate(all="ignore"):
        inv = F(1) / casts["dir"].astype(F)
        r = casts["radius"][:, None, None]
        h = casts["axis"][:, None, :]
        glo = (lo[None] - np.maximum(h, F(0))) - r
        ghi = (hi[None] - np.minimum(h, F(0))) + r
        return RR.box_entry(casts["origin"][:, None, :], inv[:, None, :], glo, ghi)


def reference(casts, a, b, c, box_lo, box_hi, casts_per_chunk=256, count_rule=False):
    """Brute force in float32.  casts: CAPSULE_RAY array; a, b, c: (T, 3) positions; box_lo, box_hi: (T, 3) the triangles' own boxes.
    records: the candidate with the least t, ties to the lower index, or the miss record; flags: 1 where a candidate exists; ties:
    how many candidates share the least t; which / s: the winning derived triangle and the axis parameter of each record.
    count_rule: also evaluate the pairs that fail the grown-box test; valid = the (active cast, triangle) pairs with a time in
    [0, T), rejected = those of them that miss the grown box or have t < entry."""
    assert casts.dtype == CAPSULE_RAY
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    lo, hi = np.ascontiguousarray(box_lo, dtype=F), np.ascontiguousarray(box_hi, dtype=F)
    e1, e2 = b - a, c - a
    n = len(casts)
    records = np.empty(n, dtype=HIT)
    records[:] = MISS
    flags = np.zeros(n, dtype=np.uint32)
    ties = np.zeros(n, dtype=np.uint32)
    which_out = np.zeros(n, dtype=np.int64)
    s_out = np.zeros(n, dtype=F)
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
        t, which, t_p = capsule_time(sub["origin"][qi], sub["dir"][qi], sub["radius"][qi], sub["axis"][qi], a[ti], e1[ti], e2[ti])
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
        m = pair[rows, k][has]
        s, u, v = contact(casts["origin"][hit], casts["dir"][hit], th, casts["axis"][hit], a[kh], e1[kh], e2[kh], which[m], t_p[m])
        records["t"][hit], records["tri"][hit], records["u"][hit], records["v"][hit] = th, kh, u, v
        flags[hit] = 1
        ties[hit] = (key[has] == th[:, None]).sum(axis=1)
        which_out[hit], s_out[hit] = which[m], s
    return Result(records, flags, ties, valid, rejected, which_out, s_out)


def nearest(casts, a, b, c, casts_per_chunk=32):
    """(t, tri, which, s): the least time below T over all triangles in float32 with no box rule, the lowest index on a tie; t =
    +inf where there is none"""
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    e1, e2 = b - a, c - a
    n, nt = len(casts), len(a)
    out = np.full(n, np.inf, dtype=F)
    tri = np.zeros(n, dtype=np.int64)
    which_out = np.zeros(n, dtype=np.int64)
    s_out = np.zeros(n, dtype=F)
    act = active(casts)
    big = limit(casts)
    for first in range(0, n, casts_per_chunk):
        sel = np.nonzero(act[first:first + casts_per_chunk])[0] + first
        if len(sel) == 0:
            continue
        qi, ti = np.repeat(np.arange(len(sel)), nt), np.tile(np.arange(nt), len(sel))
        sub = casts[sel]
        t, which, t_p = capsule_time(sub["origin"][qi], sub["dir"][qi], sub["radius"][qi], sub["axis"][qi], a[ti], e1[ti], e2[ti])
        t = np.where(t < big[sel][qi], t, F(np.inf)).reshape(len(sel), nt)
        k = t.argmin(axis=1)
        m = np.arange(len(sel)) * nt + k
        tk = t[np.arange(len(sel)), k]
        with np.errstate(all="ignore"):
            s, _, _ = contact(sub["origin"], sub["dir"], np.where(np.isfinite(tk), tk, F(0)), sub["axis"], a[k], e1[k], e2[k], which[m], t_p[m])
        out[sel], tri[sel], which_out[sel], s_out[sel] = tk, k, which[m], s
    return out, tri, which_out, s_out


# ---- the casts of `lbvh_driver capsule <n> [seed] [radius] [height]`: SplitMix64, every draw a scalar fp32 operation in the C++ order

def driver_casts(lo, hi, count, seed=3, radius=1.5, height=4.0):
    """per cast and axis: the origin around the mesh's box and the target inside it (as query_support.driver_rays), then the axis
    component uniform in [-height, height]; t_max 2"""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    casts = np.zeros(count, dtype=CAPSULE_RAY)
    for i in range(count):
        for k in range(3):
            grow = F(0.25) * F(hi[k] - lo[k])
            casts["origin"][i, k] = uni(F(lo[k] - grow), F(hi[k] + grow))
            casts["dir"][i, k] = F(uni(lo[k], hi[k]) - casts["origin"][i, k])
            casts["axis"][i, k] = uni(-F(height), F(height))
    casts["radius"], casts["t_max"] = F(radius), F(2.0)
    return casts
