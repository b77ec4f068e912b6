"""CPU restatement of the capsule contacts of include/lbvh.h (lbvh_capsule_contacts, lbvh_capsule_deepest): numpy float32, one
rounded operation per step, brute force over every (shape, triangle) pair — no tree.  A helper module, not a test file.  The
candidate set is shape_overlap_reference's and the arithmetic is imported, not written again: the active rule, rule 1 and rule 2
are shape_overlap_reference.active / rule1 / capsule_touch, the derived triangles are capsule_reference.derived, dist2 with its
barycentrics is point_reference.point_triangle, the pierce and its t are triangle_query_reference.pierce and
ray_reference.ray_triangle.  What is here is the header's own text: the pierce first, the least d_j in the order of j, s from the
winning j, the residual and its length on the scene triangle, the face contact, and the deepest record's order.

    contact(o, r, h, a, e1, e2)                   rows of candidate pairs -> Contact(depth, u, v, normal, s, which, face): which =
                                                  the winning j, PIERCE for the pierce; face = step 4 formed the record
    reference(shapes, a, b, c, box_lo, box_hi)    -> Result: offsets uint64[count + 1], contacts layouts.CONTACT (ascending tri inside
                                                  every segment), deepest layouts.CONTACT[count], pairs = the rule-1 pairs, which and
                                                  face per listed contact
    deepest_of(offsets, contacts)                 the reduction alone: the greatest depth, ties to the lower tri; NONE if empty
    sort_segments(offsets, contacts)              every segment into ascending tri order (a host sort of the device's list)
    driver_capsules(lo, hi, count, seed)          the capsules `lbvh_driver contacts` generates

box_lo / box_hi are the triangles' OWN boxes (the library's scene.triangle_aabb)."""
from collections import namedtuple

import numpy as np

import capsule_reference as CR
import point_reference as P
import ray_reference as RR
import shape_overlap_reference as S
import triangle_query_reference as TQ
from unitysimpleraytracing_amd.layouts import CAPSULE, CONTACT, NULL

F = np.float32
PIERCE = CR.PIERCE
NONE = np.zeros(1, dtype=CONTACT)[0]
NONE["tri"] = NULL

Contact = namedtuple("Contact", "depth u v normal s which face")
Result = namedtuple("Result", "offsets contacts deepest pairs which face")


def _dot(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


def _cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2], x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]], axis=1)


def contact(o, r, h, a, e1, e2):
    """rows of CANDIDATE pairs: o, h, a, e1, e2 (n, 3), r (n,) float32"""
    n = len(o)
    with np.errstate(all="ignore"):
        # 1. the pierce first
        pierced = TQ.pierce(o, h, a, e1, e2)
        t_p = RR.ray_triangle(o, h, a, e1, e2)[0]
        # 2. the least d_j in the order of j, strictly less, and s from the winning j
        least = np.full(n, np.inf, dtype=F)
        which = np.zeros(n, dtype=np.int64)
        s = np.zeros(n, dtype=F)
        for j, (pj, e1j, e2j) in enumerate(CR.derived(a, e1, e2, h)):
            d, _, v1 = P.point_triangle(o, pj, e1j, e2j)
            better = d < least
            least = np.where(better, d, least)
            which = np.where(better, j, which)
            sj = F(0) if j == 0 else F(1) if j == 1 else (F(1) - v1 if j & 1 else v1)
            s = np.where(better, sj, s).astype(F)
        s = np.where(pierced, t_p, s).astype(F)
        which = np.where(pierced, PIERCE, which)
        # 3. on the scene triangle
        x = o + h * s[:, None]
        dist2, u, v = P.point_triangle(x, a, e1, e2)
        ap = x - a
        rv = ap - (e1 * u[:, None] + e2 * v[:, None])
        dist = np.sqrt(dist2)
        normal = rv / dist[:, None]
        depth = r - dist
        face = pierced | (dist2 == F(0)) | np.isnan(dist2)
        # 4. the face contact
        nrm = _cross(e1, e2)
        length = np.sqrt(_dot(nrm, nrm))
        flat = (length == F(0)) | np.isnan(length)
        g0 = _dot(nrm, o - a)
        g1 = _dot(nrm, (o + h) - a)
        sign = np.where(g0 + g1 >= F(0), F(1), F(-1)).astype(F)
        face_normal = np.where(flat[:, None], F(0), (sign[:, None] * nrm) / length[:, None])
        face_depth = np.where(flat, r, r + np.fmax(np.fmax(-sign * g0, -sign * g1), F(0)) / length)
        normal = np.where(face[:, None], face_normal, normal).astype(F)
        depth = np.where(face, face_depth, depth).astype(F)
    assert depth.dtype == F and normal.dtype == F and s.dtype == F and u.dtype == F and dist.dtype == F and length.dtype == F
    return Contact(depth, u, v, normal, s, which, face)


def deepest_of(offsets, contacts):
    count = len(offsets) - 1
    out = np.empty(count, dtype=CONTACT)
    out[:] = NONE
    for k in range(count):
        seg = contacts[int(offsets[k]):int(offsets[k + 1])]
        if len(seg):
            out[k] = seg[np.lexsort((seg["tri"], -seg["depth"]))[0]]       # depth descending, then tri ascending
    return out


def sort_segments(offsets, contacts):
    out = contacts.copy()
    for k in range(len(offsets) - 1):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        out[lo:hi] = out[lo:hi][np.argsort(out["tri"][lo:hi], kind="stable")]
    return out


def reference(shapes, a, b, c, box_lo, box_hi, pairs_per_chunk=1 << 22):
    assert shapes.dtype == CAPSULE
    a, b, c = (np.ascontiguousarray(x, dtype=F) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    e1, e2 = b - a, c - a                                   # what the triangle line of the derived scene holds
    act = S.active(shapes)
    count, n = len(shapes), len(a)
    step = max(1, pairs_per_chunk // max(n, 1))
    counts = np.zeros(count, dtype=np.uint64)
    parts, which_parts, face_parts = [], [], []
    pairs = 0
    for first in range(0, count, step):
        sub = shapes[first:first + step]
        m = S.rule1(sub, box_lo, box_hi) & act[first:first + step, None]
        rows, tri = np.nonzero(m)                           # row-major: ascending triangle index inside each row
        pairs += len(rows)
        within, pierced = S.capsule_touch(sub["origin"][rows], sub["radius"][rows], sub["axis"][rows], a[tri], e1[tri], e2[tri])
        hit = within | pierced
        rows, tri = rows[hit], tri[hit]
        k = contact(sub["origin"][rows], sub["radius"][rows], sub["axis"][rows], a[tri], e1[tri], e2[tri])
        rec = np.zeros(len(rows), dtype=CONTACT)
        rec["depth"], rec["tri"], rec["u"], rec["v"], rec["normal"], rec["s"] = k.depth, tri, k.u, k.v, k.normal, k.s
        counts += np.bincount(rows + first, minlength=count).astype(np.uint64)
        parts.append(rec)
        which_parts.append(k.which)
        face_parts.append(k.face)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    np.cumsum(counts, out=offsets[1:])
    cat = lambda p, dt: np.concatenate(p) if p else np.zeros(0, dtype=dt)
    contacts = cat(parts, CONTACT)
    return Result(offsets, contacts, deepest_of(offsets, contacts), pairs, cat(which_parts, np.int64), cat(face_parts, bool))


# ---- the capsules of `lbvh_driver contacts <n> [seed]`: SplitMix64, every draw a scalar fp32 operation in the C++ order ----------

def driver_capsules(lo, hi, count, seed=11):
    """per capsule and axis k: the origin in the mesh's box, then the axis component in [-6, 6]; radius 3"""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    capsules = np.zeros(count, dtype=CAPSULE)
    for i in range(count):
        for k in range(3):
            capsules["origin"][i, k] = uni(lo[k], hi[k])
            capsules["axis"][i, k] = uni(-6.0, 6.0)
    capsules["radius"] = F(3.0)
    return capsules
