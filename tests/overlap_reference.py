"""CPU restatement of the overlap queries of include/lbvh.h (lbvh_box_overlaps, lbvh_gather_within_distance): numpy float32, brute
force over every (query, triangle) pair, chunked — no tree.  A helper module, not a test file.

    box_active(boxes)                                   min <= max on all three axes (False when a bound is NaN)
    box_overlaps(boxes, box_lo, box_hi)                 -> (offsets uint64[count + 1], tris uint32, ascending inside every segment)
    gather_within_distance(queries, a, b, c, box_lo, box_hi)   -> the same for point queries

The box form is six comparisons.  The distance form takes its arithmetic, its active rule and R from tests/point_reference.py and
returns the candidate mask where `reference` there returns its arg-min.  box_lo / box_hi are the triangles' OWN boxes (the library's
scene.triangle_aabb)."""
import numpy as np

from point_reference import active, box_dist2, point_triangle, radius2
from unitysimpleraytracing_amd.layouts import AABB


def box_active(boxes):
    with np.errstate(invalid="ignore"):
        return (boxes["min"][:, :3] <= boxes["max"][:, :3]).all(axis=1)


def _csr(count, masks):
    """masks: iterable of (first query, bool[rows, triangles]) covering every query once, in order"""
    counts = np.zeros(count, dtype=np.uint64)
    parts = []
    for first, m in masks:
        counts[first:first + len(m)] = m.sum(axis=1)
        parts.append(np.nonzero(m)[1].astype(np.uint32))           # row-major: ascending triangle index inside each row
    offsets = np.zeros(count + 1, dtype=np.uint64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32))


def make_boxes(lo, hi):
    b = np.zeros(len(lo), dtype=AABB)
    b["min"][:, :3], b["max"][:, :3] = lo, hi
    return b


def box_overlaps(boxes, box_lo, box_hi, pairs_per_chunk=1 << 22):
    f = np.float32
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=f), np.ascontiguousarray(box_hi, dtype=f)
    qlo, qhi = np.ascontiguousarray(boxes["min"][:, :3], dtype=f), np.ascontiguousarray(boxes["max"][:, :3], dtype=f)
    act = box_active(boxes)
    step = max(1, pairs_per_chunk // max(len(box_lo), 1))

    def masks():
        for s in range(0, len(boxes), step):
            with np.errstate(invalid="ignore"):
                m = ((qlo[s:s + step, None, :] <= box_hi[None]) & (box_lo[None] <= qhi[s:s + step, None, :])).all(axis=2)
            yield s, m & act[s:s + step, None]
    return _csr(len(boxes), masks())


def gather_within_distance(queries, a, b, c, box_lo, box_hi, pairs_per_chunk=1 << 22):
    f = np.float32
    a, b, c = (np.ascontiguousarray(x, dtype=f) for x in (a, b, c))
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=f), np.ascontiguousarray(box_hi, dtype=f)
    e1, e2 = b - a, c - a
    act = active(queries)
    with np.errstate(invalid="ignore"):
        act = act & ~np.isnan(queries["p"]).any(axis=1)             # a NaN coordinate: every dist2 is NaN, no candidate
    big = radius2(queries)
    step = max(1, pairs_per_chunk // max(len(a), 1))

    def masks():
        for s in range(0, len(queries), step):
            p = queries["p"][s:s + step][:, None, :]
            d, _, _ = point_triangle(p, a[None], e1[None], e2[None])
            own = box_dist2(p, box_lo[None], box_hi[None])
            with np.errstate(invalid="ignore"):
                m = (d < big[s:s + step, None]) & ~(d < own)         # False for a NaN dist2
            yield s, m & act[s:s + step, None]
    return _csr(len(queries), masks())


def sort_segments(offsets, tris):
    """every segment of a CSR list in ascending order (the order inside a segment is not part of the library's contract)"""
    offsets = np.asarray(offsets, dtype=np.uint64)
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets).astype(np.int64))
    assert len(seg) == len(tris)
    return np.asarray(tris)[np.lexsort((tris, seg))]
