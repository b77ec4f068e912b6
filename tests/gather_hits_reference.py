"""CPU restatement of lbvh_gather_hits (include/lbvh.h): numpy float32, brute force over every (ray, triangle) pair — no tree.
A helper module, not a test file.  The slab test, Moeller-Trumbore, activity, T and the candidate mask are ray_reference's, unchanged.

    reference(rays, a, b, c, box_lo, box_hi) -> Result(offsets, records)
        offsets     uint64, len(rays) + 1: the cumulative sum of the rays' candidate counts, offsets[0] = 0
        records     HIT, offsets[-1] of them: segment q = records[offsets[q] : offsets[q + 1]] = every candidate of ray q in
                    (t, tri) order — a STABLE sort on t over the triangles in index order, so equal t (-0 and +0 included, they
                    compare equal) fall to the lower index.  The library promises no order inside a segment: compare after
                    canonical(offsets, records) on both sides.
    canonical(offsets, records) -> the records with every segment ordered by (t as an fp32 value, tri).  Two candidates of a ray
                    never share a triangle index, so the result does not depend on the order it is given."""
from collections import namedtuple

import numpy as np

import ray_reference as R

Result = namedtuple("Result", "offsets records")


def reference(rays, a, b, c, box_lo, box_hi, pairs_per_chunk=1 << 22):
    f = np.float32
    assert rays.dtype == R.RAY
    a, b, c = (np.ascontiguousarray(x, dtype=f) for x in (a, b, c))
    lo, hi = np.ascontiguousarray(box_lo, dtype=f), np.ascontiguousarray(box_hi, dtype=f)
    e1, e2 = b - a, c - a
    n, t_count = len(rays), len(a)
    counts = np.zeros(n, dtype=np.uint64)
    blocks = []
    act = R.active(rays)
    with np.errstate(all="ignore"):
        inv_all = f(1) / rays["dir"].astype(f)
        big = np.minimum(rays["t_max"], R.MAX_FLOAT)
    step = max(1, pairs_per_chunk // max(t_count, 1))
    for s in range(0, n, step):
        sel = np.nonzero(act[s:s + step])[0] + s
        if len(sel) == 0:
            continue
        o = rays["origin"][sel][:, None, :]
        d = rays["dir"][sel][:, None, :]
        passes, entry = R.box_entry(o, inv_all[sel][:, None, :], lo[None], hi[None])
        t, u, v = R.ray_triangle(o, d, a[None], e1[None], e2[None])
        with np.errstate(invalid="ignore"):
            cand = passes & ~(t < entry) & (t > rays["t_min"][sel][:, None]) & (t < big[sel][:, None])
        counts[sel] = cand.sum(axis=1)
        row, tri = np.nonzero(cand)                            # row-major: ray by ray, the triangles in index order
        block = np.empty(len(row), dtype=R.HIT)
        block["t"], block["tri"], block["u"], block["v"] = t[row, tri], tri, u[row, tri], v[row, tri]
        blocks.append(block[np.lexsort((tri, block["t"], row))])   # lexsort is stable: equal t keep the index order
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    records = np.concatenate(blocks) if blocks else np.empty(0, dtype=R.HIT)
    assert len(records) == int(offsets[-1])
    return Result(offsets, records)


def canonical(offsets, records):
    offsets = np.asarray(offsets).astype(np.int64)
    records = np.ascontiguousarray(records[: offsets[-1]])
    segment = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return records[np.lexsort((records["tri"], records["t"], segment))]
