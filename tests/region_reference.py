"""CPU restatement of the region queries of include/lbvh.h (lbvh_region_overlaps, lbvh_region_overlaps_any): numpy float32, every
operation rounded on its own, brute force over every (region, triangle) pair, chunked — no tree.  A helper module, not a test file.
Written from the header's text; nothing of the library is imported but the record layout.

    corner_values(planes, lo, hi)                       -> (P, N): the header's two sums for broadcastable fp32 arrays
    reference(regions, box_lo, box_hi)                  -> {TOUCHING: (offsets, tris), CONTAINED: (offsets, tris)}: offsets
                                                           uint64[count + 1], tris uint32 ascending inside every segment
    make_regions(planes)                                layouts.REGION records from an array [count, 6, 4]
    driver_regions(lo, hi, count, seed)                 the regions `lbvh_driver regions` generates (SplitMix64, scalar fp32)

box_lo / box_hi are the triangles' OWN boxes (the library's scene.triangle_aabb: query_support.library_boxes on the GPU,
query_support.padded_boxes on the CPU)."""
import numpy as np

from unitysimpleraytracing_amd.layouts import REGION

F = np.float32
TOUCHING, CONTAINED = 0, 1
PAD = (0.0, 0.0, 0.0, 1.0)                  # a plane that keeps everything: a region with fewer than six faces pads with it


def make_regions(planes):
    planes = np.asarray(planes, dtype=F)
    r = np.zeros(len(planes), dtype=REGION)
    r["plane"] = planes
    return r


def corner_values(planes, lo, hi):
    """planes [..., 4], lo / hi [..., 3], broadcastable, fp32 -> (P, N) in the header's order of operations; n >= 0 is true for -0 and
    false for NaN, as numpy's comparison is"""
    planes, lo, hi = (np.asarray(x, dtype=F) for x in (planes, lo, hi))
    n, d = planes[..., :3], planes[..., 3]
    with np.errstate(all="ignore"):
        pos = n >= F(0.0)
        far, near = np.where(pos, hi, lo), np.where(pos, lo, hi)
        P = ((n[..., 0] * far[..., 0] + n[..., 1] * far[..., 1]) + n[..., 2] * far[..., 2]) + d
        N = ((n[..., 0] * near[..., 0] + n[..., 1] * near[..., 1]) + n[..., 2] * near[..., 2]) + d
    assert P.dtype == F and N.dtype == F
    return P, N


def masks(regions, box_lo, box_hi, pairs_per_chunk=1 << 19):
    """yields (first region, touching bool[rows, triangles], contained bool[rows, triangles])"""
    box_lo, box_hi = np.ascontiguousarray(box_lo, dtype=F)[:, :3], np.ascontiguousarray(box_hi, dtype=F)[:, :3]
    planes = np.ascontiguousarray(regions["plane"], dtype=F)
    step = max(1, pairs_per_chunk // max(len(box_lo), 1))
    for s in range(0, len(planes), step):
        P, N = corner_values(planes[s:s + step, :, None, :], box_lo[None, None], box_hi[None, None])      # [rows, 6, triangles]
        with np.errstate(invalid="ignore"):
            yield s, (P >= F(0.0)).all(axis=1), (N >= F(0.0)).all(axis=1)


def _csr(count, parts):
    counts = np.zeros(count, dtype=np.uint64)
    lists = []
    for first, m in parts:
        counts[first:first + len(m)] = m.sum(axis=1)
        lists.append(np.nonzero(m)[1].astype(np.uint32))           # row-major: ascending triangle index inside each row
    offsets = np.zeros(count + 1, dtype=np.uint64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.uint32))


def reference(regions, box_lo, box_hi):
    touching, contained = [], []
    for first, t, c in masks(regions, box_lo, box_hi):
        touching.append((first, t))
        contained.append((first, c))
    return {TOUCHING: _csr(len(regions), touching), CONTAINED: _csr(len(regions), contained)}


def segments(offsets, tris):
    """the per-region index lists of a CSR pair"""
    return [tris[int(offsets[k]):int(offsets[k + 1])] for k in range(len(offsets) - 1)]


# ---- the regions of `lbvh_driver regions <n> [seed]`: SplitMix64, every draw and every operation a scalar fp32 one in the C++ order --

def driver_regions(lo, hi, count, seed=6):
    """regions_in: per region three pairs of opposed planes.  Pair k: the normal is the unit vector of axis k with its two other
    components drawn uniform in [-0.5, 0.5] (ascending axis order), the centre's coordinate c_k uniform in the mesh box on that axis and the
    half width h uniform in [1, 12]; with s = (n0 * c0 + n1 * c1) + n2 * c2 the planes are {n, h - s} and {-n, h + s}.  All three
    centre coordinates are drawn first, then per pair the two components and h.  A sheared box: no trigonometry, so the mirror is exact."""
    from query_support import splitmix
    set_seed, uni = splitmix()
    set_seed(seed)
    out = np.zeros((count, 6, 4), dtype=F)
    for i in range(count):
        c = [uni(lo[k], hi[k]) for k in range(3)]
        for k in range(3):
            n = [F(0.0)] * 3
            n[k] = F(1.0)
            for j in range(3):
                if j != k:
                    n[j] = uni(-0.5, 0.5)
            h = uni(1.0, 12.0)
            s = F(F(F(n[0] * c[0]) + F(n[1] * c[1])) + F(n[2] * c[2]))
            out[i, 2 * k] = (n[0], n[1], n[2], F(h - s))
            out[i, 2 * k + 1] = (-n[0], -n[1], -n[2], F(h + s))
    return make_regions(out)
