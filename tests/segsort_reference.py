"""CPU restatement of lbvh_sort_hit_segments / lbvh_sort_index_segments (include/lbvh.h): plain numpy, no tree, no fixtures.
A helper module, not a test file.

    K(t)                                   the header's key word of an fp32 value, operation by operation, on uint32 arrays
    fitting(offsets, capacity)          -> bool per segment: offsets[q] <= offsets[q + 1] <= capacity
    reference_hits(offsets, records, capacity)  -> a copy of `records` (layouts.HIT, any length) with every fitting segment ordered
                                           by (K(t), tri) with np.lexsort; everything else — segments that do not fit, records
                                           no segment owns, records at or beyond the capacity — unchanged
    reference_index(offsets, tris, capacity)    -> the same for uint32 words, ascending

The library's sort is not stable: the expectation is unique only where the keys inside a segment are distinct (or the records of
equal key are identical in every word)."""
import numpy as np

HIT = np.dtype([("t", np.float32), ("tri", np.uint32), ("u", np.float32), ("v", np.float32)])


def K(t):
    """w = the bits of t; a NaN (w & 0x7FFFFFFF > 0x7F800000) -> 0xFFFFFFFF; -0 (w == 0x80000000) -> w = 0; then a set sign bit
    -> ~w, a clear one -> w | 0x80000000"""
    w = np.ascontiguousarray(t, dtype=np.float32).view(np.uint32).copy()
    nan = (w & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    w[w == np.uint32(0x80000000)] = 0
    k = np.where((w & np.uint32(0x80000000)) != 0, ~w, w | np.uint32(0x80000000))
    return np.where(nan, np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def fitting(offsets, capacity):
    off = np.asarray(offsets, dtype=np.uint64)
    return (off[:-1] <= off[1:]) & (off[1:] <= np.uint64(capacity))


def _segments(offsets, capacity):
    """(the record indices of all fitting segments, the segment of each)"""
    off = np.asarray(offsets, dtype=np.uint64)
    fit = np.nonzero(fitting(off, capacity))[0]
    lo = off[fit].astype(np.int64)
    length = off[fit + 1].astype(np.int64) - lo
    segment = np.repeat(fit, length)
    first = np.repeat(lo - (np.cumsum(length) - length), length)
    return first + np.arange(len(segment)), segment


def reference_hits(offsets, records, capacity):
    assert records.dtype == HIT
    out = records.copy()
    index, segment = _segments(offsets, capacity)
    part = records[index]
    out[index] = part[np.lexsort((part["tri"], K(part["t"]), segment))]
    return out


def reference_index(offsets, tris, capacity):
    assert tris.dtype == np.uint32
    out = tris.copy()
    index, segment = _segments(offsets, capacity)
    part = tris[index]
    out[index] = part[np.lexsort((part, segment))]
    return out
