"""CPU restatement of lbvh_sort_record_segments (include/lbvh.h): plain numpy, no tree, no fixtures.  A helper module, not a test
file.  K and the fitting-segment logic are segsort_reference's.

    D(x)                                   the key word of the descending order: 0xFFFFFFFF for a NaN, ~K(x) otherwise
    key_words(words, order)             -> (more significant, less significant) uint32 key words of (n, 8) record words
    reference_records(offsets, records_as_words, capacity, order)
                                        -> a copy of the (n, 8) uint32 array with every fitting segment ordered by its key with
                                           np.lexsort; everything else — segments that do not fit, records no segment owns, records
                                           at or beyond the capacity — unchanged
    as_words(records)                   -> the (n, 8) uint32 view of an array of 32-byte records

The library's sort is not stable: the expectation is unique only where the keys inside a segment are distinct."""
import numpy as np

from segsort_reference import _segments, fitting, K  # noqa: F401  (fitting: for the tests)

ASCENDING, DESCENDING, BY_TRI = 0, 1, 2             # LBVH_SORT_RECORDS_*


def D(x):
    k = K(x)
    return np.where(k == np.uint32(0xFFFFFFFF), k, ~k).astype(np.uint32)


def as_words(records):
    r = np.ascontiguousarray(records)
    assert r.dtype.itemsize == 32 or (r.dtype == np.uint32 and r.ndim == 2 and r.shape[1] == 8)
    return r.view(np.uint32).reshape(-1, 8)


def key_words(w, order):
    if order == BY_TRI:
        return w[:, 3], np.zeros(len(w), dtype=np.uint32)
    t = np.ascontiguousarray(w[:, 0]).view(np.float32)
    return (K(t) if order == ASCENDING else D(t)), w[:, 1]


def reference_records(offsets, records_as_words, capacity, order):
    assert order in (ASCENDING, DESCENDING, BY_TRI)
    w = as_words(records_as_words)
    out = w.copy()
    index, segment = _segments(offsets, capacity)
    part = w[index]
    high, low = key_words(part, order)
    out[index] = part[np.lexsort((low, high, segment))]
    return out
