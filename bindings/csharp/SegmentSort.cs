// SegmentSort.cs — every segment of a CSR list put into order on the device, in place (lbvh_sort_hit_segments and
// lbvh_sort_index_segments, include/lbvh.h): the pass after RayGather.Gather when the hits of a ray are needed front to back
// (thickness, entry / exit pairing, CSG along a ray — what one sorts Physics.RaycastAll's array for), and after OverlapQueries when
// candidate lists are to be de-duplicated or intersected.  Twin of host.py sort_hit_segments / sort_index_segments and of
// lbvh_host.hpp SortHitSegments / SortIndexSegments.  Hit records are ordered by (t, tri), indices ascending; a segment that did not
// fit the capacity of the data buffer is left as it is.  The call needs no scene and keeps the path tracer's live-path list.
// SortRecords is the same pass for the lists of 32-byte records (lbvh_sort_record_segments; host.py sort_record_segments,
// lbvh_host.hpp SortRecordSegments): contacts deepest first, proximity records nearest first, segment and section records by triangle.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public static class SegmentSort
{
    /// `offsets` (ulong, stride 8, count + 1 entries) as a gather wrote them; `hits` (LbvhNative.Hit, stride 16) the buffer that was
    /// given to that gather: its whole length is the capacity.  Asynchronous on the buffers' context.
    public static void SortHits(NativeBuffer offsets, NativeBuffer hits, int count)
    {
        Check(offsets, hits, 16, count);
        LbvhNative.Check(offsets.Context, LbvhNative.lbvh_sort_hit_segments(offsets.Context, offsets.Pointer, (UIntPtr)(ulong)count, hits.Pointer,
            (ulong)hits.count));
    }

    /// The same for the uint indices (stride 4) of an overlap query.
    public static void SortIndices(NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(offsets, tris, 4, count);
        LbvhNative.Check(offsets.Context, LbvhNative.lbvh_sort_index_segments(offsets.Context, offsets.Pointer, (UIntPtr)(ulong)count, tris.Pointer,
            (ulong)tris.count));
    }

    /// The same for the 32-byte records (stride 32) of ShapeContacts, TriangleProximity, TriangleSegments and PlaneSections
    /// (lbvh_sort_record_segments).  `order`: LbvhNative.SortRecordsAscending — (word 0 as a float, word 1): nearest first for
    /// proximity records —, SortRecordsDescending — deepest first for contacts, the first record of a segment is the Deepest
    /// call's —, SortRecordsByTri — word 3, the triangle of a segment or section record.
    public static void SortRecords(NativeBuffer offsets, NativeBuffer records, int count, uint order)
    {
        Check(offsets, records, 32, count);
        if (order > LbvhNative.SortRecordsByTri)
            throw new ArgumentException("SegmentSort: order is one of LbvhNative.SortRecords*");
        LbvhNative.Check(offsets.Context, LbvhNative.lbvh_sort_record_segments(offsets.Context, offsets.Pointer, (UIntPtr)(ulong)count,
            records.Pointer, (ulong)records.count, order));
    }

    static void Check(NativeBuffer offsets, NativeBuffer data, int stride, int count)
    {
        if (offsets == null || data == null || offsets.stride != 8 || data.stride != stride)
            throw new ArgumentException("SegmentSort: offsets are ulong (stride 8), the data LbvhNative.Hit (16), uint (4) or a 32-byte record");
        if (count < 0 || count + 1 > offsets.count)
            throw new ArgumentException("SegmentSort: offsets needs count + 1 entries");
        if (offsets.Context != data.Context)
            throw new ArgumentException("SegmentSort: the buffers live on different contexts");
    }
}
