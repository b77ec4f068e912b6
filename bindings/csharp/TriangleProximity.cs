// TriangleProximity.cs — EVERY scene triangle within a distance of a triangle (lbvh_triangle_gather_within_distance,
// include/lbvh.h): the proximity pairs of cloth and self-collision (a mesh against itself with skip), speculative contacts of a mesh
// collider inside a margin.  A query is LbvhNative.TriDistanceQuery (TriangleDistance.cs), 48 bytes; a record is LbvhNative.TriClosest,
// 32 bytes, exactly what TriangleDistance.TriangleClosestPoints would write were that triangle the only one: dist2, the ORIGINAL
// triangle index, the edge test that gave the record (| 8: pierced), s on that edge and delta from the scene triangle's nearest point
// to the query's.  The list is ShapeContacts.CapsuleContacts' CSR form: offsets always complete, the records in no particular order
// inside a query's segment, nothing ever written at or beyond the capacity.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.triangle_gather_within_distance / TriangleGatherWithinDistance.  No reference counterpart.  The scene is the
// container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class TriangleProximity
{
    public const int QueryStride = 48;
    public const int RecordStride = 32;
    public const uint NoSkip = 0xFFFFFFFFu;

    readonly MeshBufferContainer _container;

    public TriangleProximity(MeshBufferContainer container) { _container = container; }

    /// The first `count` queries of `queries` (stride 48) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `records` is
    /// null, `records` (LbvhNative.TriClosest, stride 32; its whole length is the capacity).  records = null counts only;
    /// offsets[count] says what is needed.  Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void TriangleGatherWithinDistance(NativeBuffer queries, NativeBuffer offsets, NativeBuffer records, int count)
    {
        if (queries.stride != QueryStride || count < 0 || count > queries.count)
            throw new ArgumentException("TriangleProximity: queries are LbvhNative.TriDistanceQuery (stride 48) and at least count entries");
        if (offsets.stride != 8 || count + 1 > offsets.count || (records != null && records.stride != RecordStride))
            throw new ArgumentException("TriangleProximity: offsets are ulong with count + 1 entries, records have stride 32");
        if (offsets.Context != queries.Context || (records != null && records.Context != queries.Context))
            throw new ArgumentException("TriangleProximity: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_gather_within_distance(queries.Context, queries.Pointer, (UIntPtr)(ulong)count,
            ref scene, offsets.Pointer, records == null ? IntPtr.Zero : records.Pointer, records == null ? 0UL : (ulong)records.count));
    }

    /// Count, read the total (blocking: one 8-byte-per-offset download), and say how many records the fill needs.
    public ulong Count(NativeBuffer queries, NativeBuffer offsets, int count)
    {
        TriangleGatherWithinDistance(queries, offsets, null, count);
        ulong[] host = new ulong[offsets.count];
        offsets.GetData(host);
        return host[count];
    }

    /// A self-proximity pass lists every pair twice, (i, j) and (j, i): keep the one with query < tri.
    public static bool FirstOfPair(int query, LbvhNative.TriClosest record) { return (uint)query < record.tri; }
    public static bool Pierced(LbvhNative.TriClosest record) { return (record.edge & 8u) != 0u; }
}
