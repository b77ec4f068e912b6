// TriangleQueries.cs — WHICH triangles of a scene the re-hosted classes built a triangle intersects (lbvh_triangle_intersections,
// lbvh_triangle_intersects_any, include/lbvh.h): the narrow phase behind OverlapQueries.BoxOverlaps.  A query is 48 bytes: a and
// skip, b and a pad word, c and a pad word; skip is the ORIGINAL index of a scene triangle that is never reported (a mesh against
// itself), 0xFFFFFFFF for none.  The list form is the CSR list of OverlapQueries: offsets (ulong, count + 1 of them) and the ORIGINAL
// triangle indices (uint), in no particular order inside a query's segment; SegmentSort orders them on the device.  Twin of host.py /
// lbvh_host.hpp RaytracingMeshDrawer.triangle_intersections / TriangleIntersections.  No reference counterpart.  The scene is the
// container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// Coplanar overlapping triangles are not reported and touching ones are reported when the fp32 arithmetic says so: see the header.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class TriangleQueries
{
    public const int QueryStride = 48;
    public const uint NoSkip = 0xFFFFFFFFu;

    readonly MeshBufferContainer _container;

    public TriangleQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` triangles of `queries` (stride 48) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `tris` is
    /// null, `tris` (uint, stride 4; its whole length is the capacity).  tris = null counts only; offsets[count] says what is needed.
    /// Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void TriangleIntersections(NativeBuffer queries, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(queries, count);
        if (offsets.stride != 8 || count + 1 > offsets.count || (tris != null && tris.stride != 4))
            throw new ArgumentException("TriangleQueries: offsets are ulong with count + 1 entries, tris are uint");
        if (offsets.Context != queries.Context || (tris != null && tris.Context != queries.Context))
            throw new ArgumentException("TriangleQueries: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_intersections(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// 1 into `flags` (uint, stride 4) for each of the first `count` triangles of `queries` that intersects any scene triangle, else 0.
    public void TriangleIntersectsAny(NativeBuffer queries, NativeBuffer flags, int count)
    {
        Check(queries, count);
        if (flags.stride != 4 || count > flags.count || flags.Context != queries.Context)
            throw new ArgumentException("TriangleQueries: flags are uint, at least count of them, on the queries' context");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_intersects_any(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene,
            flags.Pointer));
    }

    static void Check(NativeBuffer queries, int count)
    {
        if (queries.stride != QueryStride || count < 0 || count > queries.count)
            throw new ArgumentException("TriangleQueries: queries have stride 48 and at least count entries");
    }
}
