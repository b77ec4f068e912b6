// TriangleSegments.cs — WHERE a triangle cuts each triangle of the scene it intersects (lbvh_triangle_intersection_segments,
// include/lbvh.h): the contact polyline between two meshes, a cut curve, a cross-section.  A query is TriangleQueries' (48 bytes: a
// and skip, b and a pad word, c and a pad word); a record is LbvhNative.TriSegment, 32 bytes: the two ends p0 and p1 of the segment
// the two triangles share, the ORIGINAL index of the scene triangle, and edges — bits 0 .. 5: which of the six edge tests passed
// (0, 1, 2 the query's edges from a, b, c; 3, 4, 5 the scene triangle's edges v0-v1, v0-v2, v1-v2), bits 8 .. 10 the test that gave
// p0, bits 12 .. 14 the one that gave p1, so that a polyline is stitched by (triangle, edge) and no floats are compared.  The list
// form is TriangleQueries.TriangleIntersections with a record in place of an index: the same offsets, the records in no particular
// order inside a query's segment.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.triangle_intersection_segments /
// TriangleIntersectionSegments.  No reference counterpart.  The scene is the container's; it must have been built with the derived
// traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class TriangleSegments
{
    public const int QueryStride = 48;
    public const int SegmentStride = 32;

    readonly MeshBufferContainer _container;

    public TriangleSegments(MeshBufferContainer container) { _container = container; }

    /// The first `count` triangles of `queries` (stride 48) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `segments`
    /// is null, `segments` (LbvhNative.TriSegment, stride 32; its whole length is the capacity).  segments = null counts only;
    /// offsets[count] says what is needed.  Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void TriangleIntersectionSegments(NativeBuffer queries, NativeBuffer offsets, NativeBuffer segments, int count)
    {
        if (queries.stride != QueryStride || count < 0 || count > queries.count)
            throw new ArgumentException("TriangleSegments: queries have stride 48 and at least count entries");
        if (offsets.stride != 8 || count + 1 > offsets.count || (segments != null && segments.stride != SegmentStride))
            throw new ArgumentException("TriangleSegments: offsets are ulong with count + 1 entries, segments have stride 32");
        if (offsets.Context != queries.Context || (segments != null && segments.Context != queries.Context))
            throw new ArgumentException("TriangleSegments: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_intersection_segments(queries.Context, queries.Pointer, (UIntPtr)(ulong)count,
            ref scene, offsets.Pointer, segments == null ? IntPtr.Zero : segments.Pointer, segments == null ? 0UL : (ulong)segments.count));
    }

    /// Whether edge test j (0 .. 5) of a record passed, and the tests that gave its two ends.
    public static bool Passed(uint edges, int j) { return ((edges >> j) & 1u) != 0u; }
    public static int EdgeOfP0(uint edges) { return (int)((edges >> 8) & 7u); }
    public static int EdgeOfP1(uint edges) { return (int)((edges >> 12) & 7u); }
}
