// PlaneSections.cs — WHERE a plane cuts the mesh (lbvh_plane_sections, include/lbvh.h): a cross-section or contour line, a slice
// for 3D printing, a water line, the outline of a clipping cap.  A plane is LbvhNative.Plane (16 bytes: n and d with n . x + d = 0);
// a record is LbvhNative.PlaneSegment, 32 bytes: p0, the crossing on the triangle's edge that leaves the positive side (n . x + d >=
// 0), the ORIGINAL index of the scene triangle, p1, the crossing on the edge that returns to it, and edges — bits 0 .. 2: the two
// crossing edges (0, 1, 2: v0-v1, v1-v2, v2-v0), bits 8 .. 9 the edge that gave p0, bits 12 .. 13 the edge that gave p1, bits 16 ..
// 18 the sides of v0, v1, v2.  On a consistently wound mesh the p1-edge of a record is the p0-edge of the neighbour across it, so a
// closed, oriented contour is stitched by (triangle, edge) through the mesh's adjacency and no floats are compared.  Every plane is
// spread over the device (the frame of RegionQueries.RegionOverlapsLarge); at most MaxCount planes per call.  The records of a
// plane's segment come in no particular order.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.plane_sections / PlaneSections.
// No reference counterpart.  The scene is the container's; it must have been built with the derived traversal scene (the drawer's
// Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class PlaneSections
{
    public const int PlaneStride = 16;
    public const int SegmentStride = 32;
    public const int MaxCount = 65536;                      // LBVH_PLANE_SECTIONS_MAX_COUNT

    readonly MeshBufferContainer _container;

    public PlaneSections(MeshBufferContainer container) { _container = container; }

    /// The first `count` planes of `planes` (stride 16) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `segments` is
    /// null, `segments` (LbvhNative.PlaneSegment, stride 32; its whole length is the capacity).  segments = null counts only;
    /// offsets[count] says what is needed.  Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void Sections(NativeBuffer planes, NativeBuffer offsets, NativeBuffer segments, int count)
    {
        if (planes.stride != PlaneStride || count < 0 || count > planes.count || count > MaxCount)
            throw new ArgumentException("PlaneSections: planes have stride 16 and at least count entries, count is at most 65536");
        if (offsets.stride != 8 || count + 1 > offsets.count || (segments != null && segments.stride != SegmentStride))
            throw new ArgumentException("PlaneSections: offsets are ulong with count + 1 entries, segments have stride 32");
        if (offsets.Context != planes.Context || (segments != null && segments.Context != planes.Context))
            throw new ArgumentException("PlaneSections: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(planes.Context, LbvhNative.lbvh_plane_sections(planes.Context, planes.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, segments == null ? IntPtr.Zero : segments.Pointer, segments == null ? 0UL : (ulong)segments.count));
    }

    /// Whether edge k (0 .. 2) of a record's triangle crosses the plane, the edges that gave its two ends, and the side of vertex k.
    public static bool Crosses(uint edges, int k) { return ((edges >> k) & 1u) != 0u; }
    public static int EdgeOfP0(uint edges) { return (int)((edges >> 8) & 3u); }
    public static int EdgeOfP1(uint edges) { return (int)((edges >> 12) & 3u); }
    public static bool Positive(uint edges, int k) { return ((edges >> (16 + k)) & 1u) != 0u; }
}
