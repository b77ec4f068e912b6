// OverlapQueries.cs — WHICH triangles of a scene the re-hosted classes built touch a box (lbvh_box_overlaps) or lie within a
// distance of a point (lbvh_gather_within_distance), include/lbvh.h, as a CSR list: offsets (ulong, count + 1 of them) and the
// ORIGINAL triangle indices (uint) of every query's candidates, in no particular order inside a query's segment.  Twin of
// host.py / lbvh_host.hpp RaytracingMeshDrawer.box_overlaps / BoxOverlaps.  No reference counterpart.  The scene is the
// container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// The length of the list is not known before the call.  Either size `tris` generously and check offsets[count] afterwards, or call
// twice: once with tris = null (count only), read offsets[count] (Total), allocate, call again.  Nothing is ever written at or
// beyond the capacity of `tris`; a segment that ends at or below it is complete.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class OverlapQueries
{
    readonly MeshBufferContainer _container;

    public OverlapQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` boxes of `boxes` (AABB records, stride 32 — a container's triangle boxes can be passed as they are) ->
    /// `offsets` (ulong, stride 8, count + 1 entries) and, unless `tris` is null, `tris` (uint, stride 4; its whole length is the
    /// capacity).  Asynchronous on the buffers' context.
    public void BoxOverlaps(NativeBuffer boxes, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(boxes, 32, offsets, tris, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(boxes.Context, LbvhNative.lbvh_box_overlaps(boxes.Context, boxes.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// The same for points with radii (LbvhNative.PointQuery, stride 16): every triangle lbvh_within_distance would accept.
    public void GatherWithinDistance(NativeBuffer queries, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(queries, 16, offsets, tris, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_gather_within_distance(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// offsets[count] of the last call: the number of candidates of all queries together (blocking: waits for the call).
    public ulong Total(NativeBuffer offsets, int count)
    {
        ulong[] host = new ulong[offsets.count];
        offsets.GetData(host);
        return host[count];
    }

    static void Check(NativeBuffer queries, int queryStride, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        if (queries.stride != queryStride || offsets.stride != 8 || (tris != null && tris.stride != 4))
            throw new ArgumentException("OverlapQueries: boxes have stride 32, point queries 16, offsets 8 (ulong), tris 4 (uint)");
        if (count < 0 || count > queries.count || count + 1 > offsets.count)
            throw new ArgumentException("OverlapQueries: count exceeds a buffer (offsets needs count + 1 entries)");
        if (offsets.Context != queries.Context || (tris != null && tris.Context != queries.Context))
            throw new ArgumentException("OverlapQueries: the buffers live on different contexts");
    }
}
