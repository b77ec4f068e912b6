// SegmentQueries.cs — HOW FAR a segment is from the mesh, WHERE and IN WHICH DIRECTION (lbvh_segment_closest_point,
// lbvh_segment_within_distance, include/lbvh.h): a capsule's clearance when it touches nothing — what Unity code calls
// Physics.ClosestPoint, and the separated case of Physics.ComputePenetration.  A query is LbvhNative.SegmentQuery, 32 bytes: the
// segment origin .. origin + axis and the squared search radius (+infinity: unbounded); an answer is LbvhNative.SegmentClosest, 32
// bytes: dist2, the ORIGINAL triangle index, the nearest point's u, v on the triangle, delta from that point to the nearest point
// of the segment, and that point's parameter s.  A capsule of radius r has the clearance sqrt(dist2) - r and, where dist2 > 0, the
// separating direction delta / sqrt(dist2).  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.segment_closest_points /
// SegmentClosestPoints and segment_within_distance / SegmentWithinDistance.  No reference counterpart.  The scene is the
// container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class SegmentQueries
{
    public const int QueryStride = 32;
    public const int RecordStride = 32;
    public const float NoDistance = 2139095040.0f;

    readonly MeshBufferContainer _container;

    public SegmentQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` queries of `queries` (stride 32) -> one LbvhNative.SegmentClosest per query in `output` (stride 32): the
    /// nearest triangle with dist2 < maxDist2, or the none-record {dist2 = NoDistance, zeros}.  Asynchronous on the buffers' context.
    public void SegmentClosestPoints(NativeBuffer queries, NativeBuffer output, int count)
    {
        Check(queries, output, count, RecordStride);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_segment_closest_point(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, output.Pointer));
    }

    /// 1 per query in `flags` (uint, stride 4) if any triangle lies nearer to the segment than sqrt(maxDist2), else 0.  Asynchronous.
    public void SegmentWithinDistance(NativeBuffer queries, NativeBuffer flags, int count)
    {
        Check(queries, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_segment_within_distance(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void SegmentClosestPoints(LbvhNative.SegmentQuery[] queries, LbvhNative.SegmentClosest[] output, NativeBuffer deviceQueries, NativeBuffer deviceOutput)
    {
        deviceQueries.SetData(queries);
        SegmentClosestPoints(deviceQueries, deviceOutput, queries.Length);
        deviceOutput.GetData(output);
    }

    /// The clearance of a capsule of radius `radius` from one record: sqrt(dist2) - radius, +infinity for the none-record.
    public static float Clearance(LbvhNative.SegmentClosest record, float radius)
    {
        return record.dist2 == NoDistance ? float.PositiveInfinity : (float)Math.Sqrt(record.dist2) - radius;
    }

    static void Check(NativeBuffer queries, NativeBuffer output, int count, int outStride)
    {
        if (queries.stride != QueryStride || output.stride != outStride)
            throw new ArgumentException("SegmentQueries: queries are LbvhNative.SegmentQuery (stride 32), results SegmentClosest (32) or uint (4)");
        if (count < 0 || count > queries.count || count > output.count)
            throw new ArgumentException("SegmentQueries: count exceeds a buffer");
        if (output.Context != queries.Context)
            throw new ArgumentException("SegmentQueries: queries and results live on different contexts");
    }
}
