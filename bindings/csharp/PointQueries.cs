// PointQueries.cs — points of the application's own against a scene the re-hosted classes built: the nearest triangle of each
// point (lbvh_closest_point_query) or whether any triangle lies within its radius (lbvh_within_distance), include/lbvh.h.  Twin of
// host.py / lbvh_host.hpp RaytracingMeshDrawer.closest_points / ClosestPoints.  No reference counterpart: the reference asks its
// tree about camera rays only.  The scene is the container's; it must have been built with the derived traversal scene (the
// drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class PointQueries
{
    readonly MeshBufferContainer _container;

    public PointQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` queries of `queries` (LbvhNative.PointQuery, stride 16) -> one LbvhNative.ClosestPoint per query in `output`
    /// (stride 16): the nearest triangle with dist2 < maxDist2, or the none-record {dist2 = 2139095040, 0, 0, 0}.  Asynchronous on
    /// the buffers' context.
    public void ClosestPoints(NativeBuffer queries, NativeBuffer output, int count)
    {
        Check(queries, output, count, 16);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_closest_point_query(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, output.Pointer));
    }

    /// 1 per query in `flags` (uint, stride 4) if any triangle lies nearer than sqrt(maxDist2), else 0.  Asynchronous.
    public void WithinDistance(NativeBuffer queries, NativeBuffer flags, int count)
    {
        Check(queries, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_within_distance(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void ClosestPoints(LbvhNative.PointQuery[] queries, LbvhNative.ClosestPoint[] output, NativeBuffer deviceQueries, NativeBuffer deviceOutput)
    {
        deviceQueries.SetData(queries);
        ClosestPoints(deviceQueries, deviceOutput, queries.Length);
        deviceOutput.GetData(output);
    }

    public void WithinDistance(LbvhNative.PointQuery[] queries, uint[] flags, NativeBuffer deviceQueries, NativeBuffer deviceFlags)
    {
        deviceQueries.SetData(queries);
        WithinDistance(deviceQueries, deviceFlags, queries.Length);
        deviceFlags.GetData(flags);
    }

    static void Check(NativeBuffer queries, NativeBuffer output, int count, int outStride)
    {
        if (queries.stride != 16 || output.stride != outStride)
            throw new ArgumentException("PointQueries: queries are LbvhNative.PointQuery (stride 16), results ClosestPoint (16) or uint (4)");
        if (count < 0 || count > queries.count || count > output.count)
            throw new ArgumentException("PointQueries: count exceeds a buffer");
        if (output.Context != queries.Context)
            throw new ArgumentException("PointQueries: queries and results live on different contexts");
    }
}
