// KClosestPoints.cs — the k nearest triangles of each point of the application's own (lbvh_k_closest_points, include/lbvh.h), against
// a scene the re-hosted classes built.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.k_closest_points / KClosestPoints.  No
// reference counterpart: the reference asks its tree about camera rays only.  The scene is the container's; it must have been
// built with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class KClosestPoints
{
    readonly MeshBufferContainer _container;

    public KClosestPoints(MeshBufferContainer container) { _container = container; }

    /// The first `count` queries of `queries` (LbvhNative.PointQuery, stride 16) -> k LbvhNative.ClosestPoint per query in `output`
    /// (stride 16, at least count * k entries): output[q * k + j] is the j-th nearest triangle of query q with dist2 < maxDist2, ties
    /// by the lower triangle index; rows are padded with the none-record {dist2 = 2139095040, 0, 0, 0}.  `found` (uint, stride 4, may
    /// be null) receives the number of real records of each row.  Asynchronous on the buffers' context.
    public void Query(NativeBuffer queries, int k, NativeBuffer output, NativeBuffer found, int count)
    {
        if (k < 1 || k > LbvhNative.K_CLOSEST_MAX)
            throw new ArgumentException("KClosestPoints: k must be 1 .. " + LbvhNative.K_CLOSEST_MAX);
        if (queries.stride != 16 || output.stride != 16 || (found != null && found.stride != 4))
            throw new ArgumentException("KClosestPoints: queries are LbvhNative.PointQuery (stride 16), results ClosestPoint (16), counts uint (4)");
        if (count < 0 || count > queries.count || (long)count * k > output.count || (found != null && count > found.count))
            throw new ArgumentException("KClosestPoints: count exceeds a buffer");
        if (output.Context != queries.Context || (found != null && found.Context != queries.Context))
            throw new ArgumentException("KClosestPoints: queries and results live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_k_closest_points(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, (uint)k, ref scene,
                                                                          output.Pointer, found != null ? found.Pointer : IntPtr.Zero));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).  output.Length >=
    /// queries.Length * k; found may be null together with deviceFound.
    public void Query(LbvhNative.PointQuery[] queries, int k, LbvhNative.ClosestPoint[] output, uint[] found, NativeBuffer deviceQueries,
                      NativeBuffer deviceOutput, NativeBuffer deviceFound)
    {
        deviceQueries.SetData(queries);
        Query(deviceQueries, k, deviceOutput, deviceFound, queries.Length);
        deviceOutput.GetData(output);
        if (found != null && deviceFound != null) deviceFound.GetData(found);
    }
}
