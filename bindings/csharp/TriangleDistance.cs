// TriangleDistance.cs — HOW FAR a triangle is from the mesh, WHERE and IN WHICH DIRECTION (lbvh_triangle_closest_point,
// lbvh_triangle_within_distance, include/lbvh.h): the distance between two meshes, proximity pairs of a mesh against itself (skip),
// speculative contacts of a mesh collider inside a margin.  A query is LbvhNative.TriDistanceQuery, 48 bytes: the vertices a, b, c,
// the ORIGINAL index never reported (0xFFFFFFFF: none) and the squared search radius (+infinity: unbounded); an answer is
// LbvhNative.TriClosest, 32 bytes: dist2, the ORIGINAL triangle index, the edge test that gave the record (0 .. 2: the query's edges
// from a, b, c; 3 .. 5: the scene triangle's edges v0-v1, v0-v2, v1-v2; | 8: that edge pierces the other triangle), s on that edge and
// delta from the scene triangle's nearest point to the query's.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.triangle_closest_points / TriangleClosestPoints and triangle_within_distance / TriangleWithinDistance.  No
// reference counterpart.  The scene is the container's; it must have been built with the derived traversal scene (the drawer's Awake
// does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class TriangleDistance
{
    public const int QueryStride = 48;
    public const int RecordStride = 32;
    public const float NoDistance = 2139095040.0f;
    public const uint NoSkip = 0xFFFFFFFFu;

    readonly MeshBufferContainer _container;

    public TriangleDistance(MeshBufferContainer container) { _container = container; }

    /// The first `count` queries of `queries` (stride 48) -> one LbvhNative.TriClosest per query in `output` (stride 32): the nearest
    /// triangle with dist2 < maxDist2, or the none-record {dist2 = NoDistance, zeros}.  Asynchronous on the buffers' context.
    public void TriangleClosestPoints(NativeBuffer queries, NativeBuffer output, int count)
    {
        Check(queries, output, count, RecordStride);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_closest_point(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, output.Pointer));
    }

    /// 1 per query in `flags` (uint, stride 4) if any triangle lies nearer to the query than sqrt(maxDist2), else 0.  Asynchronous.
    public void TriangleWithinDistance(NativeBuffer queries, NativeBuffer flags, int count)
    {
        Check(queries, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(queries.Context, LbvhNative.lbvh_triangle_within_distance(queries.Context, queries.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void TriangleClosestPoints(LbvhNative.TriDistanceQuery[] queries, LbvhNative.TriClosest[] output, NativeBuffer deviceQueries, NativeBuffer deviceOutput)
    {
        deviceQueries.SetData(queries);
        TriangleClosestPoints(deviceQueries, deviceOutput, queries.Length);
        deviceOutput.GetData(output);
    }

    /// The distance of one record: sqrt(dist2), +infinity for the none-record.
    public static float Distance(LbvhNative.TriClosest record)
    {
        return record.dist2 == NoDistance ? float.PositiveInfinity : (float)Math.Sqrt(record.dist2);
    }

    /// Whether the record's edge belongs to the query (tests 0 .. 2) or to scene triangle `tri` (3 .. 5), and whether it pierces.
    public static bool OnQueryEdge(LbvhNative.TriClosest record) { return (record.edge & 7u) < 3u; }
    public static bool Pierced(LbvhNative.TriClosest record) { return (record.edge & 8u) != 0u; }

    static void Check(NativeBuffer queries, NativeBuffer output, int count, int outStride)
    {
        if (queries.stride != QueryStride || output.stride != outStride)
            throw new ArgumentException("TriangleDistance: queries are LbvhNative.TriDistanceQuery (stride 48), results TriClosest (32) or uint (4)");
        if (count < 0 || count > queries.count || count > output.count)
            throw new ArgumentException("TriangleDistance: count exceeds a buffer");
        if (output.Context != queries.Context)
            throw new ArgumentException("TriangleDistance: queries and results live on different contexts");
    }
}
