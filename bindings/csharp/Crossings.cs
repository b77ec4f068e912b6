// Crossings.cs — how many triangles rays of the application's own cross (lbvh_count_hits), and crossing parities of points along
// fixed directions (lbvh_point_crossings), include/lbvh.h.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.count_hits /
// point_crossings / CountHits / PointCrossings.  No reference counterpart: the reference asks its tree about camera rays only.  The
// scene is the container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// Inside / outside of a closed mesh: Inside(parity, nDirs), the majority of the directions; with PointQueries.ClosestPoints on the
// same buffer (maxDist2 is not read here) it gives a signed distance (INTEGRATION §7).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class Crossings
{
    // (1,1,1)/sqrt 3, (-1,2,3)/sqrt 14, (4,-1,2)/sqrt 21, each rounded to float once (host.py DEFAULT_DIRS)
    public static readonly float[] DefaultDirs =
    {
        (float)(1.0 / Math.Sqrt(3.0)), (float)(1.0 / Math.Sqrt(3.0)), (float)(1.0 / Math.Sqrt(3.0)),
        (float)(-1.0 / Math.Sqrt(14.0)), (float)(2.0 / Math.Sqrt(14.0)), (float)(3.0 / Math.Sqrt(14.0)),
        (float)(4.0 / Math.Sqrt(21.0)), (float)(-1.0 / Math.Sqrt(21.0)), (float)(2.0 / Math.Sqrt(21.0)),
    };

    readonly MeshBufferContainer _container;

    public Crossings(MeshBufferContainer container) { _container = container; }

    /// The first `count` rays of `rays` (LbvhNative.Ray, stride 32) -> one uint per ray in `counts` (stride 4): the number of
    /// triangles the ray crosses in (tMin, tMax); two at the same t count 2, 0 for an inactive ray.  Asynchronous.
    public void CountHits(NativeBuffer rays, NativeBuffer counts, int count)
    {
        Check(rays, 32, counts, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(rays.Context, LbvhNative.lbvh_count_hits(rays.Context, rays.Pointer, (UIntPtr)(ulong)count, ref scene, counts.Pointer));
    }

    /// The first `count` points of `points` (LbvhNative.PointQuery, stride 16) -> one uint per point in `parity`: bit j is the
    /// parity of the number of triangles the ray from the point along direction j crosses.  `dirs`: x, y, z per direction, 1 .. 32
    /// of them (default DefaultDirs).  Asynchronous.
    public void PointCrossings(NativeBuffer points, NativeBuffer parity, int count, float[] dirs = null)
    {
        dirs = dirs ?? DefaultDirs;
        if (dirs.Length == 0 || dirs.Length % 3 != 0)
            throw new ArgumentException("Crossings: dirs holds x, y, z per direction");
        Check(points, 16, parity, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(points.Context, LbvhNative.lbvh_point_crossings(points.Context, points.Pointer, (UIntPtr)(ulong)count, dirs,
            (uint)(dirs.Length / 3), ref scene, parity.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void PointCrossings(LbvhNative.PointQuery[] points, uint[] parity, NativeBuffer devicePoints, NativeBuffer deviceParity, float[] dirs = null)
    {
        devicePoints.SetData(points);
        PointCrossings(devicePoints, deviceParity, points.Length, dirs);
        deviceParity.GetData(parity);
    }

    /// Inside when more than half of the nDirs directions saw an odd number of crossings.
    public static bool Inside(uint parity, int nDirs)
    {
        int ones = 0;
        for (int j = 0; j < nDirs; j++) ones += (int)((parity >> j) & 1u);
        return 2 * ones > nDirs;
    }

    static void Check(NativeBuffer input, int inStride, NativeBuffer output, int count)
    {
        if (input.stride != inStride || output.stride != 4)
            throw new ArgumentException("Crossings: rays are LbvhNative.Ray (stride 32), points LbvhNative.PointQuery (16), results uint (4)");
        if (count < 0 || count > input.count || count > output.count)
            throw new ArgumentException("Crossings: count exceeds a buffer");
        if (output.Context != input.Context)
            throw new ArgumentException("Crossings: input and results live on different contexts");
    }
}
