// RayQueries.cs — rays of the application's own over a scene the re-hosted classes built: the closest hit of each ray
// (lbvh_trace_closest) or whether anything lies between its tMin and tMax (lbvh_trace_occluded), include/lbvh.h.  Twin of
// host.py / lbvh_host.hpp RaytracingMeshDrawer.trace_closest / TraceClosest.  No reference counterpart: the reference traces
// its camera's primary rays only.  The scene is the container's; it must have been built with the derived traversal scene
// (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class RayQueries
{
    readonly MeshBufferContainer _container;

    public RayQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` rays of `rays` (LbvhNative.Ray, stride 32) -> one LbvhNative.Hit per ray in `hits` (stride 16): the nearest
    /// hit with tMin < t < tMax, or the miss record {t = 2139095040, 0, 0, 0}.  Asynchronous on the buffers' context.
    public void TraceClosest(NativeBuffer rays, NativeBuffer hits, int count)
    {
        Check(rays, hits, count, 16);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(rays.Context, LbvhNative.lbvh_trace_closest(rays.Context, rays.Pointer, (UIntPtr)(ulong)count, ref scene, hits.Pointer));
    }

    /// 1 per ray in `flags` (uint, stride 4) if anything lies between its tMin and tMax, else 0.  Asynchronous.
    public void TraceOccluded(NativeBuffer rays, NativeBuffer flags, int count)
    {
        Check(rays, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(rays.Context, LbvhNative.lbvh_trace_occluded(rays.Context, rays.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the trace).
    public void TraceClosest(LbvhNative.Ray[] rays, LbvhNative.Hit[] hits, NativeBuffer deviceRays, NativeBuffer deviceHits)
    {
        deviceRays.SetData(rays);
        TraceClosest(deviceRays, deviceHits, rays.Length);
        deviceHits.GetData(hits);
    }

    public void TraceOccluded(LbvhNative.Ray[] rays, uint[] flags, NativeBuffer deviceRays, NativeBuffer deviceFlags)
    {
        deviceRays.SetData(rays);
        TraceOccluded(deviceRays, deviceFlags, rays.Length);
        deviceFlags.GetData(flags);
    }

    static void Check(NativeBuffer rays, NativeBuffer output, int count, int outStride)
    {
        if (rays.stride != 32 || output.stride != outStride)
            throw new ArgumentException("RayQueries: rays are LbvhNative.Ray (stride 32), results Hit (16) or uint (4)");
        if (count < 0 || count > rays.count || count > output.count)
            throw new ArgumentException("RayQueries: count exceeds a buffer");
        if (output.Context != rays.Context)
            throw new ArgumentException("RayQueries: rays and results live on different contexts");
    }
}
