// KClosestHits.cs — the first k hits along each ray of the application's own (lbvh_trace_k_closest, include/lbvh.h), against a
// scene the re-hosted classes built.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.trace_k_closest / TraceKClosest.  No
// reference counterpart: the reference traces its camera's primary rays to the first hit only.  The scene is the container's; it
// must have been built with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class KClosestHits
{
    readonly MeshBufferContainer _container;

    public KClosestHits(MeshBufferContainer container) { _container = container; }

    /// The first `count` rays of `rays` (LbvhNative.Ray, stride 32) -> k LbvhNative.Hit per ray in `hits` (stride 16, at least
    /// count * k entries): hits[q * k + j] is the j-th nearest hit of ray q with tMin < t < tMax, ties by the lower triangle index;
    /// rows are padded with the miss record {t = 2139095040, 0, 0, 0}.  `found` (uint, stride 4, may be null) receives the number of
    /// real records of each row.  Asynchronous on the buffers' context.
    public void Trace(NativeBuffer rays, int k, NativeBuffer hits, NativeBuffer found, int count)
    {
        if (k < 1 || k > LbvhNative.K_CLOSEST_MAX)
            throw new ArgumentException("KClosestHits: k must be 1 .. " + LbvhNative.K_CLOSEST_MAX);
        if (rays.stride != 32 || hits.stride != 16 || (found != null && found.stride != 4))
            throw new ArgumentException("KClosestHits: rays are LbvhNative.Ray (stride 32), results Hit (16), counts uint (4)");
        if (count < 0 || count > rays.count || (long)count * k > hits.count || (found != null && count > found.count))
            throw new ArgumentException("KClosestHits: count exceeds a buffer");
        if (hits.Context != rays.Context || (found != null && found.Context != rays.Context))
            throw new ArgumentException("KClosestHits: rays and results live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(rays.Context, LbvhNative.lbvh_trace_k_closest(rays.Context, rays.Pointer, (UIntPtr)(ulong)count, (uint)k, ref scene,
                                                                       hits.Pointer, found != null ? found.Pointer : IntPtr.Zero));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).  hits.Length >=
    /// rays.Length * k; found may be null together with deviceFound.
    public void Trace(LbvhNative.Ray[] rays, int k, LbvhNative.Hit[] hits, uint[] found, NativeBuffer deviceRays, NativeBuffer deviceHits,
                      NativeBuffer deviceFound)
    {
        deviceRays.SetData(rays);
        Trace(deviceRays, k, deviceHits, deviceFound, rays.Length);
        deviceHits.GetData(hits);
        if (found != null && deviceFound != null) deviceFound.GetData(found);
    }
}
