// TriangleCasts.cs — moving triangles of the application's own against a scene the re-hosted classes built: the first contact of each
// (lbvh_triangle_cast) or whether it touches anything on its way (lbvh_triangle_cast_any), include/lbvh.h.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.triangle_cast / TriangleCast; what Unity code calls Rigidbody.SweepTest for a mesh collider, one cast per triangle
// of the moving mesh with the same dir, the least record taken by the caller.  No reference counterpart: the reference asks its tree
// about camera rays only.  The scene is the container's; it must have been built with the derived traversal scene (the drawer's Awake
// does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class TriangleCasts
{
    readonly MeshBufferContainer _container;

    public TriangleCasts(MeshBufferContainer container) { _container = container; }

    /// The first `count` casts of `casts` (LbvhNative.TriRay, stride 64) -> one LbvhNative.TriCastHit per cast in `hits` (stride 16): the
    /// triangle is at a + dir * t, b + dir * t, c + dir * t when it first touches triangle `tri`; `feature` is the pair that gave the
    /// time (0 - 2: moving vertex on the scene face; 3 - 5: scene vertex on the moving face; 6 + 3m + n: moving edge m on scene edge n
    /// at position w of it; 16 | j: intersecting at the start, t = 0), or the miss record {t = 2139095040, 0, 0, 0} if it touches
    /// nothing for 0 <= t < tMax.  Asynchronous on the buffers' context.
    public void Cast(NativeBuffer casts, NativeBuffer hits, int count)
    {
        Check(casts, hits, count, 16);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_triangle_cast(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, hits.Pointer));
    }

    /// 1 per cast in `flags` (uint, stride 4) if the triangle touches anything on its way, else 0.  Asynchronous.
    public void CastAny(NativeBuffer casts, NativeBuffer flags, int count)
    {
        Check(casts, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_triangle_cast_any(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void Cast(LbvhNative.TriRay[] casts, LbvhNative.TriCastHit[] hits, NativeBuffer deviceCasts, NativeBuffer deviceHits)
    {
        deviceCasts.SetData(casts);
        Cast(deviceCasts, deviceHits, casts.Length);
        deviceHits.GetData(hits);
    }

    public void CastAny(LbvhNative.TriRay[] casts, uint[] flags, NativeBuffer deviceCasts, NativeBuffer deviceFlags)
    {
        deviceCasts.SetData(casts);
        CastAny(deviceCasts, deviceFlags, casts.Length);
        deviceFlags.GetData(flags);
    }

    static void Check(NativeBuffer casts, NativeBuffer output, int count, int outStride)
    {
        if (casts.stride != 64 || output.stride != outStride)
            throw new ArgumentException("TriangleCasts: casts are LbvhNative.TriRay (stride 64), results TriCastHit (16) or uint (4)");
        if (count < 0 || count > casts.count || count > output.count)
            throw new ArgumentException("TriangleCasts: count exceeds a buffer");
        if (output.Context != casts.Context)
            throw new ArgumentException("TriangleCasts: casts and results live on different contexts");
    }
}
