// CapsuleCasts.cs — moving capsules of the application's own against a scene the re-hosted classes built: the first contact of each
// (lbvh_capsule_cast) or whether it touches anything on its way (lbvh_capsule_cast_any), include/lbvh.h.  Twin of host.py /
// lbvh_host.hpp RaytracingMeshDrawer.capsule_cast / CapsuleCast; what Unity code calls Physics.CapsuleCast (point1 = origin,
// point2 = origin + axis) and, with a short cast, Physics.CheckCapsule.  No reference counterpart:
// the reference asks its tree about camera rays only.  The scene is the container's; it must have been built with the derived
// traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class CapsuleCasts
{
    readonly MeshBufferContainer _container;

    public CapsuleCasts(MeshBufferContainer container) { _container = container; }

    /// The first `count` casts of `casts` (LbvhNative.CapsuleRay, stride 48) -> one LbvhNative.Hit per cast in `hits` (stride 16): the
    /// capsule's axis starts at origin + dir * t when it first touches triangle `tri` at a + e1 * u + e2 * v, or the miss record
    /// {t = 2139095040, 0, 0, 0} if it touches nothing for 0 <= t < tMax.  Asynchronous on the buffers' context.
    public void Cast(NativeBuffer casts, NativeBuffer hits, int count)
    {
        Check(casts, hits, count, 16);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_capsule_cast(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, hits.Pointer));
    }

    /// 1 per cast in `flags` (uint, stride 4) if the capsule touches anything on its way, else 0.  Asynchronous.
    public void CastAny(NativeBuffer casts, NativeBuffer flags, int count)
    {
        Check(casts, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_capsule_cast_any(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void Cast(LbvhNative.CapsuleRay[] casts, LbvhNative.Hit[] hits, NativeBuffer deviceCasts, NativeBuffer deviceHits)
    {
        deviceCasts.SetData(casts);
        Cast(deviceCasts, deviceHits, casts.Length);
        deviceHits.GetData(hits);
    }

    public void CastAny(LbvhNative.CapsuleRay[] casts, uint[] flags, NativeBuffer deviceCasts, NativeBuffer deviceFlags)
    {
        deviceCasts.SetData(casts);
        CastAny(deviceCasts, deviceFlags, casts.Length);
        deviceFlags.GetData(flags);
    }

    static void Check(NativeBuffer casts, NativeBuffer output, int count, int outStride)
    {
        if (casts.stride != 48 || output.stride != outStride)
            throw new ArgumentException("CapsuleCasts: casts are LbvhNative.CapsuleRay (stride 48), results Hit (16) or uint (4)");
        if (count < 0 || count > casts.count || count > output.count)
            throw new ArgumentException("CapsuleCasts: count exceeds a buffer");
        if (output.Context != casts.Context)
            throw new ArgumentException("CapsuleCasts: casts and results live on different contexts");
    }
}
