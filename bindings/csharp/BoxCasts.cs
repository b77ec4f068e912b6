// BoxCasts.cs — moving boxes of the application's own against a scene the re-hosted classes built: the first contact of each
// (lbvh_box_cast) or whether it touches anything on its way (lbvh_box_cast_any), include/lbvh.h.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.box_cast / BoxCast; what Unity code calls Physics.BoxCast (centre, halfExtents and orientation folded into the
// three half-axis vectors ax, ay, az = rotation * (hx, 0, 0), (0, hy, 0), (0, 0, hz)) and, with a short cast, Physics.CheckBox.  No
// reference counterpart: the reference asks its tree about camera rays only.  The scene is the container's; it must have been built
// with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class BoxCasts
{
    readonly MeshBufferContainer _container;

    public BoxCasts(MeshBufferContainer container) { _container = container; }

    /// The first `count` casts of `casts` (LbvhNative.BoxRay, stride 80) -> one LbvhNative.BoxHit per cast in `hits` (stride 16): the
    /// box's centre is at centre + dir * t when it first touches triangle `tri`, `axis` is the separating axis that gave the time
    /// (13: overlapping at the start; the contact normal is -sign(dot(dir, L)) * L / |L| for the header's L of that axis), or the
    /// miss record {t = 2139095040, 0, 0, 0} if it touches nothing for 0 <= t < tMax.  Asynchronous on the buffers' context.
    public void Cast(NativeBuffer casts, NativeBuffer hits, int count)
    {
        Check(casts, hits, count, 16);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_box_cast(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, hits.Pointer));
    }

    /// 1 per cast in `flags` (uint, stride 4) if the box touches anything on its way, else 0.  Asynchronous.
    public void CastAny(NativeBuffer casts, NativeBuffer flags, int count)
    {
        Check(casts, flags, count, 4);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_box_cast_any(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, flags.Pointer));
    }

    /// Host arrays in and out through the caller's device buffers (blocking: GetData waits for the walk).
    public void Cast(LbvhNative.BoxRay[] casts, LbvhNative.BoxHit[] hits, NativeBuffer deviceCasts, NativeBuffer deviceHits)
    {
        deviceCasts.SetData(casts);
        Cast(deviceCasts, deviceHits, casts.Length);
        deviceHits.GetData(hits);
    }

    public void CastAny(LbvhNative.BoxRay[] casts, uint[] flags, NativeBuffer deviceCasts, NativeBuffer deviceFlags)
    {
        deviceCasts.SetData(casts);
        CastAny(deviceCasts, deviceFlags, casts.Length);
        deviceFlags.GetData(flags);
    }

    static void Check(NativeBuffer casts, NativeBuffer output, int count, int outStride)
    {
        if (casts.stride != 80 || output.stride != outStride)
            throw new ArgumentException("BoxCasts: casts are LbvhNative.BoxRay (stride 80), results BoxHit (16) or uint (4)");
        if (count < 0 || count > casts.count || count > output.count)
            throw new ArgumentException("BoxCasts: count exceeds a buffer");
        if (output.Context != casts.Context)
            throw new ArgumentException("BoxCasts: casts and results live on different contexts");
    }
}
