// CastGather.cs — EVERY triangle each moving sphere, capsule or box of the application's own touches before its t_max
// (lbvh_sphere_cast_all, lbvh_capsule_cast_all, lbvh_box_cast_all, include/lbvh.h), against a scene the re-hosted classes built, as a
// CSR list: offsets (ulong, count + 1 of them) and 16-byte records, segment q = hits[offsets[q] .. offsets[q + 1]) — LbvhNative.Hit
// {t, tri, u, v} for spheres and capsules, LbvhNative.BoxHit {t, tri, axis, 0} for boxes: what SphereCasts / CapsuleCasts / BoxCasts
// would write were that triangle the first.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.sphere_cast_all / SphereCastAll
// and their capsule and box forms.  TriangleCastAll is the same for moving triangles (lbvh_triangle_cast_all; LbvhNative.TriCastHit
// {t, tri, feature, w}, what TriangleCasts would write), twin of triangle_cast_all / TriangleCastAll.  The counterparts of Unity's Physics.SphereCastAll, CapsuleCastAll and BoxCastAll, with the
// same promise about order: NONE.  Each record carries its t: SegmentSort.SortHits orders every segment by (t, tri) on the device
// (box records included: t and tri are the same two words).  The scene is the container's; it must have been built with the derived
// traversal scene (the drawer's Awake does that).
// The length of the list is not known before the call.  Either size `hits` generously and check offsets[count] afterwards, or call
// twice: once with hits = null (count only), read offsets[count] (Total), allocate, call again.  Nothing is ever written at or
// beyond the capacity of `hits`; a segment that ends at or below it is complete.  Give a move its real length as t_max: the cost
// grows with the swept volume.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class CastGather
{
    readonly MeshBufferContainer _container;

    public CastGather(MeshBufferContainer container) { _container = container; }

    /// The first `count` casts of `casts` (LbvhNative.SphereRay, stride 32) -> `offsets` (ulong, stride 8, count + 1 entries) and,
    /// unless `hits` is null, `hits` (LbvhNative.Hit, stride 16; its whole length is the capacity).  Asynchronous.
    public void SphereCastAll(NativeBuffer casts, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        Check(casts, 32, offsets, hits, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_sphere_cast_all(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            hits == null ? IntPtr.Zero : hits.Pointer, hits == null ? 0UL : (ulong)hits.count));
    }

    /// The same for capsules (LbvhNative.CapsuleRay, stride 48).
    public void CapsuleCastAll(NativeBuffer casts, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        Check(casts, 48, offsets, hits, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_capsule_cast_all(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            hits == null ? IntPtr.Zero : hits.Pointer, hits == null ? 0UL : (ulong)hits.count));
    }

    /// The same for boxes (LbvhNative.BoxRay, stride 80); `hits` holds LbvhNative.BoxHit records (stride 16).
    public void BoxCastAll(NativeBuffer casts, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        Check(casts, 80, offsets, hits, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_box_cast_all(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            hits == null ? IntPtr.Zero : hits.Pointer, hits == null ? 0UL : (ulong)hits.count));
    }

    /// The same for moving triangles (LbvhNative.TriRay, stride 64, as TriangleCasts takes them; lbvh_triangle_cast_all); `hits`
    /// holds LbvhNative.TriCastHit records (stride 16): {t, tri, feature, w} of every triangle touched, `skip` never among them.
    /// SegmentSort.SortHits takes these records too: feature and w travel with their record.
    public void TriangleCastAll(NativeBuffer casts, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        Check(casts, 64, offsets, hits, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(casts.Context, LbvhNative.lbvh_triangle_cast_all(casts.Context, casts.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            hits == null ? IntPtr.Zero : hits.Pointer, hits == null ? 0UL : (ulong)hits.count));
    }

    /// offsets[count] of the last call: the number of records of all casts together (blocking: waits for the call).
    public ulong Total(NativeBuffer offsets, int count)
    {
        ulong[] host = new ulong[offsets.count];
        offsets.GetData(host);
        return host[count];
    }

    static void Check(NativeBuffer casts, int stride, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        if (casts.stride != stride || offsets.stride != 8 || (hits != null && hits.stride != 16))
            throw new ArgumentException("CastGather: casts have stride " + stride + ", offsets are ulong (8), hits 16-byte records");
        if (count < 0 || count > casts.count || count + 1 > offsets.count)
            throw new ArgumentException("CastGather: count exceeds a buffer (offsets needs count + 1 entries)");
        if (offsets.Context != casts.Context || (hits != null && hits.Context != casts.Context))
            throw new ArgumentException("CastGather: the buffers live on different contexts");
    }
}
