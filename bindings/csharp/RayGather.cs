// RayGather.cs — EVERY hit along each ray of the application's own (lbvh_gather_hits, include/lbvh.h), against a scene the
// re-hosted classes built, as a CSR list: offsets (ulong, count + 1 of them) and LbvhNative.Hit records {t, tri, u, v}, segment q =
// hits[offsets[q] .. offsets[q + 1]).  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.gather_hits / GatherHits.  The
// counterpart of Unity's Physics.RaycastAll, with the same promise about order: NONE.  The records of a segment come in the order
// of the library's walk; each carries its t, so SortSegments below (a host sort by (t, tri)) gives the canonical order where one
// is needed.  The first 32 in order are KClosestHits.  The scene is the container's; it must have been built with the derived
// traversal scene (the drawer's Awake does that).
// The length of the list is not known before the call.  Either size `hits` generously and check offsets[count] afterwards, or call
// twice: once with hits = null (count only), read offsets[count] (Total), allocate, call again.  Nothing is ever written at or
// beyond the capacity of `hits`; a segment that ends at or below it is complete.
// SOURCE ONLY (no C# toolchain in the build image).
using System;
using System.Collections.Generic;

public sealed class RayGather
{
    readonly MeshBufferContainer _container;

    public RayGather(MeshBufferContainer container) { _container = container; }

    /// The first `count` rays of `rays` (LbvhNative.Ray, stride 32) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless
    /// `hits` is null, `hits` (LbvhNative.Hit, stride 16; its whole length is the capacity).  Asynchronous on the buffers' context.
    public void Gather(NativeBuffer rays, NativeBuffer offsets, NativeBuffer hits, int count)
    {
        if (rays.stride != 32 || offsets.stride != 8 || (hits != null && hits.stride != 16))
            throw new ArgumentException("RayGather: rays are LbvhNative.Ray (stride 32), offsets ulong (8), hits LbvhNative.Hit (16)");
        if (count < 0 || count > rays.count || count + 1 > offsets.count)
            throw new ArgumentException("RayGather: count exceeds a buffer (offsets needs count + 1 entries)");
        if (offsets.Context != rays.Context || (hits != null && hits.Context != rays.Context))
            throw new ArgumentException("RayGather: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(rays.Context, LbvhNative.lbvh_gather_hits(rays.Context, rays.Pointer, (UIntPtr)(ulong)count, ref scene, offsets.Pointer,
            hits == null ? IntPtr.Zero : hits.Pointer, hits == null ? 0UL : (ulong)hits.count));
    }

    /// offsets[count] of the last call: the number of hits of all rays together (blocking: waits for the call).
    public ulong Total(NativeBuffer offsets, int count)
    {
        ulong[] host = new ulong[offsets.count];
        offsets.GetData(host);
        return host[count];
    }

    /// Orders every segment of downloaded records by (t, tri), in place, on the host.
    public static void SortSegments(ulong[] offsets, LbvhNative.Hit[] hits, int count)
    {
        Comparer<LbvhNative.Hit> byTThenTri = Comparer<LbvhNative.Hit>.Create(
            (x, y) => x.t != y.t ? x.t.CompareTo(y.t) : x.tri.CompareTo(y.tri));
        for (int q = 0; q < count; q++)
            Array.Sort(hits, (int)offsets[q], (int)(offsets[q + 1] - offsets[q]), byTThenTri);
    }
}
