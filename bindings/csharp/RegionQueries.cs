// RegionQueries.cs — WHICH triangles of a scene the re-hosted classes built lie in a convex region bounded by six planes
// (lbvh_region_overlaps, lbvh_region_overlaps_any, include/lbvh.h): a camera or light frustum, an oriented box, an editor's window /
// crossing selection.  A region is 96 bytes: six planes {nx, ny, nz, d}, each keeping the half space n . x + d >= 0; a region with
// fewer faces repeats a plane or pads with {0, 0, 0, 1}.  Touching: the triangles whose own box is not wholly outside any plane (the
// conservative frustum test); Contained: those whose own box is wholly inside every plane, hence wholly inside the region.  The list
// form is the CSR list of OverlapQueries: offsets (ulong, count + 1 of them) and the ORIGINAL triangle indices (uint), in no particular
// order inside a region's segment; SegmentSort orders them on the device.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.region_overlaps / RegionOverlaps.  No reference counterpart.  The scene is the container's; it must have been
// built with the derived traversal scene (the drawer's Awake does that).  One region per lane: RegionOverlaps is for many regions;
// RegionOverlapsLarge (lbvh_region_overlaps_large) spreads each of a few large regions — one camera frustum, a cascade, a marquee
// selection — over the device and gives the same lists.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class RegionQueries
{
    public const int RegionStride = 96;
    public const uint Touching = 0u;
    public const uint Contained = 1u;
    public const int LargeMaxCount = 65536;

    readonly MeshBufferContainer _container;

    public RegionQueries(MeshBufferContainer container) { _container = container; }

    /// The first `count` regions of `regions` (stride 96) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `tris` is
    /// null, `tris` (uint, stride 4; its whole length is the capacity).  tris = null counts only; offsets[count] says what is needed.
    /// Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void RegionOverlaps(NativeBuffer regions, uint mode, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(regions, mode, count);
        if (offsets.stride != 8 || count + 1 > offsets.count || (tris != null && tris.stride != 4))
            throw new ArgumentException("RegionQueries: offsets are ulong with count + 1 entries, tris are uint");
        if (offsets.Context != regions.Context || (tris != null && tris.Context != regions.Context))
            throw new ArgumentException("RegionQueries: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(regions.Context, LbvhNative.lbvh_region_overlaps(regions.Context, regions.Pointer, (UIntPtr)(ulong)count, mode, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// RegionOverlaps for few large regions (count <= LargeMaxCount): the same offsets and, per segment, the same set of indices, in
    /// another order.
    public void RegionOverlapsLarge(NativeBuffer regions, uint mode, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        Check(regions, mode, count);
        if (count > LargeMaxCount) throw new ArgumentException("RegionQueries: RegionOverlapsLarge takes at most 65536 regions");
        if (offsets.stride != 8 || count + 1 > offsets.count || (tris != null && tris.stride != 4))
            throw new ArgumentException("RegionQueries: offsets are ulong with count + 1 entries, tris are uint");
        if (offsets.Context != regions.Context || (tris != null && tris.Context != regions.Context))
            throw new ArgumentException("RegionQueries: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(regions.Context, LbvhNative.lbvh_region_overlaps_large(regions.Context, regions.Pointer, (UIntPtr)(ulong)count, mode, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// 1 into `flags` (uint, stride 4) for each of the first `count` regions of `regions` that has a candidate in `mode`, else 0.
    public void RegionOverlapsAny(NativeBuffer regions, uint mode, NativeBuffer flags, int count)
    {
        Check(regions, mode, count);
        if (flags.stride != 4 || count > flags.count || flags.Context != regions.Context)
            throw new ArgumentException("RegionQueries: flags are uint, at least count of them, on the regions' context");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(regions.Context, LbvhNative.lbvh_region_overlaps_any(regions.Context, regions.Pointer, (UIntPtr)(ulong)count, mode, ref scene,
            flags.Pointer));
    }

    static void Check(NativeBuffer regions, uint mode, int count)
    {
        if (regions.stride != RegionStride || mode > Contained || count < 0 || count > regions.count)
            throw new ArgumentException("RegionQueries: regions have stride 96 and at least count entries, mode is Touching or Contained");
    }
}
