// ShapeOverlaps.cs — WHICH triangles of a scene the re-hosted classes built a capsule or an oriented box touches where it stands
// (lbvh_capsule_overlaps, lbvh_obb_overlaps and their _any forms, include/lbvh.h): the start overlap of CapsuleCasts / BoxCasts
// without a direction.  What Unity code calls Physics.OverlapCapsule / OverlapBox (the lists) and CheckCapsule / CheckBox (the
// flags).  A capsule is LbvhNative.Capsule, 32 bytes: one end of the axis and the radius, then the axis (the other end is origin +
// axis) and a pad word.  A box is LbvhNative.Obb, 64 bytes: the centre and the three half-axis vectors ax, ay, az = rotation *
// (hx, 0, 0), (0, hy, 0), (0, 0, hz), each followed by a pad word; nothing is normalised, a sheared box is taken as it is.  The list
// form is the CSR list of OverlapQueries: offsets (ulong, count + 1 of them) and the ORIGINAL triangle indices (uint), in no
// particular order inside a shape's segment; SegmentSort orders them on the device.  Twin of host.py / lbvh_host.hpp
// RaytracingMeshDrawer.capsule_overlaps / CapsuleOverlaps and obb_overlaps / ObbOverlaps.  No reference counterpart.  The scene is
// the container's; it must have been built with the derived traversal scene (the drawer's Awake does that).
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class ShapeOverlaps
{
    public const int CapsuleStride = 32;
    public const int ObbStride = 64;

    readonly MeshBufferContainer _container;

    public ShapeOverlaps(MeshBufferContainer container) { _container = container; }

    /// The first `count` capsules of `shapes` (stride 32) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `tris` is
    /// null, `tris` (uint, stride 4; its whole length is the capacity).  tris = null counts only; offsets[count] says what is needed.
    /// Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void CapsuleOverlaps(NativeBuffer shapes, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        CheckLists(shapes, CapsuleStride, offsets, tris, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_capsule_overlaps(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    /// 1 into `flags` (uint, stride 4) for each of the first `count` capsules of `shapes` that touches any triangle, else 0.
    public void CapsuleOverlapsAny(NativeBuffer shapes, NativeBuffer flags, int count)
    {
        CheckFlags(shapes, CapsuleStride, flags, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_capsule_overlaps_any(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            flags.Pointer));
    }

    /// The same for the first `count` boxes of `shapes` (stride 64).
    public void ObbOverlaps(NativeBuffer shapes, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        CheckLists(shapes, ObbStride, offsets, tris, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_obb_overlaps(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, tris == null ? IntPtr.Zero : tris.Pointer, tris == null ? 0UL : (ulong)tris.count));
    }

    public void ObbOverlapsAny(NativeBuffer shapes, NativeBuffer flags, int count)
    {
        CheckFlags(shapes, ObbStride, flags, count);
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_obb_overlaps_any(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            flags.Pointer));
    }

    static void CheckLists(NativeBuffer shapes, int stride, NativeBuffer offsets, NativeBuffer tris, int count)
    {
        if (shapes.stride != stride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeOverlaps: capsules have stride 32, boxes 64, and at least count entries");
        if (offsets.stride != 8 || count + 1 > offsets.count || (tris != null && tris.stride != 4))
            throw new ArgumentException("ShapeOverlaps: offsets are ulong with count + 1 entries, tris are uint");
        if (offsets.Context != shapes.Context || (tris != null && tris.Context != shapes.Context))
            throw new ArgumentException("ShapeOverlaps: the buffers live on different contexts");
    }

    static void CheckFlags(NativeBuffer shapes, int stride, NativeBuffer flags, int count)
    {
        if (shapes.stride != stride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeOverlaps: capsules have stride 32, boxes 64, and at least count entries");
        if (flags.stride != 4 || count > flags.count || flags.Context != shapes.Context)
            throw new ArgumentException("ShapeOverlaps: flags are uint, at least count of them, on the shapes' context");
    }
}
