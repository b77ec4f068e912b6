// ShapeContacts.cs — HOW DEEP a capsule is in each triangle it touches and WHICH WAY OUT (lbvh_capsule_contacts,
// lbvh_capsule_deepest, include/lbvh.h): what Unity code calls Physics.ComputePenetration, per touched triangle.  A capsule is
// LbvhNative.Capsule (ShapeOverlaps.cs); a contact is LbvhNative.Contact, 32 bytes: depth, the ORIGINAL triangle index, the contact
// point's u, v on the triangle, the unit push-out normal (from the triangle towards the axis) and the contact point's parameter s
// on the axis.  The list form is ShapeOverlaps.CapsuleOverlaps with a record in place of an index: the same offsets, the records in
// no particular order inside a capsule's segment.  The deepest form writes one record per capsule, tri = 0xFFFFFFFF and zeros for
// a capsule that touches nothing.  Twin of host.py / lbvh_host.hpp RaytracingMeshDrawer.capsule_contacts / CapsuleContacts and
// capsule_deepest / CapsuleDeepest.  No reference counterpart.  The scene is the container's; it must have been built with the
// derived traversal scene (the drawer's Awake does that).
// ObbContacts / ObbDeepest are the same two forms for an oriented box (LbvhNative.Obb, stride 64; lbvh_obb_contacts,
// lbvh_obb_deepest) with LbvhNative.BoxContact records: depth = the least push along the unit normal that frees the box from the
// triangle, axis = which of the box cast's thirteen axes gave it, back = the push along -normal.  Twin of obb_contacts / ObbContacts
// and obb_deepest / ObbDeepest.
// SOURCE ONLY (no C# toolchain in the build image).
using System;

public sealed class ShapeContacts
{
    public const int CapsuleStride = 32;
    public const int ObbStride = 64;
    public const int ContactStride = 32;
    public const uint NoTriangle = 0xFFFFFFFFu;

    readonly MeshBufferContainer _container;

    public ShapeContacts(MeshBufferContainer container) { _container = container; }

    /// The first `count` capsules of `shapes` (stride 32) -> `offsets` (ulong, stride 8, count + 1 entries) and, unless `contacts` is
    /// null, `contacts` (LbvhNative.Contact, stride 32; its whole length is the capacity).  contacts = null counts only;
    /// offsets[count] says what is needed.  Nothing is ever written at or beyond the capacity.  Asynchronous on the buffers' context.
    public void CapsuleContacts(NativeBuffer shapes, NativeBuffer offsets, NativeBuffer contacts, int count)
    {
        if (shapes.stride != CapsuleStride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeContacts: capsules have stride 32 and at least count entries");
        if (offsets.stride != 8 || count + 1 > offsets.count || (contacts != null && contacts.stride != ContactStride))
            throw new ArgumentException("ShapeContacts: offsets are ulong with count + 1 entries, contacts have stride 32");
        if (offsets.Context != shapes.Context || (contacts != null && contacts.Context != shapes.Context))
            throw new ArgumentException("ShapeContacts: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_capsule_contacts(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, contacts == null ? IntPtr.Zero : contacts.Pointer, contacts == null ? 0UL : (ulong)contacts.count));
    }

    /// The contact with the greatest depth of each of the first `count` capsules of `shapes` into `deepest` (LbvhNative.Contact,
    /// stride 32): ties to the lower triangle index; tri = NoTriangle for a capsule that touches nothing.
    public void CapsuleDeepest(NativeBuffer shapes, NativeBuffer deepest, int count)
    {
        if (shapes.stride != CapsuleStride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeContacts: capsules have stride 32 and at least count entries");
        if (deepest.stride != ContactStride || count > deepest.count || deepest.Context != shapes.Context)
            throw new ArgumentException("ShapeContacts: contacts have stride 32, at least count of them, on the shapes' context");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_capsule_deepest(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            deepest.Pointer));
    }

    /// The first `count` boxes of `shapes` (stride 64) -> `offsets` (ulong, count + 1 entries) and, unless `contacts` is null,
    /// `contacts` (LbvhNative.BoxContact, stride 32; its whole length is the capacity), exactly as CapsuleContacts.
    public void ObbContacts(NativeBuffer shapes, NativeBuffer offsets, NativeBuffer contacts, int count)
    {
        if (shapes.stride != ObbStride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeContacts: boxes have stride 64 and at least count entries");
        if (offsets.stride != 8 || count + 1 > offsets.count || (contacts != null && contacts.stride != ContactStride))
            throw new ArgumentException("ShapeContacts: offsets are ulong with count + 1 entries, contacts have stride 32");
        if (offsets.Context != shapes.Context || (contacts != null && contacts.Context != shapes.Context))
            throw new ArgumentException("ShapeContacts: the buffers live on different contexts");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_obb_contacts(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            offsets.Pointer, contacts == null ? IntPtr.Zero : contacts.Pointer, contacts == null ? 0UL : (ulong)contacts.count));
    }

    /// The contact with the greatest depth of each of the first `count` boxes of `shapes` into `deepest` (LbvhNative.BoxContact,
    /// stride 32): ties to the lower triangle index; tri = NoTriangle for a box that touches nothing.
    public void ObbDeepest(NativeBuffer shapes, NativeBuffer deepest, int count)
    {
        if (shapes.stride != ObbStride || count < 0 || count > shapes.count)
            throw new ArgumentException("ShapeContacts: boxes have stride 64 and at least count entries");
        if (deepest.stride != ContactStride || count > deepest.count || deepest.Context != shapes.Context)
            throw new ArgumentException("ShapeContacts: contacts have stride 32, at least count of them, on the shapes' context");
        LbvhNative.Scene scene = _container.NativeScene();
        LbvhNative.Check(shapes.Context, LbvhNative.lbvh_obb_deepest(shapes.Context, shapes.Pointer, (UIntPtr)(ulong)count, ref scene,
            deepest.Pointer));
    }
}
