// LbvhNative.cs — P/Invoke binding of liblbvh.so (include/lbvh.h) for the reference's C# host.
//
// SOURCE ONLY: this image has no C# toolchain (no dotnet/mono/csc), so this file is not compiled here;
// tests/test_abi.py checks every declaration's name and arity against include/lbvh.h.  It is the shim a
// maintainer of drzhn/UnitySimpleRaytracing adds under Assets/_Scripts/ together with the re-hosted classes
// next to it (DataBuffer / MeshBufferContainer / ComputeBufferSorter / BVHConstructor / RaytracingMeshDrawer
// `.Native.cs`, which replace the reference files of the same class names; see INTEGRATION.md).
// Struct layouts are the reference's own Sequential/Pack=16 structs (SceneDataTypes.cs), which are
// already byte-identical to lbvh_triangle / lbvh_aabb / lbvh_internal_node / lbvh_leaf_node.
using System;
using System.Runtime.InteropServices;

public static class LbvhNative
{
    const string Lib = "lbvh";   // liblbvh.so on Linux

    public const int K_CLOSEST_MAX = 32;           // LBVH_K_CLOSEST_MAX
    public const int ABI_VERSION = 11;             // LBVH_ABI_VERSION of the include/lbvh.h this file was written against
    public const int TRACE_REFERENCE = 0, TRACE_FAST = 1;
    // TRACE_FAST + the reference's choice wherever two triangles are hit at exactly the same t: every record == TRACE_REFERENCE's
    // (both fast modes: a computed t in front of its own triangle's box — fp32 noise on a grazing ray, which the un-pruned reference
    // loop reports — does not count: include/lbvh.h at the traversal flavours, DESIGN 2.4)
    public const int TRACE_FAST_EXACT = 2;
    public const uint BUILD_FAST_SCENE = 1, BUILD_RESET_NODES = 2;      // lbvh_build_scene flags

    [StructLayout(LayoutKind.Sequential)]
    public struct Hit { public float t; public uint tri; public float u, v; }

    // lbvh_ray (include/lbvh.h): a ray of the caller's own, 32 bytes; active iff tMin < tMax (RayQueries.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct Ray { public float originX, originY, originZ, tMin; public float dirX, dirY, dirZ, tMax; }

    // lbvh_sphere_ray (include/lbvh.h): a moving sphere, 32 bytes: Ray with the radius where tMin is (SphereCasts.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct SphereRay { public float originX, originY, originZ, radius; public float dirX, dirY, dirZ, tMax; }

    // lbvh_capsule_ray (include/lbvh.h): a moving capsule, 48 bytes: SphereRay and the axis, whose other end is origin + axis
    // (CapsuleCasts.cs); pad is not read
    [StructLayout(LayoutKind.Sequential)]
    public struct CapsuleRay { public float originX, originY, originZ, radius; public float dirX, dirY, dirZ, tMax; public float axisX, axisY, axisZ; public uint pad; }

    // lbvh_box_ray / lbvh_box_hit (include/lbvh.h): a moving box, 80 bytes: the centre, tMax, dir and three half-axis vectors (the box is
    // centre + s0*ax + s1*ay + s2*az, |s_i| <= 1; the pads are not read), and its record, 16 bytes: axis = the separating axis that
    // gave the time, 13 = overlapping at the start (BoxCasts.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct BoxRay { public float centreX, centreY, centreZ, tMax; public float dirX, dirY, dirZ; public uint pad0; public float axX, axY, axZ; public uint pad1; public float ayX, ayY, ayZ; public uint pad2; public float azX, azY, azZ; public uint pad3; }
    [StructLayout(LayoutKind.Sequential)]
    public struct BoxHit { public float t; public uint tri; public uint axis; public uint zero; }

    // lbvh_capsule / lbvh_obb (include/lbvh.h): a capsule (32 bytes) and an oriented box (64 bytes) where they stand, CapsuleRay and
    // BoxRay without the motion; the pads are not read (ShapeOverlaps.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct Capsule { public float originX, originY, originZ, radius; public float axisX, axisY, axisZ; public uint pad; }
    [StructLayout(LayoutKind.Sequential)]
    public struct Obb { public float centreX, centreY, centreZ; public uint pad0; public float axX, axY, axZ; public uint pad1; public float ayX, ayY, ayZ; public uint pad2; public float azX, azY, azZ; public uint pad3; }
    // lbvh_contact (include/lbvh.h): one contact of a capsule with a triangle, 32 bytes: depth = radius - distance of the axis from the
    // triangle, the contact point a + e1*u + e2*v on the triangle, the unit push-out normal, the contact point origin + axis*s on the
    // axis; tri = 0xFFFFFFFF in the none-record of lbvh_capsule_deepest (ShapeContacts.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct Contact { public float depth; public uint tri; public float u, v; public float normalX, normalY, normalZ; public float s; }
    // lbvh_segment_query / lbvh_segment_closest (include/lbvh.h): the segment origin .. origin + axis with its squared search radius
    // (active iff maxDist2 > 0), and the answer, 32 bytes: dist2 of the segment from triangle tri (2139095040 = none), the nearest
    // point a + e1*u + e2*v on the triangle, delta from it to the nearest point origin + axis*s of the segment (SegmentQueries.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct SegmentQuery { public float originX, originY, originZ, maxDist2; public float axisX, axisY, axisZ; public uint pad; }
    [StructLayout(LayoutKind.Sequential)]
    public struct SegmentClosest { public float dist2; public uint tri; public float u, v; public float deltaX, deltaY, deltaZ; public float s; }
    // lbvh_tri_distance_query / lbvh_tri_closest (include/lbvh.h): a query triangle with `skip` and its squared search radius (active iff
    // maxDist2 > 0 and all nine coordinates are finite), 48 bytes, and the answer, 32 bytes: dist2 from triangle tri (2139095040 = none),
    // the edge test that gave it (0 .. 2 the query's edges, 3 .. 5 the scene triangle's; | 8: it pierces), s on that edge, delta from the
    // scene triangle's nearest point to the query's (TriangleDistance.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct TriDistanceQuery { public float ax, ay, az; public uint skip; public float bx, by, bz; public float maxDist2; public float cx, cy, cz; public uint pad; }
    [StructLayout(LayoutKind.Sequential)]
    public struct TriClosest { public float dist2; public uint tri; public uint edge; public float s; public float deltaX, deltaY, deltaZ; public uint zero; }
    // lbvh_box_contact (include/lbvh.h): one contact of an oriented box with a triangle, 32 bytes: depth = the least push along the
    // unit normal that separates them, axis = which of the box cast's thirteen axes gave it (13: none counted), back = the push
    // along -normal on the same axis; tri = 0xFFFFFFFF in the none-record of lbvh_obb_deepest (ShapeContacts.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct BoxContact { public float depth; public uint tri; public uint axis; public float back; public float normalX, normalY, normalZ; public uint zero; }
    // lbvh_tri_segment (include/lbvh.h): where a query triangle cuts scene triangle tri, 32 bytes: the two ends p0 and p1, and edges:
    // bits 0 .. 5 which of the six edge tests passed, bits 8 .. 10 the test that gave p0, bits 12 .. 14 the one that gave p1
    // (TriangleSegments.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct PlaneSegment { public float p0X, p0Y, p0Z; public uint tri; public float p1X, p1Y, p1Z; public uint edges; }
    // lbvh_plane (include/lbvh.h): n . x + d = 0, 16 bytes; lbvh_plane_segment above: where a plane cuts scene triangle tri, 32 bytes:
    // p0 on the edge that leaves the positive side, p1 on the edge that returns to it, and edges: bits 0 .. 2 the two crossing edges,
    // bits 8 .. 9 the edge of p0, bits 12 .. 13 the edge of p1, bits 16 .. 18 the sides of v0, v1, v2 (PlaneSections.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct Plane { public float nX, nY, nZ; public float d; }
    [StructLayout(LayoutKind.Sequential)]
    public struct TriSegment { public float p0X, p0Y, p0Z; public uint tri; public float p1X, p1Y, p1Z; public uint edges; }

    // lbvh_tri_ray / lbvh_tri_cast_hit (include/lbvh.h): a triangle moving along dir without turning, 64 bytes (skip = the ORIGINAL index of
    // a scene triangle never reported, 0xFFFFFFFF = none; the pads are not read), and its record, 16 bytes: feature = the pair that gave
    // the time (0 - 2 a moving vertex on the scene face, 3 - 5 a scene vertex on the moving face, 6 + 3m + n moving edge m on scene edge
    // n at position w of it, 16 | j = intersecting at the start) (TriangleCasts.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct TriRay { public float aX, aY, aZ; public uint skip; public float bX, bY, bZ, tMax; public float cX, cY, cZ; public uint pad0; public float dirX, dirY, dirZ; public uint pad1; }
    [StructLayout(LayoutKind.Sequential)]
    public struct TriCastHit { public float t; public uint tri; public uint feature; public float w; }

    // lbvh_point_query / lbvh_closest_point (include/lbvh.h): a point with its squared search radius (active iff maxDist2 > 0) and
    // the nearest triangle's record, 16 bytes each (PointQueries.cs)
    [StructLayout(LayoutKind.Sequential)]
    public struct PointQuery { public float pX, pY, pZ, maxDist2; }
    [StructLayout(LayoutKind.Sequential)]
    public struct ClosestPoint { public float dist2; public uint tri; public float u, v; }

    // lbvh_camera (include/lbvh.h): the 16 matrix floats are plain fields, row-major m00..m33 as Unity's Matrix4x4 names
    // them, so the struct needs no `unsafe` / "allow unsafe code" project setting and marshals by value as it is.
    [StructLayout(LayoutKind.Sequential)]
    public struct Camera
    {
        public int screenWidth, screenHeight;
        public float cameraFov, nearPlane;
        public float m00, m01, m02, m03, m10, m11, m12, m13, m20, m21, m22, m23, m30, m31, m32, m33;
    }

    [StructLayout(LayoutKind.Sequential, CharSet = CharSet.Ansi)]
    public struct ProfileRow
    {
        [MarshalAs(UnmanagedType.ByValTStr, SizeConst = 48)] public string name;     // char name[48]
        public uint launches;
        public float totalMs;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct Scene
    {
        public uint n;
        public IntPtr sortedIndices, triangleAabb, internalNodes, leafNodes, bvh, triangles;
    }

    [DllImport(Lib)] public static extern int lbvh_abi_version();
    [DllImport(Lib)] public static extern int lbvh_device_count();
    [DllImport(Lib)] public static extern int lbvh_create(int deviceId, out IntPtr ctx);
    [DllImport(Lib)] public static extern int lbvh_destroy(IntPtr ctx);
    [DllImport(Lib)] public static extern IntPtr lbvh_last_error(IntPtr ctx);
    [DllImport(Lib)] public static extern int lbvh_sync(IntPtr ctx);

    [DllImport(Lib)] public static extern int lbvh_buffer_alloc(IntPtr ctx, UIntPtr count, UIntPtr stride, out IntPtr dPtr);
    [DllImport(Lib)] public static extern int lbvh_buffer_free(IntPtr ctx, IntPtr dPtr);
    [DllImport(Lib)] public static extern int lbvh_buffer_fill_u32(IntPtr ctx, IntPtr dPtr, uint value, UIntPtr nWords);
    [DllImport(Lib)] public static extern int lbvh_buffer_upload(IntPtr ctx, IntPtr dDst, IntPtr hSrc, UIntPtr bytes);
    [DllImport(Lib)] public static extern int lbvh_buffer_download(IntPtr ctx, IntPtr hDst, IntPtr dSrc, UIntPtr bytes);

    [DllImport(Lib)] public static extern int lbvh_morton_aabb(IntPtr ctx, IntPtr dTriangles, uint n, uint capacity,
        float[] boxMin, float[] boxMax, IntPtr dKeys, IntPtr dIndices, IntPtr dAabb);
    [DllImport(Lib)] public static extern int lbvh_sort_pairs(IntPtr ctx, IntPtr dKeys, IntPtr dValues, uint count);
    [DllImport(Lib)] public static extern int lbvh_distribute_keys(IntPtr ctx, IntPtr dKeys, uint n);
    [DllImport(Lib)] public static extern int lbvh_build_tree(IntPtr ctx, uint n, IntPtr dSortedKeys, IntPtr dInternal, IntPtr dLeaf);
    [DllImport(Lib)] public static extern int lbvh_refit(IntPtr ctx, uint n, IntPtr dInternal, IntPtr dLeaf,
        IntPtr dTriangleAabb, IntPtr dSortedIndices, IntPtr dBvh);
    [DllImport(Lib)] public static extern int lbvh_build_fast_scene(IntPtr ctx, ref Scene scene, float[] boxMin, float[] boxMax);
    [DllImport(Lib)] public static extern int lbvh_trace_primary(IntPtr ctx, ref Camera camera, int x0, int y0, int x1, int y1,
        ref Scene scene, int mode, IntPtr dHits, IntPtr dStats);

    [DllImport(Lib)] public static extern int lbvh_trace_primary_shard(IntPtr ctx, ref Camera camera, uint shardIndex, uint shardCount,
        ref Scene scene, int mode, IntPtr dHits, IntPtr dStats);

    [DllImport(Lib)] public static extern int lbvh_shade(IntPtr ctx, IntPtr dHits, UIntPtr count, IntPtr dTriangles,
        IntPtr dTextureRgba8, int texW, int texH, IntPtr dRgba16f);
    [DllImport(Lib)] public static extern int lbvh_compose(IntPtr ctx, IntPtr dBackgroundRgba16f, IntPtr dObjectRgba16f, UIntPtr count,
                                                            IntPtr dOutRgba16f);

    // the whole Awake() build chain in one call (per-frame rebuilds); flags: 1 = fast scene, 2 = reset node arrays
    [DllImport(Lib)] public static extern int lbvh_build_scene(IntPtr ctx, IntPtr dTriangles, uint n, uint capacity, float[] boxMin,
        float[] boxMax, IntPtr dKeys, IntPtr dIndices, IntPtr dAabb, IntPtr dInternal, IntPtr dLeaf, IntPtr dBvh, uint flags);

    // LBVH_TRACE_FAST keeps a dispatch hint from the previous frame; this drops it (the next frame runs as a first frame)
    [DllImport(Lib)] public static extern int lbvh_trace_forget(IntPtr ctx);
    // multi-GPU frames: this context's per-tile costs into a full-frame array / the merged array of all ranks back
    [DllImport(Lib)] public static extern int lbvh_trace_costs_export(IntPtr ctx, IntPtr dFrameCosts, uint tilesX, uint tilesY);
    [DllImport(Lib)] public static extern int lbvh_trace_costs_import(IntPtr ctx, IntPtr dFrameCosts, uint tilesX, uint tilesY);

    // one frame from N GPUs (BASELINE configs[2]): peer-mapped frame buffer, ordering between contexts of this process
    // (sync events) or between processes (IPC handle of the buffer + completion flags waited for on the device), and
    // packed shares for transports that want one contiguous block per GPU
    [DllImport(Lib)] public static extern int lbvh_peer_enable(IntPtr ctx, int peerDevice);
    [DllImport(Lib)] public static extern int lbvh_sync_event_create(IntPtr ctx, out IntPtr ev);
    [DllImport(Lib)] public static extern int lbvh_event_wait(IntPtr ctx, IntPtr ev);
    [DllImport(Lib)] public static extern int lbvh_ipc_export(IntPtr ctx, IntPtr dPtr, [Out] byte[] handle64);
    [DllImport(Lib)] public static extern int lbvh_ipc_import(IntPtr ctx, byte[] handle64, out IntPtr dPtr);
    [DllImport(Lib)] public static extern int lbvh_ipc_close(IntPtr ctx, IntPtr dPtr);
    // completion flags a running kernel may poll while another GPU / process stores into them: uncached device memory
    [DllImport(Lib)] public static extern int lbvh_flags_alloc(IntPtr ctx, UIntPtr nWords, out IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_frame_signal(IntPtr ctx, IntPtr dFlags, uint slot, uint value);
    [DllImport(Lib)] public static extern int lbvh_frame_wait(IntPtr ctx, IntPtr dFlags, uint nSlots, uint value);
    [DllImport(Lib)] public static extern int lbvh_trace_primary_shard_packed(IntPtr ctx, ref Camera camera, uint shardIndex, uint shardCount,
        ref Scene scene, int mode, IntPtr dPacked, IntPtr dStats);
    [DllImport(Lib)] public static extern ulong lbvh_shard_records(int width, int height, uint shardIndex, uint shardCount);
    [DllImport(Lib)] public static extern int lbvh_frame_unpack(IntPtr ctx, IntPtr dPacked, ulong shareStride, uint firstShard, uint nShards,
        uint shardCount, int width, int height, IntPtr dFrameHits);
    // a context whose work is ordered by a stream the caller owns (hipStream_t), e.g. an interop stream
    [DllImport(Lib)] public static extern int lbvh_create_on_stream(int deviceId, IntPtr hipStream, out IntPtr ctx);
    // HIP events on the context's stream
    [DllImport(Lib)] public static extern int lbvh_event_create(IntPtr ctx, out IntPtr ev);
    [DllImport(Lib)] public static extern int lbvh_event_destroy(IntPtr ctx, IntPtr ev);
    [DllImport(Lib)] public static extern int lbvh_event_record(IntPtr ctx, IntPtr ev);
    [DllImport(Lib)] public static extern int lbvh_event_elapsed_ms(IntPtr ctx, IntPtr start, IntPtr stop, out float ms);

    // dynamic scene + secondary rays (BASELINE configs[4]; extension, no reference counterpart)
    [DllImport(Lib)] public static extern int lbvh_animate(IntPtr ctx, IntPtr dRestTriangles, uint n, IntPtr dBodyIds, IntPtr dBodyCentres,
        float cosAngle, float sinAngle, IntPtr dTrianglesOut);
    [DllImport(Lib)] public static extern int lbvh_animate_build_scene(IntPtr ctx, IntPtr dRestTriangles, IntPtr dBodyIds, IntPtr dBodyCentres,
        float cosAngle, float sinAngle, IntPtr dTriangles, uint n, uint capacity, float[] boxMin, float[] boxMax, IntPtr dKeys, IntPtr dIndices,
        IntPtr dAabb, IntPtr dInternal, IntPtr dLeaf, IntPtr dBvh, uint flags);
    [DllImport(Lib)] public static extern int lbvh_path_begin(IntPtr ctx, ref Camera camera, IntPtr dStates);
    [DllImport(Lib)] public static extern int lbvh_trace_rays(IntPtr ctx, IntPtr dStates, UIntPtr count, float tMin, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_trace_closest(IntPtr ctx, IntPtr dRays, UIntPtr count, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_trace_occluded(IntPtr ctx, IntPtr dRays, UIntPtr count, ref Scene scene, IntPtr dOccluded);
    [DllImport(Lib)] public static extern int lbvh_closest_point_query(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOut);
    [DllImport(Lib)] public static extern int lbvh_within_distance(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_sphere_cast(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_sphere_cast_any(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_capsule_cast(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_capsule_cast_any(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_box_cast(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_box_cast_any(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_triangle_cast(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dHits);
    [DllImport(Lib)] public static extern int lbvh_triangle_cast_any(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_sphere_cast_all(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_capsule_cast_all(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_box_cast_all(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_triangle_cast_all(IntPtr ctx, IntPtr dCasts, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_triangle_intersections(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_triangle_intersects_any(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_triangle_intersection_segments(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dSegments, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_capsule_overlaps(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_capsule_overlaps_any(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_capsule_contacts(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dContacts, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_capsule_deepest(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOut);
    [DllImport(Lib)] public static extern int lbvh_segment_closest_point(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOut);
    [DllImport(Lib)] public static extern int lbvh_segment_within_distance(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_triangle_closest_point(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOut);
    [DllImport(Lib)] public static extern int lbvh_triangle_within_distance(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_triangle_gather_within_distance(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dRecords, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_obb_contacts(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dContacts, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_obb_deepest(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOut);
    [DllImport(Lib)] public static extern int lbvh_obb_overlaps(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_obb_overlaps_any(IntPtr ctx, IntPtr dShapes, UIntPtr count, ref Scene scene, IntPtr dFlags);
    [DllImport(Lib)] public static extern int lbvh_region_overlaps(IntPtr ctx, IntPtr dRegions, UIntPtr count, uint mode, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_region_overlaps_any(IntPtr ctx, IntPtr dRegions, UIntPtr count, uint mode, ref Scene scene, IntPtr dFlags);
    // few large regions (at most 65 536), each spread over the device: the same lists as lbvh_region_overlaps
    [DllImport(Lib)] public static extern int lbvh_region_overlaps_large(IntPtr ctx, IntPtr dRegions, UIntPtr count, uint mode, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_plane_sections(IntPtr ctx, IntPtr dPlanes, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dSegments, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_k_closest_points(IntPtr ctx, IntPtr dQueries, UIntPtr count, uint k, ref Scene scene, IntPtr dOut,
        IntPtr dFound);
    [DllImport(Lib)] public static extern int lbvh_trace_k_closest(IntPtr ctx, IntPtr dRays, UIntPtr count, uint k, ref Scene scene, IntPtr dHits,
        IntPtr dFound);
    [DllImport(Lib)] public static extern int lbvh_box_overlaps(IntPtr ctx, IntPtr dBoxes, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dTris,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_gather_within_distance(IntPtr ctx, IntPtr dQueries, UIntPtr count, ref Scene scene, IntPtr dOffsets,
        IntPtr dTris, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_gather_hits(IntPtr ctx, IntPtr dRays, UIntPtr count, ref Scene scene, IntPtr dOffsets, IntPtr dHits,
        ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_sort_hit_segments(IntPtr ctx, IntPtr dOffsets, UIntPtr count, IntPtr dHits, ulong capacity);
    [DllImport(Lib)] public static extern int lbvh_sort_index_segments(IntPtr ctx, IntPtr dOffsets, UIntPtr count, IntPtr dTris, ulong capacity);
    public const uint SortRecordsAscending = 0, SortRecordsDescending = 1, SortRecordsByTri = 2;   // LBVH_SORT_RECORDS_*
    [DllImport(Lib)] public static extern int lbvh_sort_record_segments(IntPtr ctx, IntPtr dOffsets, UIntPtr count, IntPtr dRecords, ulong capacity,
        uint order);
    [DllImport(Lib)] public static extern int lbvh_count_hits(IntPtr ctx, IntPtr dRays, UIntPtr count, ref Scene scene, IntPtr dCounts);
    [DllImport(Lib)] public static extern int lbvh_point_crossings(IntPtr ctx, IntPtr dPoints, UIntPtr count, float[] hDirs, uint nDirs, ref Scene scene,
        IntPtr dParity);
    [DllImport(Lib)] public static extern int lbvh_path_scatter(IntPtr ctx, ref Scene scene, IntPtr dHits, UIntPtr count, uint bounce, uint seed,
        float albedo, IntPtr dStates);
    [DllImport(Lib)] public static extern int lbvh_path_bounce(IntPtr ctx, ref Scene scene, IntPtr dStates, IntPtr dHits, UIntPtr count,
        uint bounce, uint seed, float albedo, float tMin);
    [DllImport(Lib)] public static extern int lbvh_path_first_bounce(IntPtr ctx, ref Camera camera, ref Scene scene, IntPtr dStates, IntPtr dHits,
        uint seed, float albedo, float tMin);
    [DllImport(Lib)] public static extern int lbvh_path_resolve(IntPtr ctx, IntPtr dStates, UIntPtr count, IntPtr dRgba16f);

    // local kernels of the multi-GPU key-range sharded sort (BASELINE configs[3])
    [DllImport(Lib)] public static extern int lbvh_key_histogram(IntPtr ctx, IntPtr dKeys, uint count, uint[] prefixes, uint nPrefixes,
        uint prefixShift, uint shift, IntPtr dHist);
    [DllImport(Lib)] public static extern int lbvh_lower_bound(IntPtr ctx, IntPtr dSortedKeys, uint count, uint[] probes, uint nProbes,
        IntPtr dPositions);

    // the same two with prefixes / probes in device memory (the sharded sort's splitter search stays on the GPU)
    [DllImport(Lib)] public static extern int lbvh_key_histogram_device(IntPtr ctx, IntPtr dKeys, uint count, IntPtr dPrefixes, uint nPrefixes,
        uint prefixShift, uint shift, IntPtr dHist);
    [DllImport(Lib)] public static extern int lbvh_lower_bound_device(IntPtr ctx, IntPtr dSortedKeys, uint count, IntPtr dProbes, uint nProbes,
        IntPtr dPositions);
    // the key-range sharded sort over N contexts of this process in one call (include/lbvh.h; MultiGpuSorter.cs)
    public const int SORT_SHARDED_MAX_CONTEXTS = 16;
    public const uint SORT_SHARDED_REPLICATE = 1;
    [DllImport(Lib)] public static extern int lbvh_sort_pairs_sharded(IntPtr[] ctxs, uint nCtx, IntPtr[] dKeys, IntPtr[] dValues,
        uint[] hCounts, IntPtr[] dOutKeys, IntPtr[] dOutValues, uint[] hOutCapacity, [Out] uint[] hOutCounts, uint flags);

    public static void Check(IntPtr ctx, int status)
    {
        if (status != 0)
            throw new InvalidOperationException($"lbvh status {status}: {Marshal.PtrToStringAnsi(lbvh_last_error(ctx))}");
    }
}
