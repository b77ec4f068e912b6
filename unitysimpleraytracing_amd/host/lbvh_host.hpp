// lbvh_host.hpp — the reference's C# host classes restated in C++ over the C ABI (include/lbvh.h).
//
// The reference's host side is compiled C# against UnityEngine (no C# toolchain in this image), so
// the host layer above the C ABI is C++: same class names, constructor arguments, method names and
// call order as Assets/_Scripts/{DataBuffer,MeshBufferContainer,ComputeBufferSorter,BVHConstructor,
// RaytracingMeshDrawer}.cs.  Each method is one C-ABI call; nothing here computes.  Errors: the
// reference logs and carries on; here every failing call throws lbvh::Error with the library's text.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/lbvh.h"

namespace lbvh {

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string& m) : std::runtime_error("lbvh status " + std::to_string(s) + ": " + m), status(s) {}
};

inline void check(lbvh_context* ctx, lbvh_status s)
{
    if (s != LBVH_OK) throw Error(s, lbvh_last_error(ctx));
}

// The implicit Unity graphics device + IShaderContainer (Assets/_Scripts/ShaderContainer.cs:6-40).
class Context {
public:
    explicit Context(int device_id = 0)
    {
        check_abi();
        check(nullptr, lbvh_create(device_id, &ctx_));
    }
    // a context whose work is ordered by a stream the caller owns (hipStream_t)
    Context(int device_id, void* hip_stream)
    {
        check_abi();
        check(nullptr, lbvh_create_on_stream(device_id, hip_stream, &ctx_));
    }
    ~Context() { if (ctx_) lbvh_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    lbvh_context* get() const { return ctx_; }
    void sync() { check(ctx_, lbvh_sync(ctx_)); }
    // LBVH_TRACE_FAST keeps the previous frame's per-tile costs as a dispatch hint: drop it (the next frame is a first frame)
    void trace_forget() { check(ctx_, lbvh_trace_forget(ctx_)); }
    static int device_count() { return lbvh_device_count(); }
private:
    static void check_abi()
    {
        if (lbvh_abi_version() != LBVH_ABI_VERSION)
            throw Error(LBVH_ERR_INVALID_ARG, "liblbvh.so was built from another include/lbvh.h (ABI version)");
    }
    lbvh_context* ctx_ = nullptr;
};

// A HIP event on the context's stream (measurement: elapsed_ms waits for `stop`).
class Event {
public:
    explicit Event(Context& ctx) : ctx_(ctx) { check(ctx_.get(), lbvh_event_create(ctx_.get(), &ev_)); }
    ~Event() { if (ev_) lbvh_event_destroy(ctx_.get(), ev_); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    void record() { check(ctx_.get(), lbvh_event_record(ctx_.get(), ev_)); }
    static float elapsed_ms(Event& start, Event& stop)
    {
        float ms = 0.0f;
        check(start.ctx_.get(), lbvh_event_elapsed_ms(start.ctx_.get(), start.ev_, stop.ev_, &ms));
        return ms;
    }
private:
    Context& ctx_;
    void* ev_ = nullptr;
};

// An ORDERING event (lbvh_sync_event_create): recorded on one context's stream, waited for by another's, on the device.
class SyncEvent {
public:
    explicit SyncEvent(Context& ctx) : ctx_(ctx) { check(ctx_.get(), lbvh_sync_event_create(ctx_.get(), &ev_)); }
    ~SyncEvent() { if (ev_) lbvh_event_destroy(ctx_.get(), ev_); }
    SyncEvent(const SyncEvent&) = delete;
    SyncEvent& operator=(const SyncEvent&) = delete;
    void record() { check(ctx_.get(), lbvh_event_record(ctx_.get(), ev_)); }
    // everything enqueued on `waiter` after this call starts after the work recorded before record()
    void make_wait(Context& waiter) { check(waiter.get(), lbvh_event_wait(waiter.get(), ev_)); }
private:
    Context& ctx_;
    void* ev_ = nullptr;
};

// Assets/_Scripts/DataBuffer.cs
template <typename T>
class DataBuffer {
public:
    DataBuffer(Context& ctx, size_t size) : ctx_(ctx), local_(size)                       // :25-30
    {
        check(ctx_.get(), lbvh_buffer_alloc(ctx_.get(), size, sizeof(T), &device_));
    }
    DataBuffer(Context& ctx, size_t size, uint32_t initial_word) : DataBuffer(ctx, size)  // :14-23
    {
        Fill(initial_word);
    }
    ~DataBuffer() { Dispose(); }
    DataBuffer(const DataBuffer&) = delete;
    DataBuffer& operator=(const DataBuffer&) = delete;

    void* DeviceBuffer() const { return device_; }
    std::vector<T>& LocalBuffer() { return local_; }
    size_t Size() const { return local_.size(); }

    void Fill(uint32_t word, bool mirror = true)
    {
        check(ctx_.get(), lbvh_buffer_fill_u32(ctx_.get(), device_, word, local_.size() * sizeof(T) / 4));
        if (mirror) {
            uint32_t* w = reinterpret_cast<uint32_t*>(local_.data());
            for (size_t i = 0; i < local_.size() * sizeof(T) / 4; i++) w[i] = word;
        }
    }
    void GetData()                                                                         // :50-54
    {
        check(ctx_.get(), lbvh_buffer_download(ctx_.get(), local_.data(), device_, local_.size() * sizeof(T)));
    }
    void Sync()                                                                            // :56-60
    {
        check(ctx_.get(), lbvh_buffer_upload(ctx_.get(), device_, local_.data(), local_.size() * sizeof(T)));
    }
    void Dispose()                                                                         // :72-75
    {
        if (device_) { lbvh_buffer_free(ctx_.get(), device_); device_ = nullptr; }
    }
private:
    Context& ctx_;
    void* device_ = nullptr;
    std::vector<T> local_;
};

inline uint32_t CapacityFor(uint32_t n, uint32_t tile = 1024) { return (n + tile - 1) / tile * tile; }

// ---- plane builders for lbvh_region_overlaps: conveniences, computed in double and rounded once to float.  The contract is on the
// planes (include/lbvh.h), not on these builders: a plane {nx, ny, nz, d} keeps n . x + d >= 0, normals point inward. ----------------
inline void SetPlane(lbvh_region& r, int j, double nx, double ny, double nz, double d)
{
    r.plane[j][0] = (float)nx; r.plane[j][1] = (float)ny; r.plane[j][2] = (float)nz; r.plane[j][3] = (float)d;
}

// the box [lo, hi]: unit axis normals, d = -lo / +hi (exact for float bounds: in TOUCHING mode the region is lbvh_box_overlaps' box)
inline lbvh_region AabbPlanes(const float lo[3], const float hi[3])
{
    lbvh_region r;
    for (int k = 0; k < 3; k++) {
        SetPlane(r, 2 * k, k == 0, k == 1, k == 2, -(double)lo[k]);
        SetPlane(r, 2 * k + 1, -(double)(k == 0), -(double)(k == 1), -(double)(k == 2), (double)hi[k]);
    }
    return r;
}

// the oriented box { centre + sum_k s_k * axes[k] : |s_k| <= half_extents[k] }; the rows of `axes` are normalised here and
// assumed orthogonal
inline lbvh_region ObbPlanes(const float centre[3], const float axes[3][3], const float half_extents[3])
{
    lbvh_region r;
    for (int k = 0; k < 3; k++) {
        const double len = std::sqrt((double)axes[k][0] * axes[k][0] + (double)axes[k][1] * axes[k][1] + (double)axes[k][2] * axes[k][2]);
        const double n[3] = {axes[k][0] / len, axes[k][1] / len, axes[k][2] / len};
        const double along = n[0] * centre[0] + n[1] * centre[1] + n[2] * centre[2];
        SetPlane(r, 2 * k, n[0], n[1], n[2], half_extents[k] - along);
        SetPlane(r, 2 * k + 1, -n[0], -n[1], -n[2], half_extents[k] + along);
    }
    return r;
}

// The view frustum of `cam` in the convention of lbvh_trace_primary's ray generation: the eye at camera_to_world * (0, 0, 0, 1),
// looking along the camera's -z, the image plane at depth near_plane 2 * near_plane * camera_fov high (camera_fov: the tangent of
// half the vertical angle) and screen_width / screen_height times as wide.  Planes: left, right, bottom, top (through the eye), near
// (depth >= near_plane), far (depth <= far); depth is measured along the view axis.  camera_to_world is taken as a rigid motion
// times a uniform scale (what a camera has): its inverse's rotation part is its transpose over the squared scale.
inline lbvh_region FrustumPlanes(const lbvh_camera& cam, float far_depth)
{
    const double t = cam.camera_fov, ta = t * (double)cam.screen_width / (double)cam.screen_height;
    const double c[6][4] = {{1, 0, -ta, 0}, {-1, 0, -ta, 0}, {0, 1, -t, 0}, {0, -1, -t, 0}, {0, 0, -1, -(double)cam.near_plane}, {0, 0, 1, far_depth}};
    const float* m = cam.camera_to_world;                     // row-major 4 x 4
    const double s2 = (double)m[0] * m[0] + (double)m[4] * m[4] + (double)m[8] * m[8];
    lbvh_region r;
    for (int j = 0; j < 6; j++) {
        // x_c = R^T (x_w - T) / s2, so n_w = R n_c / s2 and d_w = d_c - n_w . T
        double n[3];
        for (int k = 0; k < 3; k++) n[k] = (m[4 * k] * c[j][0] + m[4 * k + 1] * c[j][1] + m[4 * k + 2] * c[j][2]) / s2;
        SetPlane(r, j, n[0], n[1], n[2], c[j][3] - (n[0] * m[3] + n[1] * m[7] + n[2] * m[11]));
    }
    return r;
}

// Assets/_Scripts/MeshBufferContainer.cs
class MeshBufferContainer {
public:
    MeshBufferContainer(Context& ctx, const std::vector<lbvh_triangle>& triangles, uint32_t capacity = 0)
        : ctx_(ctx), n_((uint32_t)triangles.size()), cap_(capacity ? capacity : CapacityFor(n_)),
          keys_(ctx, cap_), index_(ctx, cap_), tris_(ctx, cap_), aabb_(ctx, cap_), bvh_(ctx, cap_),
          leaf_(ctx, cap_, LBVH_NULL), internal_(ctx, cap_, LBVH_NULL)                     // :108-115
    {
        std::memcpy(tris_.LocalBuffer().data(), triangles.data(), triangles.size() * sizeof(lbvh_triangle));
        tris_.Sync();                                                                      // :150
        GenerateKeys();                                                                    // :123-151 as one kernel
    }
    void GenerateKeys()
    {
        const float mn[3] = {-125.0f, -125.0f, -125.0f}, mx[3] = {125.0f, 125.0f, 125.0f}; // Whole, :9-15
        check(ctx_.get(), lbvh_morton_aabb(ctx_.get(), (const lbvh_triangle*)tris_.DeviceBuffer(), n_, cap_, mn, mx,
                                           (uint32_t*)keys_.DeviceBuffer(), (uint32_t*)index_.DeviceBuffer(),
                                           (lbvh_aabb*)aabb_.DeviceBuffer()));
    }
    void DistributeKeys()                                                                  // :154-169
    {
        check(ctx_.get(), lbvh_distribute_keys(ctx_.get(), (uint32_t*)keys_.DeviceBuffer(), n_));
    }
    void GetAllGpuData()                                                                   // :171-196
    {
        keys_.GetData(); index_.GetData(); tris_.GetData(); aabb_.GetData(); bvh_.GetData(); leaf_.GetData();
        internal_.GetData();
        for (uint32_t i = 0; i < n_; i++)
            if (leaf_.LocalBuffer()[i].index == LBVH_NULL && leaf_.LocalBuffer()[i].parent == LBVH_NULL)
                throw Error(-100, "LEAF CORRUPTED " + std::to_string(i));                  // :183-186
        for (uint32_t i = 0; i + 1 < n_; i++)
            if (internal_.LocalBuffer()[i].index == LBVH_NULL && internal_.LocalBuffer()[i].parent == LBVH_NULL)
                throw Error(-101, "INTERNAL CORRUPTED " + std::to_string(i));              // :191-194
    }
    lbvh_scene Scene() const
    {
        lbvh_scene s;
        s.n = n_;
        s.sorted_indices = (const uint32_t*)index_.DeviceBuffer();
        s.triangle_aabb = (const lbvh_aabb*)aabb_.DeviceBuffer();
        s.internal_nodes = (const lbvh_internal_node*)internal_.DeviceBuffer();
        s.leaf_nodes = (const lbvh_leaf_node*)leaf_.DeviceBuffer();
        s.bvh = (const lbvh_aabb*)bvh_.DeviceBuffer();
        s.triangles = (const lbvh_triangle*)tris_.DeviceBuffer();
        return s;
    }
    uint32_t TrianglesLength() const { return n_; }
    uint32_t Capacity() const { return cap_; }
    DataBuffer<uint32_t>& Keys() { return keys_; }
    DataBuffer<uint32_t>& TriangleIndex() { return index_; }
    DataBuffer<lbvh_triangle>& TriangleData() { return tris_; }
    DataBuffer<lbvh_aabb>& TriangleAABB() { return aabb_; }
    DataBuffer<lbvh_aabb>& BvhData() { return bvh_; }
    DataBuffer<lbvh_leaf_node>& BvhLeafNode() { return leaf_; }
    DataBuffer<lbvh_internal_node>& BvhInternalNode() { return internal_; }
private:
    Context& ctx_;
    uint32_t n_, cap_;
    DataBuffer<uint32_t> keys_, index_;
    DataBuffer<lbvh_triangle> tris_;
    DataBuffer<lbvh_aabb> aabb_, bvh_;
    DataBuffer<lbvh_leaf_node> leaf_;
    DataBuffer<lbvh_internal_node> internal_;
};

// Assets/_Scripts/ComputeBufferSorter.cs — dataLength only bounds the validation, Sort() covers the
// whole padded buffers (every dispatch of the reference covers DATA_ARRAY_COUNT, :107,116).
class ComputeBufferSorter {
public:
    ComputeBufferSorter(Context& ctx, uint32_t data_length, DataBuffer<uint32_t>& keys, DataBuffer<uint32_t>& values)
        : ctx_(ctx), data_length_(data_length), keys_(keys), values_(values) {}
    void Sort()                                                                            // :100-126
    {
        check(ctx_.get(), lbvh_sort_pairs(ctx_.get(), (uint32_t*)keys_.DeviceBuffer(), (uint32_t*)values_.DeviceBuffer(),
                                          (uint32_t)keys_.Size()));
    }
    bool ValidateSortedData()                                                              // :150-177
    {
        keys_.GetData();
        for (uint32_t i = 1; i < data_length_; i++)
            if (keys_.LocalBuffer()[i] < keys_.LocalBuffer()[i - 1]) return false;
        return true;
    }
private:
    Context& ctx_;
    uint32_t data_length_;
    DataBuffer<uint32_t>& keys_;
    DataBuffer<uint32_t>& values_;
};

// Assets/_Scripts/BVHConstructor.cs
class BVHConstructor {
public:
    BVHConstructor(Context& ctx, uint32_t triangles_count, DataBuffer<uint32_t>& sorted_morton_codes,
                   DataBuffer<uint32_t>& sorted_triangle_indices, DataBuffer<lbvh_aabb>& triangle_aabb,
                   DataBuffer<lbvh_internal_node>& internal_nodes, DataBuffer<lbvh_leaf_node>& leaf_nodes,
                   DataBuffer<lbvh_aabb>& bvh_data)
        : ctx_(ctx), n_(triangles_count), keys_(sorted_morton_codes), idx_(sorted_triangle_indices), aabb_(triangle_aabb),
          internal_(internal_nodes), leaf_(leaf_nodes), bvh_(bvh_data) {}
    void ConstructTree()                                                                   // :61-64
    {
        check(ctx_.get(), lbvh_build_tree(ctx_.get(), n_, (const uint32_t*)keys_.DeviceBuffer(),
                                          (lbvh_internal_node*)internal_.DeviceBuffer(), (lbvh_leaf_node*)leaf_.DeviceBuffer()));
    }
    void ConstructBVH()                                                                    // :66-69
    {
        check(ctx_.get(), lbvh_refit(ctx_.get(), n_, (const lbvh_internal_node*)internal_.DeviceBuffer(),
                                     (const lbvh_leaf_node*)leaf_.DeviceBuffer(), (const lbvh_aabb*)aabb_.DeviceBuffer(),
                                     (const uint32_t*)idx_.DeviceBuffer(), (lbvh_aabb*)bvh_.DeviceBuffer()));
    }
private:
    Context& ctx_;
    uint32_t n_;
    DataBuffer<uint32_t>& keys_;
    DataBuffer<uint32_t>& idx_;
    DataBuffer<lbvh_aabb>& aabb_;
    DataBuffer<lbvh_internal_node>& internal_;
    DataBuffer<lbvh_leaf_node>& leaf_;
    DataBuffer<lbvh_aabb>& bvh_;
};

// Assets/_Scripts/RaytracingMeshDrawer.cs: Awake() = build chain (:30-51), Update() = per-frame
// dispatch (:76-84) producing hit records.
class RaytracingMeshDrawer {
public:
    RaytracingMeshDrawer(Context& ctx, const std::vector<lbvh_triangle>& mesh) : ctx_(ctx), mesh_(mesh) {}
    void Awake()
    {
        container_.reset(new MeshBufferContainer(ctx_, mesh_));                                            // :34
        sorter_.reset(new ComputeBufferSorter(ctx_, container_->TrianglesLength(), container_->Keys(),
                                              container_->TriangleIndex()));                               // :36
        sorter_->Sort();                                                                                   // :37
        container_->DistributeKeys();                                                                      // :39
        bvh_.reset(new BVHConstructor(ctx_, container_->TrianglesLength(), container_->Keys(), container_->TriangleIndex(),
                                      container_->TriangleAABB(), container_->BvhInternalNode(),
                                      container_->BvhLeafNode(), container_->BvhData()));                  // :41-48
        bvh_->ConstructTree();                                                                             // :50
        bvh_->ConstructBVH();                                                                              // :51
        const lbvh_scene s = container_->Scene();
        const float mn[3] = {-125.0f, -125.0f, -125.0f}, mx[3] = {125.0f, 125.0f, 125.0f};   // MeshBufferContainer.Whole
        check(ctx_.get(), lbvh_build_fast_scene(ctx_.get(), &s, mn, mx));
    }
    // screenWidth/screenHeight/cameraFov/cameraToWorldMatrix + Dispatch, :78-83
    void Update(const lbvh_camera& cam, int mode = LBVH_TRACE_FAST)
    {
        const size_t rays = (size_t)cam.screen_width * cam.screen_height;
        if (!hits_ || hits_->Size() < rays) hits_.reset(new DataBuffer<lbvh_hit>(ctx_, rays));
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_primary(ctx_.get(), &cam, 0, 0, cam.screen_width, cam.screen_height, &s, mode,
                                             (lbvh_hit*)hits_->DeviceBuffer(), nullptr));
    }
    // one GPU's share of the frame (every shard_count-th group of 8 adjacent 8x8-pixel tiles), one launch; the hit buffer
    // has the full frame's layout and only the shard's pixels are written (BASELINE configs[2]: BVH replicated, rays sharded)
    void UpdateShard(const lbvh_camera& cam, uint32_t shard_index, uint32_t shard_count, int mode = LBVH_TRACE_FAST)
    {
        const size_t rays = (size_t)cam.screen_width * cam.screen_height;
        if (!hits_ || hits_->Size() < rays) hits_.reset(new DataBuffer<lbvh_hit>(ctx_, rays));
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_primary_shard(ctx_.get(), &cam, shard_index, shard_count, &s, mode,
                                                   (lbvh_hit*)hits_->DeviceBuffer(), nullptr));
    }
    // rays of the caller's own (lbvh_ray: origin, t_min, dir, t_max) over the derived scene: the closest hit of each, or
    // whether anything lies in (t_min, t_max) — 1 / 0 per ray (lbvh_trace_closest / lbvh_trace_occluded; asynchronous)
    void TraceClosest(const DataBuffer<lbvh_ray>& rays, DataBuffer<lbvh_hit>& hits)
    {
        if (hits.Size() < rays.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TraceClosest: fewer hit records than rays");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_closest(ctx_.get(), (const lbvh_ray*)rays.DeviceBuffer(), rays.Size(), &s, (lbvh_hit*)hits.DeviceBuffer()));
    }
    void TraceOccluded(const DataBuffer<lbvh_ray>& rays, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < rays.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TraceOccluded: fewer flags than rays");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_occluded(ctx_.get(), (const lbvh_ray*)rays.DeviceBuffer(), rays.Size(), &s, (uint32_t*)flags.DeviceBuffer()));
    }
    // points of the caller's own (lbvh_point_query: p, max_dist2) over the derived scene: the nearest triangle of each, or
    // whether any lies within the radius — 1 / 0 per point (lbvh_closest_point_query / lbvh_within_distance; asynchronous)
    void ClosestPoints(const DataBuffer<lbvh_point_query>& queries, DataBuffer<lbvh_closest_point>& out)
    {
        if (out.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "ClosestPoints: fewer records than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_closest_point_query(ctx_.get(), (const lbvh_point_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                   (lbvh_closest_point*)out.DeviceBuffer()));
    }
    void WithinDistance(const DataBuffer<lbvh_point_query>& queries, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "WithinDistance: fewer flags than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_within_distance(ctx_.get(), (const lbvh_point_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                               (uint32_t*)flags.DeviceBuffer()));
    }
    // moving spheres of the caller's own (lbvh_sphere_ray: origin, radius, dir, t_max) over the derived scene: the first contact of
    // each — {t, tri, u, v}, the centre at origin + dir * t, (u, v) the barycentrics of the contact point — or whether it touches
    // anything on its way, 1 / 0 per cast (lbvh_sphere_cast / lbvh_sphere_cast_any; asynchronous)
    void SphereCast(const DataBuffer<lbvh_sphere_ray>& casts, DataBuffer<lbvh_hit>& hits)
    {
        if (hits.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "SphereCast: fewer hit records than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_sphere_cast(ctx_.get(), (const lbvh_sphere_ray*)casts.DeviceBuffer(), casts.Size(), &s, (lbvh_hit*)hits.DeviceBuffer()));
    }
    void SphereCastAny(const DataBuffer<lbvh_sphere_ray>& casts, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "SphereCastAny: fewer flags than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_sphere_cast_any(ctx_.get(), (const lbvh_sphere_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint32_t*)flags.DeviceBuffer()));
    }
    // moving capsules of the caller's own (lbvh_capsule_ray: origin, radius, dir, t_max, axis; the axis is the segment from origin
    // to origin + axis) over the derived scene: the first contact of each — {t, tri, u, v}, the axis starting at origin + dir * t,
    // (u, v) the barycentrics of the contact point on the triangle — or whether it touches anything on its way, 1 / 0 per cast
    // (lbvh_capsule_cast / lbvh_capsule_cast_any; asynchronous)
    void CapsuleCast(const DataBuffer<lbvh_capsule_ray>& casts, DataBuffer<lbvh_hit>& hits)
    {
        if (hits.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleCast: fewer hit records than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_cast(ctx_.get(), (const lbvh_capsule_ray*)casts.DeviceBuffer(), casts.Size(), &s, (lbvh_hit*)hits.DeviceBuffer()));
    }
    void CapsuleCastAny(const DataBuffer<lbvh_capsule_ray>& casts, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleCastAny: fewer flags than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_cast_any(ctx_.get(), (const lbvh_capsule_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint32_t*)flags.DeviceBuffer()));
    }
    // moving boxes of the caller's own (lbvh_box_ray: centre, t_max, dir and the three half-axis vectors ax, ay, az; the box is
    // centre + s0*ax + s1*ay + s2*az, |s_i| <= 1) over the derived scene: the first contact of each — {t, tri, axis, 0}, the centre
    // at centre + dir * t, axis the separating axis that gave the time (LBVH_BOX_AXIS_START: overlapping at the start) — or
    // whether it touches anything on its way, 1 / 0 per cast (lbvh_box_cast / lbvh_box_cast_any; asynchronous)
    void BoxCast(const DataBuffer<lbvh_box_ray>& casts, DataBuffer<lbvh_box_hit>& hits)
    {
        if (hits.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "BoxCast: fewer hit records than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_box_cast(ctx_.get(), (const lbvh_box_ray*)casts.DeviceBuffer(), casts.Size(), &s, (lbvh_box_hit*)hits.DeviceBuffer()));
    }
    void BoxCastAny(const DataBuffer<lbvh_box_ray>& casts, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "BoxCastAny: fewer flags than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_box_cast_any(ctx_.get(), (const lbvh_box_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint32_t*)flags.DeviceBuffer()));
    }
    // moving triangles of the caller's own (lbvh_tri_ray: a, skip, b, t_max, c, dir; the triangle is at a + dir * t, b + dir * t,
    // c + dir * t) over the derived scene: the first contact of each — {t, tri, feature, w}, feature the pair that gave the time
    // (0 - 2 a moving vertex on the scene face, 3 - 5 a scene vertex on the moving face, 6 + 3m + n moving edge m on scene edge n
    // at Q + F * w, LBVH_TRI_CAST_START | j: intersecting at the start) — or whether it touches anything on its way, 1 / 0 per
    // cast (lbvh_triangle_cast / lbvh_triangle_cast_any; asynchronous)
    void TriangleCast(const DataBuffer<lbvh_tri_ray>& casts, DataBuffer<lbvh_tri_cast_hit>& hits)
    {
        if (hits.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TriangleCast: fewer hit records than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_cast(ctx_.get(), (const lbvh_tri_ray*)casts.DeviceBuffer(), casts.Size(), &s, (lbvh_tri_cast_hit*)hits.DeviceBuffer()));
    }
    void TriangleCastAny(const DataBuffer<lbvh_tri_ray>& casts, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < casts.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TriangleCastAny: fewer flags than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_cast_any(ctx_.get(), (const lbvh_tri_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint32_t*)flags.DeviceBuffer()));
    }
    // the k nearest triangles of each point (1 <= k <= LBVH_K_CLOSEST_MAX): out[q * k + j] = the j-th nearest of query q, ties by
    // the lower triangle index, padded with none-records; found (optional): the number of real records per row
    // (lbvh_k_closest_points; asynchronous)
    void KClosestPoints(const DataBuffer<lbvh_point_query>& queries, uint32_t k, DataBuffer<lbvh_closest_point>& out,
                        DataBuffer<uint32_t>* found = nullptr)
    {
        if (out.Size() < queries.Size() * (size_t)k) throw Error(LBVH_ERR_INVALID_ARG, "KClosestPoints: fewer than k records per query");
        if (found && found->Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "KClosestPoints: fewer counts than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_k_closest_points(ctx_.get(), (const lbvh_point_query*)queries.DeviceBuffer(), queries.Size(), k, &s,
                                                (lbvh_closest_point*)out.DeviceBuffer(), found ? (uint32_t*)found->DeviceBuffer() : nullptr));
    }
    // WHICH triangles touch each box / lie within each point's radius, as a CSR list (lbvh_box_overlaps /
    // lbvh_gather_within_distance; asynchronous): offsets[k] .. offsets[k + 1] = query k's segment of `tris` (ORIGINAL triangle
    // indices, in no particular order).  tris == nullptr counts only; otherwise its size is the capacity: nothing is written
    // beyond it, and offsets[queries.Size()] says what was needed.
    void BoxOverlaps(const DataBuffer<lbvh_aabb>& boxes, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < boxes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "BoxOverlaps: offsets needs one entry more than boxes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_box_overlaps(ctx_.get(), (const lbvh_aabb*)boxes.DeviceBuffer(), boxes.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                            tris ? (uint32_t*)tris->DeviceBuffer() : nullptr, tris ? (uint64_t)tris->Size() : 0));
    }
    void GatherWithinDistance(const DataBuffer<lbvh_point_query>& queries, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < queries.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "GatherWithinDistance: offsets needs one entry more than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_gather_within_distance(ctx_.get(), (const lbvh_point_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                      (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                                      tris ? (uint64_t)tris->Size() : 0));
    }
    // WHICH scene triangles each query triangle intersects — the narrow phase behind BoxOverlaps —, as the same CSR list, or one
    // flag per query (lbvh_triangle_intersections / lbvh_triangle_intersects_any; asynchronous).  skip = the ORIGINAL index of a
    // scene triangle that is never reported (a mesh against itself), LBVH_NULL for none.
    void TriangleIntersections(const DataBuffer<lbvh_tri_query>& queries, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < queries.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "TriangleIntersections: offsets needs one entry more than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_intersections(ctx_.get(), (const lbvh_tri_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                      (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                                      tris ? (uint64_t)tris->Size() : 0));
    }
    void TriangleIntersectsAny(const DataBuffer<lbvh_tri_query>& queries, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TriangleIntersectsAny: fewer flags than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_intersects_any(ctx_.get(), (const lbvh_tri_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                       (uint32_t*)flags.DeviceBuffer()));
    }
    // WHERE each query triangle cuts every scene triangle it intersects: TriangleIntersections with a lbvh_tri_segment record (the
    // two ends p0, p1, tri, and edges: which of the six edge tests passed and which gave each end) in place of an index, the same
    // offsets (lbvh_triangle_intersection_segments; asynchronous)
    void TriangleIntersectionSegments(const DataBuffer<lbvh_tri_query>& queries, DataBuffer<uint64_t>& offsets,
                                      DataBuffer<lbvh_tri_segment>* segments = nullptr)
    {
        if (offsets.Size() < queries.Size() + 1)
            throw Error(LBVH_ERR_INVALID_ARG, "TriangleIntersectionSegments: offsets needs one entry more than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_intersection_segments(ctx_.get(), (const lbvh_tri_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                              (uint64_t*)offsets.DeviceBuffer(),
                                                              segments ? (lbvh_tri_segment*)segments->DeviceBuffer() : nullptr,
                                                              segments ? (uint64_t)segments->Size() : 0));
    }
    // WHICH triangles each capsule (lbvh_capsule: origin, radius, axis) or oriented box (lbvh_obb: centre and the three half-axis
    // vectors) touches where it stands — the start overlap of CapsuleCast / BoxCast without a direction —, as the same CSR list, or
    // one flag per shape (lbvh_capsule_overlaps / _any, lbvh_obb_overlaps / _any; asynchronous)
    void CapsuleOverlaps(const DataBuffer<lbvh_capsule>& shapes, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < shapes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleOverlaps: offsets needs one entry more than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_overlaps(ctx_.get(), (const lbvh_capsule*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                                (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                                tris ? (uint64_t)tris->Size() : 0));
    }
    void CapsuleOverlapsAny(const DataBuffer<lbvh_capsule>& shapes, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < shapes.Size()) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleOverlapsAny: fewer flags than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_overlaps_any(ctx_.get(), (const lbvh_capsule*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                                    (uint32_t*)flags.DeviceBuffer()));
    }
    // HOW DEEP each capsule is in every triangle it touches and which way out: CapsuleOverlaps with a lbvh_contact record (depth,
    // tri, u, v, the unit push-out normal, s) in place of an index, the same offsets; or the deepest record per capsule, tri =
    // LBVH_NULL for one that touches nothing (lbvh_capsule_contacts / lbvh_capsule_deepest; asynchronous)
    void CapsuleContacts(const DataBuffer<lbvh_capsule>& shapes, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_contact>* contacts = nullptr)
    {
        if (offsets.Size() < shapes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleContacts: offsets needs one entry more than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_contacts(ctx_.get(), (const lbvh_capsule*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                                (uint64_t*)offsets.DeviceBuffer(), contacts ? (lbvh_contact*)contacts->DeviceBuffer() : nullptr,
                                                contacts ? (uint64_t)contacts->Size() : 0));
    }
    void CapsuleDeepest(const DataBuffer<lbvh_capsule>& shapes, DataBuffer<lbvh_contact>& out)
    {
        if (out.Size() < shapes.Size()) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleDeepest: fewer records than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_deepest(ctx_.get(), (const lbvh_capsule*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                               (lbvh_contact*)out.DeviceBuffer()));
    }
    // segments of the caller's own (lbvh_segment_query: origin, max_dist2, axis) over the derived scene: the nearest triangle of each
    // — {dist2, tri, u, v, delta, s}: a capsule's clearance is sqrt(dist2) - radius — or whether any lies within the radius, 1 / 0 per
    // segment (lbvh_segment_closest_point / lbvh_segment_within_distance; asynchronous)
    void SegmentClosestPoints(const DataBuffer<lbvh_segment_query>& queries, DataBuffer<lbvh_segment_closest>& out)
    {
        if (out.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "SegmentClosestPoints: fewer records than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_segment_closest_point(ctx_.get(), (const lbvh_segment_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                     (lbvh_segment_closest*)out.DeviceBuffer()));
    }
    void SegmentWithinDistance(const DataBuffer<lbvh_segment_query>& queries, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "SegmentWithinDistance: fewer flags than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_segment_within_distance(ctx_.get(), (const lbvh_segment_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                       (uint32_t*)flags.DeviceBuffer()));
    }
    // triangles of the caller's own (lbvh_tri_distance_query: a, skip, b, max_dist2, c) over the derived scene: the nearest scene
    // triangle of each — {dist2, tri, edge, s, delta}: the distance between two meshes is the least record's sqrt(dist2) — or whether
    // any lies within the radius, 1 / 0 per query (lbvh_triangle_closest_point / lbvh_triangle_within_distance; asynchronous)
    void TriangleClosestPoints(const DataBuffer<lbvh_tri_distance_query>& queries, DataBuffer<lbvh_tri_closest>& out)
    {
        if (out.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TriangleClosestPoints: fewer records than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_closest_point(ctx_.get(), (const lbvh_tri_distance_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                      (lbvh_tri_closest*)out.DeviceBuffer()));
    }
    void TriangleWithinDistance(const DataBuffer<lbvh_tri_distance_query>& queries, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < queries.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TriangleWithinDistance: fewer flags than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_within_distance(ctx_.get(), (const lbvh_tri_distance_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                        (uint32_t*)flags.DeviceBuffer()));
    }
    // EVERY scene triangle within the radius of each query triangle, one lbvh_tri_closest record per pair (what TriangleClosestPoints
    // would write were that triangle the only one) as a CSR list in no particular order inside a segment; records = nullptr counts
    // only, offsets[queries] says what is needed (lbvh_triangle_gather_within_distance; asynchronous)
    void TriangleGatherWithinDistance(const DataBuffer<lbvh_tri_distance_query>& queries, DataBuffer<uint64_t>& offsets,
                                      DataBuffer<lbvh_tri_closest>* records = nullptr)
    {
        if (offsets.Size() < queries.Size() + 1)
            throw Error(LBVH_ERR_INVALID_ARG, "TriangleGatherWithinDistance: offsets needs one entry more than queries");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_gather_within_distance(ctx_.get(), (const lbvh_tri_distance_query*)queries.DeviceBuffer(), queries.Size(), &s,
                                                               (uint64_t*)offsets.DeviceBuffer(),
                                                               records ? (lbvh_tri_closest*)records->DeviceBuffer() : nullptr,
                                                               records ? (uint64_t)records->Size() : 0));
    }
    // The same for oriented boxes: ObbOverlaps with a lbvh_box_contact record (depth, tri, the axis of the thirteen that gave it,
    // back, the unit push-out normal) in place of an index; or the deepest record per box (lbvh_obb_contacts / lbvh_obb_deepest)
    void ObbContacts(const DataBuffer<lbvh_obb>& shapes, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_box_contact>* contacts = nullptr)
    {
        if (offsets.Size() < shapes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "ObbContacts: offsets needs one entry more than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_obb_contacts(ctx_.get(), (const lbvh_obb*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                            (uint64_t*)offsets.DeviceBuffer(), contacts ? (lbvh_box_contact*)contacts->DeviceBuffer() : nullptr,
                                            contacts ? (uint64_t)contacts->Size() : 0));
    }
    void ObbDeepest(const DataBuffer<lbvh_obb>& shapes, DataBuffer<lbvh_box_contact>& out)
    {
        if (out.Size() < shapes.Size()) throw Error(LBVH_ERR_INVALID_ARG, "ObbDeepest: fewer records than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_obb_deepest(ctx_.get(), (const lbvh_obb*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                           (lbvh_box_contact*)out.DeviceBuffer()));
    }
    void ObbOverlaps(const DataBuffer<lbvh_obb>& shapes, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < shapes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "ObbOverlaps: offsets needs one entry more than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_obb_overlaps(ctx_.get(), (const lbvh_obb*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                            (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                            tris ? (uint64_t)tris->Size() : 0));
    }
    void ObbOverlapsAny(const DataBuffer<lbvh_obb>& shapes, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < shapes.Size()) throw Error(LBVH_ERR_INVALID_ARG, "ObbOverlapsAny: fewer flags than shapes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_obb_overlaps_any(ctx_.get(), (const lbvh_obb*)shapes.DeviceBuffer(), shapes.Size(), &s,
                                                (uint32_t*)flags.DeviceBuffer()));
    }
    // WHICH triangles lie in each convex region of six planes (a frustum, an oriented box, a selection window), as the same CSR
    // list, or one flag per region (lbvh_region_overlaps / lbvh_region_overlaps_any; asynchronous).  mode: LBVH_REGION_TOUCHING —
    // the triangle's own box is not wholly outside any plane — or LBVH_REGION_CONTAINED — it is wholly inside every plane.
    // FrustumPlanes / ObbPlanes / AabbPlanes below make the planes.
    void RegionOverlaps(const DataBuffer<lbvh_region>& regions, uint32_t mode, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < regions.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "RegionOverlaps: offsets needs one entry more than regions");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_region_overlaps(ctx_.get(), (const lbvh_region*)regions.DeviceBuffer(), regions.Size(), mode, &s,
                                               (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                               tris ? (uint64_t)tris->Size() : 0));
    }
    // RegionOverlaps for few large regions (one frustum, a cascade, a marquee selection; at most LBVH_REGION_LARGE_MAX_COUNT): every
    // region is spread over the device.  The same offsets and, per segment, the same set of indices, in another order
    // (lbvh_region_overlaps_large; asynchronous).
    void RegionOverlapsLarge(const DataBuffer<lbvh_region>& regions, uint32_t mode, DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>* tris = nullptr)
    {
        if (offsets.Size() < regions.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "RegionOverlapsLarge: offsets needs one entry more than regions");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_region_overlaps_large(ctx_.get(), (const lbvh_region*)regions.DeviceBuffer(), regions.Size(), mode, &s,
                                                     (uint64_t*)offsets.DeviceBuffer(), tris ? (uint32_t*)tris->DeviceBuffer() : nullptr,
                                                     tris ? (uint64_t)tris->Size() : 0));
    }
    // WHERE each plane (lbvh_plane: n . x + d = 0) cuts the mesh: one lbvh_plane_segment per cut triangle — p0 on the edge that
    // leaves the positive side, p1 on the edge that returns to it, tri, and edges: bits 0 .. 2 the two crossing edges, bits 8 .. 9 /
    // 12 .. 13 the edges of p0 / p1, bits 16 .. 18 the sides of the three vertices —, every plane spread over the device; at most
    // LBVH_PLANE_SECTIONS_MAX_COUNT planes.  A contour is stitched by (triangle, edge): the p1-edge of a record is the p0-edge of
    // the neighbour across it (lbvh_plane_sections; asynchronous).
    void PlaneSections(const DataBuffer<lbvh_plane>& planes, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_plane_segment>* segments = nullptr)
    {
        if (offsets.Size() < planes.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "PlaneSections: offsets needs one entry more than planes");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_plane_sections(ctx_.get(), (const lbvh_plane*)planes.DeviceBuffer(), planes.Size(), &s,
                                              (uint64_t*)offsets.DeviceBuffer(),
                                              segments ? (lbvh_plane_segment*)segments->DeviceBuffer() : nullptr,
                                              segments ? (uint64_t)segments->Size() : 0));
    }
    void RegionOverlapsAny(const DataBuffer<lbvh_region>& regions, uint32_t mode, DataBuffer<uint32_t>& flags)
    {
        if (flags.Size() < regions.Size()) throw Error(LBVH_ERR_INVALID_ARG, "RegionOverlapsAny: fewer flags than regions");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_region_overlaps_any(ctx_.get(), (const lbvh_region*)regions.DeviceBuffer(), regions.Size(), mode, &s,
                                                   (uint32_t*)flags.DeviceBuffer()));
    }
    // how many triangles each ray crosses in (t_min, t_max), and crossing parities of points along fixed directions — bit j of a
    // point's word: the count of the ray from it along dirs[j] (x, y, z; 1 .. 32 of them), AND 1 (lbvh_count_hits /
    // lbvh_point_crossings; asynchronous).  Inside / outside: more than half of the bits set.
    void CountHits(const DataBuffer<lbvh_ray>& rays, DataBuffer<uint32_t>& counts)
    {
        if (counts.Size() < rays.Size()) throw Error(LBVH_ERR_INVALID_ARG, "CountHits: fewer counts than rays");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_count_hits(ctx_.get(), (const lbvh_ray*)rays.DeviceBuffer(), rays.Size(), &s, (uint32_t*)counts.DeviceBuffer()));
    }
    // the first k hits along each ray (1 <= k <= LBVH_K_CLOSEST_MAX): hits[q * k + j] = the j-th nearest hit of ray q, ties by the
    // lower triangle index, padded with miss records; found (optional): the number of real records per row
    // (lbvh_trace_k_closest; asynchronous)
    void TraceKClosest(const DataBuffer<lbvh_ray>& rays, uint32_t k, DataBuffer<lbvh_hit>& hits, DataBuffer<uint32_t>* found = nullptr)
    {
        if (hits.Size() < rays.Size() * (size_t)k) throw Error(LBVH_ERR_INVALID_ARG, "TraceKClosest: fewer than k hit records per ray");
        if (found && found->Size() < rays.Size()) throw Error(LBVH_ERR_INVALID_ARG, "TraceKClosest: fewer counts than rays");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_k_closest(ctx_.get(), (const lbvh_ray*)rays.DeviceBuffer(), rays.Size(), k, &s,
                                               (lbvh_hit*)hits.DeviceBuffer(), found ? (uint32_t*)found->DeviceBuffer() : nullptr));
    }
    // EVERY hit along each ray, as a CSR list (lbvh_gather_hits; asynchronous): offsets[q] .. offsets[q + 1] = ray q's segment of
    // `hits` ({t, tri, u, v} records, IN NO PARTICULAR ORDER: sort a segment by (t, tri) if an order is needed).  hits == nullptr
    // counts only; otherwise its size is the capacity: nothing is written beyond it, and offsets[rays.Size()] says what was needed.
    void GatherHits(const DataBuffer<lbvh_ray>& rays, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_hit>* hits = nullptr)
    {
        if (offsets.Size() < rays.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "GatherHits: offsets needs one entry more than rays");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_gather_hits(ctx_.get(), (const lbvh_ray*)rays.DeviceBuffer(), rays.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                           hits ? (lbvh_hit*)hits->DeviceBuffer() : nullptr, hits ? (uint64_t)hits->Size() : 0));
    }
    // EVERY triangle each sweep touches before its t_max, as a CSR list exactly as GatherHits writes it (lbvh_sphere_cast_all /
    // lbvh_capsule_cast_all / lbvh_box_cast_all; asynchronous): offsets[q] .. offsets[q + 1] = cast q's segment of `hits`, the
    // records the first-contact call would write were that triangle the first ({t, tri, u, v}; boxes: {t, tri, axis, 0}), IN NO
    // PARTICULAR ORDER — SortHitSegments orders them by (t, tri).  hits == nullptr counts only; otherwise its size is the capacity.
    void SphereCastAll(const DataBuffer<lbvh_sphere_ray>& casts, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_hit>* hits = nullptr)
    {
        if (offsets.Size() < casts.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "SphereCastAll: offsets needs one entry more than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_sphere_cast_all(ctx_.get(), (const lbvh_sphere_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                               hits ? (lbvh_hit*)hits->DeviceBuffer() : nullptr, hits ? (uint64_t)hits->Size() : 0));
    }
    void CapsuleCastAll(const DataBuffer<lbvh_capsule_ray>& casts, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_hit>* hits = nullptr)
    {
        if (offsets.Size() < casts.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "CapsuleCastAll: offsets needs one entry more than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_capsule_cast_all(ctx_.get(), (const lbvh_capsule_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                                hits ? (lbvh_hit*)hits->DeviceBuffer() : nullptr, hits ? (uint64_t)hits->Size() : 0));
    }
    void BoxCastAll(const DataBuffer<lbvh_box_ray>& casts, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_box_hit>* hits = nullptr)
    {
        if (offsets.Size() < casts.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "BoxCastAll: offsets needs one entry more than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_box_cast_all(ctx_.get(), (const lbvh_box_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                            hits ? (lbvh_box_hit*)hits->DeviceBuffer() : nullptr, hits ? (uint64_t)hits->Size() : 0));
    }
    // the same for moving triangles (lbvh_triangle_cast_all): TriangleCast's record {t, tri, feature, w} of every triangle touched,
    // `skip` never among them
    void TriangleCastAll(const DataBuffer<lbvh_tri_ray>& casts, DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_tri_cast_hit>* hits = nullptr)
    {
        if (offsets.Size() < casts.Size() + 1) throw Error(LBVH_ERR_INVALID_ARG, "TriangleCastAll: offsets needs one entry more than casts");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_triangle_cast_all(ctx_.get(), (const lbvh_tri_ray*)casts.DeviceBuffer(), casts.Size(), &s, (uint64_t*)offsets.DeviceBuffer(),
                                                 hits ? (lbvh_tri_cast_hit*)hits->DeviceBuffer() : nullptr, hits ? (uint64_t)hits->Size() : 0));
    }
    // Every segment of a gathered list into (t, tri) order / ascending index order, in place, on the device (lbvh_sort_hit_segments,
    // lbvh_sort_index_segments; asynchronous, no scratch, the path tracer's live-path list is kept).  The data buffer's size is the
    // capacity: pass the buffer that was given to GatherHits / the overlap query.  A segment that did not fit is left as it is.
    void SortHitSegments(const DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_hit>& hits, size_t count)
    {
        if (offsets.Size() < count + 1) throw Error(LBVH_ERR_INVALID_ARG, "SortHitSegments: offsets needs count + 1 entries");
        check(ctx_.get(), lbvh_sort_hit_segments(ctx_.get(), (const uint64_t*)offsets.DeviceBuffer(), count, (lbvh_hit*)hits.DeviceBuffer(),
                                                 (uint64_t)hits.Size()));
    }
    // the same for the lbvh_box_hit records of BoxCastAll: t and tri are the same two words, axis travels with its record
    void SortHitSegments(const DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_box_hit>& hits, size_t count)
    {
        if (offsets.Size() < count + 1) throw Error(LBVH_ERR_INVALID_ARG, "SortHitSegments: offsets needs count + 1 entries");
        check(ctx_.get(), lbvh_sort_hit_segments(ctx_.get(), (const uint64_t*)offsets.DeviceBuffer(), count, (lbvh_hit*)hits.DeviceBuffer(),
                                                 (uint64_t)hits.Size()));
    }
    // and for the lbvh_tri_cast_hit records of TriangleCastAll: feature and w travel with their record
    void SortHitSegments(const DataBuffer<uint64_t>& offsets, DataBuffer<lbvh_tri_cast_hit>& hits, size_t count)
    {
        if (offsets.Size() < count + 1) throw Error(LBVH_ERR_INVALID_ARG, "SortHitSegments: offsets needs count + 1 entries");
        check(ctx_.get(), lbvh_sort_hit_segments(ctx_.get(), (const uint64_t*)offsets.DeviceBuffer(), count, (lbvh_hit*)hits.DeviceBuffer(),
                                                 (uint64_t)hits.Size()));
    }
    void SortIndexSegments(const DataBuffer<uint64_t>& offsets, DataBuffer<uint32_t>& tris, size_t count)
    {
        if (offsets.Size() < count + 1) throw Error(LBVH_ERR_INVALID_ARG, "SortIndexSegments: offsets needs count + 1 entries");
        check(ctx_.get(), lbvh_sort_index_segments(ctx_.get(), (const uint64_t*)offsets.DeviceBuffer(), count, (uint32_t*)tris.DeviceBuffer(),
                                                   (uint64_t)tris.Size()));
    }
    // The same pass for the 32-byte records of CapsuleContacts / ObbContacts (order LBVH_SORT_RECORDS_DESCENDING: deepest first, the
    // first record is the _deepest call's), TriangleGatherWithinDistance (LBVH_SORT_RECORDS_ASCENDING: nearest first) and
    // TriangleIntersectionSegments / PlaneSections (LBVH_SORT_RECORDS_BY_TRI), lbvh_sort_record_segments: T is any 32-byte record.
    template <typename T>
    void SortRecordSegments(const DataBuffer<uint64_t>& offsets, DataBuffer<T>& records, size_t count, uint32_t order)
    {
        static_assert(sizeof(T) == 32, "SortRecordSegments: a 32-byte record");
        if (offsets.Size() < count + 1) throw Error(LBVH_ERR_INVALID_ARG, "SortRecordSegments: offsets needs count + 1 entries");
        check(ctx_.get(), lbvh_sort_record_segments(ctx_.get(), (const uint64_t*)offsets.DeviceBuffer(), count, (void*)records.DeviceBuffer(),
                                                    (uint64_t)records.Size(), order));
    }
    void PointCrossings(const DataBuffer<lbvh_point_query>& points, const std::vector<float>& dirs, DataBuffer<uint32_t>& parity)
    {
        if (parity.Size() < points.Size()) throw Error(LBVH_ERR_INVALID_ARG, "PointCrossings: fewer parity words than points");
        if (dirs.size() % 3 != 0) throw Error(LBVH_ERR_INVALID_ARG, "PointCrossings: dirs is not a list of x, y, z");
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_point_crossings(ctx_.get(), (const lbvh_point_query*)points.DeviceBuffer(), points.Size(), dirs.data(),
                                               (uint32_t)(dirs.size() / 3), &s, (uint32_t*)parity.DeviceBuffer()));
    }
    // _objectDrawer.SetTexture("_meshTexture", ...) :61 — RGBA8, row 0 at v = 0
    void SetTexture(const std::vector<uint8_t>& rgba8, int width, int height)
    {
        tex_.reset(new DataBuffer<uint32_t>(ctx_, (size_t)width * height));
        std::memcpy(tex_->LocalBuffer().data(), rgba8.data(), (size_t)width * height * 4);
        tex_->Sync();
        tex_w_ = width; tex_h_ = height;
    }
    // the shading tail of the Raytracing kernel (Raytracing.compute:178-184) -> RGBA16F, 4 halves per pixel
    void Shade()
    {
        const size_t rays = hits_->Size();
        if (!image_ || image_->Size() < rays) image_.reset(new DataBuffer<uint64_t>(ctx_, rays));
        check(ctx_.get(), lbvh_shade(ctx_.get(), (const lbvh_hit*)hits_->DeviceBuffer(), rays,
                                     (const lbvh_triangle*)container_->TriangleData().DeviceBuffer(),
                                     (const uint8_t*)tex_->DeviceBuffer(), tex_w_, tex_h_, (uint16_t*)image_->DeviceBuffer()));
    }
    // OnRenderImage :86-90 — Graphics.Blit(src, dest, _imageComposerMaterial): the shaded image over the camera's own
    // rendering (RGBA16F, 4 halves per pixel), in place in `src_dest`
    void OnRenderImage(DataBuffer<uint64_t>& src_dest)
    {
        check(ctx_.get(), lbvh_compose(ctx_.get(), (const uint16_t*)src_dest.DeviceBuffer(), (const uint16_t*)image_->DeviceBuffer(),
                                       hits_->Size(), (uint16_t*)src_dest.DeviceBuffer()));
    }
    // per-frame rebuild on the same buffers (dynamic scenes): the whole Awake() chain in one call
    void Rebuild()
    {
        MeshBufferContainer& c = *container_;
        const float mn[3] = {-125.0f, -125.0f, -125.0f}, mx[3] = {125.0f, 125.0f, 125.0f};   // MeshBufferContainer.Whole
        check(ctx_.get(), lbvh_build_scene(ctx_.get(), (const lbvh_triangle*)c.TriangleData().DeviceBuffer(), c.TrianglesLength(),
                                           c.Capacity(), mn, mx, (uint32_t*)c.Keys().DeviceBuffer(),
                                           (uint32_t*)c.TriangleIndex().DeviceBuffer(), (lbvh_aabb*)c.TriangleAABB().DeviceBuffer(),
                                           (lbvh_internal_node*)c.BvhInternalNode().DeviceBuffer(),
                                           (lbvh_leaf_node*)c.BvhLeafNode().DeviceBuffer(), (lbvh_aabb*)c.BvhData().DeviceBuffer(),
                                           LBVH_BUILD_FAST_SCENE | LBVH_BUILD_RESET_NODES));
    }
    // this GPU's share of the frame written into `frame` — a full-frame buffer that may live on ANOTHER GPU (peer-mapped:
    // lbvh_peer_enable on this context first): the records travel as the tiles finish, nothing is copied afterwards
    void UpdateShardInto(const lbvh_camera& cam, uint32_t shard_index, uint32_t shard_count, lbvh_hit* frame, int mode = LBVH_TRACE_FAST)
    {
        const lbvh_scene s = container_->Scene();
        check(ctx_.get(), lbvh_trace_primary_shard(ctx_.get(), &cam, shard_index, shard_count, &s, mode, frame, nullptr));
    }
    DataBuffer<uint64_t>& Image() { return *image_; }
    MeshBufferContainer& Container() { return *container_; }
    DataBuffer<lbvh_hit>& Hits() { return *hits_; }
private:
    Context& ctx_;
    std::vector<lbvh_triangle> mesh_;
    std::unique_ptr<MeshBufferContainer> container_;
    std::unique_ptr<ComputeBufferSorter> sorter_;
    std::unique_ptr<BVHConstructor> bvh_;
    std::unique_ptr<DataBuffer<lbvh_hit>> hits_;
    std::unique_ptr<DataBuffer<uint32_t>> tex_;
    std::unique_ptr<DataBuffer<uint64_t>> image_;
    int tex_w_ = 0, tex_h_ = 0;
};

// One frame from N GPUs driven by ONE process — what a Unity MonoBehaviour is (Assets/_Scripts/RaytracingMeshDrawer.cs:30-84
// runs Awake / Update on the main thread of one process) and BASELINE configs[2] asks for: BVH replicated, rays sharded, no
// collective.  One Context per entry of `devices` (a device may appear more than once: logical ranks on one GPU, which is
// how the tests run it on a one-GPU box), each with its own replica of the scene; Awake() / Rebuild() enqueue every
// replica's build round-robin (all calls are asynchronous, so the N GPUs build side by side); Update() has every context
// trace its share of the frame straight into ONE full-frame hit buffer that lives on the first device — peer-mapped
// stores over xGMI while the tiles finish, no second pass — and makes the first context's stream wait for the others'
// completion events on the device.  Whatever the first context enqueues next (lbvh_shade, a download, Unity's blit) sees a
// whole frame; the host never blocks inside Update().  The next Update() may only overwrite the buffer once the owner is
// done reading the previous frame: the owner records `consumed_` at the top of Update() and every other stream waits for it.
class MultiGpuDrawer {
public:
    MultiGpuDrawer(const std::vector<int>& devices, const std::vector<lbvh_triangle>& mesh)
    {
        if (devices.empty()) throw Error(LBVH_ERR_INVALID_ARG, "MultiGpuDrawer: no devices");
        for (int d : devices) {
            contexts_.emplace_back(new Context(d));
            drawers_.emplace_back(new RaytracingMeshDrawer(*contexts_.back(), mesh));
            done_.emplace_back(new SyncEvent(*contexts_.back()));
        }
        consumed_.reset(new SyncEvent(*contexts_[0]));
        for (size_t r = 1; r < contexts_.size(); ++r)            // rank r stores into the owner's memory
            check(contexts_[r]->get(), lbvh_peer_enable(contexts_[r]->get(), devices[0]));
    }
    ~MultiGpuDrawer()
    {
        try { Sync(); } catch (const Error&) {}                            // no rank may still be storing into the frame buffer
    }
    size_t Ranks() const { return contexts_.size(); }
    Context& Owner() { return *contexts_[0]; }
    RaytracingMeshDrawer& Drawer(size_t rank) { return *drawers_[rank]; }
    void Awake() { for (auto& d : drawers_) d->Awake(); }                  // replicas: deterministic, bit-identical trees
    void Rebuild() { for (auto& d : drawers_) d->Rebuild(); }              // per-frame rebuilds of dynamic scenes
    void Update(const lbvh_camera& cam, int mode = LBVH_TRACE_FAST)
    {
        const size_t rays = (size_t)cam.screen_width * cam.screen_height;
        if (!frame_ || frame_->Size() < rays) {
            Sync();                                                        // nobody may still be writing the old buffer
            frame_.reset(new DataBuffer<lbvh_hit>(*contexts_[0], rays));
        }
        const uint32_t n = (uint32_t)contexts_.size();
        consumed_->record();                                               // the owner's reads of the previous frame end here
        for (uint32_t r = 1; r < n; ++r) consumed_->make_wait(*contexts_[r]);
        for (uint32_t r = 0; r < n; ++r) {                                 // round-robin enqueue: N GPUs trace side by side
            drawers_[r]->UpdateShardInto(cam, r, n, (lbvh_hit*)frame_->DeviceBuffer(), mode);
            if (r != 0) done_[r]->record();
        }
        for (uint32_t r = 1; r < n; ++r) done_[r]->make_wait(*contexts_[0]);   // the gather: a device-side wait, no copy
    }
    // the whole frame, on the first device; valid for work enqueued on Owner() after Update()
    DataBuffer<lbvh_hit>& Hits() { return *frame_; }
    void Sync() { for (auto& c : contexts_) c->sync(); }
private:
    // (destruction order: buffers and events before their contexts)
    std::vector<std::unique_ptr<Context>> contexts_;
    std::vector<std::unique_ptr<RaytracingMeshDrawer>> drawers_;
    std::vector<std::unique_ptr<SyncEvent>> done_;
    std::unique_ptr<SyncEvent> consumed_;
    std::unique_ptr<DataBuffer<lbvh_hit>> frame_;
};

// ComputeBufferSorter over N contexts of one process (BASELINE configs[3]; twin of host.py MultiGpuSorter): one context per
// entry of `devices` (a device may repeat) and ONE lbvh_sort_pairs_sharded call per Sort().  Block r = the first counts[r]
// pairs of Keys(r) / Values(r); Sort() leaves context q's slice of the globally sorted sequence in OutKeys(q) / OutValues(q)
// (replicate: the whole sequence on every context) and returns the slice lengths.  Buffers are grown on demand; the outputs
// hold as many pairs as the whole sequence (any slice may need all of them).
class MultiGpuSorter {
public:
    explicit MultiGpuSorter(const std::vector<int>& devices)
    {
        if (devices.empty() || devices.size() > LBVH_SORT_SHARDED_MAX_CONTEXTS)
            throw Error(LBVH_ERR_INVALID_ARG, "MultiGpuSorter: 1 .. 16 contexts");
        for (int d : devices) contexts_.emplace_back(new Context(d));
        keys_.resize(devices.size());
        values_.resize(devices.size());
        out_keys_.resize(devices.size());
        out_values_.resize(devices.size());
    }
    ~MultiGpuSorter()
    {
        try { Sync(); } catch (const Error&) {}
    }
    size_t Ranks() const { return contexts_.size(); }
    Context& Ctx(size_t r) { return *contexts_[r]; }
    DataBuffer<uint32_t>& Keys(size_t r) { return *keys_[r]; }
    DataBuffer<uint32_t>& Values(size_t r) { return *values_[r]; }
    DataBuffer<uint32_t>& OutKeys(size_t r) { return *out_keys_[r]; }
    DataBuffer<uint32_t>& OutValues(size_t r) { return *out_values_[r]; }
    // host blocks -> the contexts' input buffers (blocking uploads)
    void SetBlocks(const std::vector<std::vector<uint32_t>>& keys, const std::vector<std::vector<uint32_t>>& values)
    {
        if (keys.size() != contexts_.size() || values.size() != contexts_.size())
            throw Error(LBVH_ERR_INVALID_ARG, "MultiGpuSorter::SetBlocks: one block per context");
        size_t total = 0;
        for (size_t r = 0; r < keys.size(); ++r) total += keys[r].size();
        counts_.assign(contexts_.size(), 0);
        for (size_t r = 0; r < contexts_.size(); ++r) {
            if (keys[r].size() != values[r].size()) throw Error(LBVH_ERR_INVALID_ARG, "MultiGpuSorter::SetBlocks: keys / values lengths");
            grow(keys_[r], r, keys[r].size());
            grow(values_[r], r, values[r].size());
            grow(out_keys_[r], r, total);
            grow(out_values_[r], r, total);
            std::copy(keys[r].begin(), keys[r].end(), keys_[r]->LocalBuffer().begin());
            std::copy(values[r].begin(), values[r].end(), values_[r]->LocalBuffer().begin());
            keys_[r]->Sync();
            values_[r]->Sync();
            counts_[r] = (uint32_t)keys[r].size();
        }
    }
    std::vector<uint32_t> Sort(bool replicate = false)
    {
        const size_t n = contexts_.size();
        std::vector<lbvh_context*> ctxs(n);
        std::vector<uint32_t*> k(n), v(n), ok(n), ov(n);
        std::vector<uint32_t> cap(n), out(n);
        for (size_t r = 0; r < n; ++r) {
            if (!keys_[r]) throw Error(LBVH_ERR_INVALID_ARG, "MultiGpuSorter::Sort: SetBlocks first");
            ctxs[r] = contexts_[r]->get();
            k[r] = (uint32_t*)keys_[r]->DeviceBuffer();
            v[r] = (uint32_t*)values_[r]->DeviceBuffer();
            ok[r] = (uint32_t*)out_keys_[r]->DeviceBuffer();
            ov[r] = (uint32_t*)out_values_[r]->DeviceBuffer();
            cap[r] = (uint32_t)out_keys_[r]->Size();
        }
        check(ctxs[0], lbvh_sort_pairs_sharded(ctxs.data(), (uint32_t)n, k.data(), v.data(), counts_.data(), ok.data(), ov.data(),
                                               cap.data(), out.data(), replicate ? LBVH_SORT_SHARDED_REPLICATE : 0u));
        return out;
    }
    void Sync() { for (auto& c : contexts_) c->sync(); }
private:
    void grow(std::unique_ptr<DataBuffer<uint32_t>>& b, size_t r, size_t size)
    {
        if (!b || b->Size() < size) b.reset(new DataBuffer<uint32_t>(*contexts_[r], size ? size : 1));
    }
    // (destruction order: buffers before their contexts)
    std::vector<std::unique_ptr<Context>> contexts_;
    std::vector<std::unique_ptr<DataBuffer<uint32_t>>> keys_, values_, out_keys_, out_values_;
    std::vector<uint32_t> counts_;
};

// BASELINE configs[4] (extension): rigid bodies rotate every frame, the LBVH is rebuilt, primary rays + `bounces`
// diffuse bounces at 1 spp.  Twin of host.py DynamicPathTracer.
class DynamicPathTracer {
public:
    DynamicPathTracer(Context& ctx, const std::vector<lbvh_triangle>& rest, const std::vector<uint32_t>& body_ids,
                      const std::vector<float>& body_centres_xyzw, float t_min = 1e-3f, float albedo = 0.7f, uint32_t seed = 1)
        : ctx_(ctx), drawer_(ctx, rest), rest_(ctx, rest.size()), body_(ctx, body_ids.size()),
          centres_(ctx, body_centres_xyzw.size()), t_min_(t_min), albedo_(albedo), seed_(seed)
    {
        drawer_.Awake();
        rest_.LocalBuffer() = rest;                 rest_.Sync();
        body_.LocalBuffer() = body_ids;             body_.Sync();
        centres_.LocalBuffer() = body_centres_xyzw; centres_.Sync();
    }
    // the bodies turned to `angle` and the whole LBVH rebuilt, one call (= lbvh_animate + RaytracingMeshDrawer::Rebuild)
    void Animate(float angle)
    {
        MeshBufferContainer& c = drawer_.Container();
        const float mn[3] = {-125.0f, -125.0f, -125.0f}, mx[3] = {125.0f, 125.0f, 125.0f};   // MeshBufferContainer.Whole
        check(ctx_.get(), lbvh_animate_build_scene(ctx_.get(), (const lbvh_triangle*)rest_.DeviceBuffer(), (const uint32_t*)body_.DeviceBuffer(),
                                                   (const float*)centres_.DeviceBuffer(), std::cos(angle), std::sin(angle),
                                                   (lbvh_triangle*)c.TriangleData().DeviceBuffer(), c.TrianglesLength(), c.Capacity(), mn, mx,
                                                   (uint32_t*)c.Keys().DeviceBuffer(), (uint32_t*)c.TriangleIndex().DeviceBuffer(),
                                                   (lbvh_aabb*)c.TriangleAABB().DeviceBuffer(), (lbvh_internal_node*)c.BvhInternalNode().DeviceBuffer(),
                                                   (lbvh_leaf_node*)c.BvhLeafNode().DeviceBuffer(), (lbvh_aabb*)c.BvhData().DeviceBuffer(),
                                                   LBVH_BUILD_FAST_SCENE | LBVH_BUILD_RESET_NODES));
    }
    void Render(const lbvh_camera& cam, uint32_t bounces = 4)
    {
        const size_t rays = (size_t)cam.screen_width * cam.screen_height;
        if (!states_ || states_->Size() < rays) {
            states_.reset(new DataBuffer<lbvh_path_state>(ctx_, rays));
            image_.reset(new DataBuffer<uint64_t>(ctx_, rays));
        }
        drawer_.Update(cam);                                                     // primary rays: the packet kernel
        const lbvh_scene s = drawer_.Container().Scene();
        lbvh_path_state* st = (lbvh_path_state*)states_->DeviceBuffer();
        lbvh_hit* hits = (lbvh_hit*)drawer_.Hits().DeviceBuffer();
        // bounce b = scatter at segment b's hits + trace of segment b + 1; the first one makes the path states from the camera
        if (bounces == 0) check(ctx_.get(), lbvh_path_begin(ctx_.get(), &cam, st));
        else check(ctx_.get(), lbvh_path_first_bounce(ctx_.get(), &cam, &s, st, hits, seed_, albedo_, t_min_));
        for (uint32_t b = 1; b < bounces; ++b)
            check(ctx_.get(), lbvh_path_bounce(ctx_.get(), &s, st, hits, rays, b, seed_, albedo_, t_min_));
        check(ctx_.get(), lbvh_path_scatter(ctx_.get(), &s, hits, rays, bounces, seed_, albedo_, st));
        check(ctx_.get(), lbvh_path_resolve(ctx_.get(), st, rays, (uint16_t*)image_->DeviceBuffer()));
    }
    DataBuffer<uint64_t>& Image() { return *image_; }
    RaytracingMeshDrawer& Drawer() { return drawer_; }
private:
    Context& ctx_;
    RaytracingMeshDrawer drawer_;
    DataBuffer<lbvh_triangle> rest_;
    DataBuffer<uint32_t> body_;
    DataBuffer<float> centres_;
    std::unique_ptr<DataBuffer<lbvh_path_state>> states_;
    std::unique_ptr<DataBuffer<uint64_t>> image_;
    float t_min_, albedo_;
    uint32_t seed_;
};

}  // namespace lbvh
