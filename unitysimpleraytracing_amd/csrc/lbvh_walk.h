// lbvh_walk.h — what the per-lane walkers over the derived traversal scene and their launchers share: the path tracer's, the
// plain rays' and the queries still beside them (lbvh_path.hip), the ray queries' (lbvh_query_ray.hip) and the shared launches'
// (lbvh_walk.hip).  Internal.
// The device side sits in the unnamed namespace, like the kernels that use it (their mangled names carry it, and a kernel's name is
// what the device-code identity gate and the profiles go by).  So lbvh_wide_node is a type of each file's own, and walk_launch
// below, which has external linkage and a member `const lbvh_wide_node*`, formally BREAKS the one-definition rule: its
// definitions in the files that include this header name different types.  Accepted knowingly: the layout is the same in every
// file (one pointer), only walk_launch's own name is mangled into begin_walk and use_wide_nodes, and no file looks through `wn`
// at another file's nodes on the host.  A build with link-time optimisation or type-based checking across files has to settle
// this first — by taking lbvh_wide_node out of the unnamed namespace, which renames every four-wide kernel.
#pragma once
#include <algorithm>
#include <type_traits>
#include "lbvh_common.h"
#include "lbvh_rt.h"

namespace {

// ---- a lane's stack ------------------------------------------------------------------------------------------
// The first kRayStackLds entries of a lane's stack are in LDS (4 KB per wave: all 32 wave slots of a CU fit; with 34
// entries in LDS only 18 did and the four bounces took 1.70 ms instead of 1.46), deeper ones — rare: the fused tree
// is walked near child first — in a per-wave slab of global memory, up to 64 entries in all like the reference's
// stack (Raytracing.compute:113).
constexpr int kRayStackLds = 16;
constexpr int kRayStackDeep = 48;
// the four-wide walk (lbvh_wide_node below): three siblings can wait per level.  (Neither stack can overflow on a tree of this library:
// the derived tree is a radix tree over unique 32-bit keys, at most 32 levels deep — 32 waiting entries for the binary walk,
// 3 x 32 for the four-wide one, whose levels are binary levels or pairs of them.)
constexpr int kWideStackLds = 16;
constexpr int kWideStackDeep = 112;

// ---- the grid and the ray scratch ------------------------------------------------------------------------------
// One ray per lane; a wave owns a run of consecutive entries of the live-ray list and REFILLS a lane from it as
// soon as that lane's ray is finished, so a wave's run time is the sum of its rays' steps / 64 and not the step
// count of its longest ray (incoherent rays: mean ~100 steps, maxima of several hundred).  The grid is a fixed
// number of waves (every wave slot of the chip once) and the live rays are dealt out evenly: at least 64 per wave.
// Measured per frame of 4 bounces: no refill 3.75 ms; fixed runs of 128 / 256 / 512 rays 1.83 / 2.62 / 4.44 ms
// (long runs leave most of the chip empty).
constexpr uint32_t kRayWaves = 8192;
// ray scratch: [live-ray count (256 B) | indices of the live rays | deep stack slabs of the launch's waves]
static inline uint32_t ray_waves_of(size_t count) { return (uint32_t)std::min<size_t>(kRayWaves, (count + LBVH_WAVE - 1) / LBVH_WAVE); }
// the slab is indexed by blockIdx.x: one launch needs ray_waves_of(count) of them (a 64-ray call: 12 KB, not 96 MB)
static inline size_t deep_bytes(size_t count) { return (size_t)ray_waves_of(count) * std::max(kWideStackDeep, kRayStackDeep) * LBVH_WAVE * 4; }
static inline size_t list_bytes(size_t count) { return (count * 4 + 255) & ~(size_t)255; }
// ray scratch: [two live-ray counters (256 B: words 0 and 16) | live-ray list 0 | live-ray list 1 | deep stack slabs].  Two lists
// take turns (round 5): lbvh_path_bounce b builds the list of the paths that go on FROM the list bounce b - 1 left behind, not
// from a scan over all pixels — after the first bounce most of a frame's paths are dead (870 k, 350 k, 150 k, 60 k live of 2 M).
static inline size_t ray_scratch_bytes_for(size_t count);
static inline uint32_t* ray_counter(lbvh_context* ctx, uint32_t turn) { return (uint32_t*)ctx->ray_scratch + 16u * turn; }
static inline uint32_t* ray_list(lbvh_context* ctx, size_t count, uint32_t turn) { return (uint32_t*)((char*)ctx->ray_scratch + 256 + turn * list_bytes(count)); }
static inline uint32_t* deep_stacks(lbvh_context* ctx, size_t count) { return (uint32_t*)((char*)ctx->ray_scratch + 256 + 2 * list_bytes(count)); }
static inline size_t ray_scratch_bytes_for(size_t count) { return 256 + 2 * list_bytes(count) + deep_bytes(count); }

// ---- the per-ray walk over four-wide nodes -------------------------------------------------------------------
// The per-ray kernel's time follows the number of steps its lanes take (profiles/r3: requests, bytes and L1 traffic per
// step could be halved without moving it), so the derived scene gets a second, shallower form for rays that do not
// come in packets: every binary node with its larger children opened once or twice = up to four child boxes in one
// 128-byte line.  Same leaves, same boxes, same triangle lines: which triangles a ray can meet does not change, and
// with ties going to the lower triangle index neither does the record it ends with.
struct alignas(128) lbvh_wide_node {
    float lo[3][4];          // [axis][slot]
    float hi[3][4];
    uint32_t ref[4];         // node index | LEAF + triangle line | kWideEmpty
    uint32_t pad[4];
};
static_assert(sizeof(lbvh_wide_node) == 128, "wide node must be one 128-byte line");
constexpr uint32_t kWideEmpty = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t pick4(const uint4 v, uint32_t k) { return k == 0u ? v.x : (k == 1u ? v.y : (k == 2u ? v.z : v.w)); }

// RayBoxIntersection (Raytracing.compute:75-87) on one slot of a wide node: the same six products, minima and maxima
__device__ __forceinline__ bool wide_box(float lx, float ly, float lz, float hx, float hy, float hz, const ray_t& r, float& tmin_out)
{
    return ray_box(make_float4(lx, ly, lz, 0.0f), make_float4(hx, hy, hz, 0.0f), r, tmin_out);
}

// what a launch of the per-ray walk did (lbvh_ray_stats_target: the algorithmic bytes of cfg5's roofline): wave reduction,
// one atomic per counter per wave at the end of the kernel
__device__ __forceinline__ void add_ray_stats(lbvh_ray_stats* stats, uint32_t rays, uint32_t steps, uint32_t tris)
{
    uint32_t v[3] = {rays, steps, tris};
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = wave_total_from_inclusive(wave_inclusive_sum(v[k]));
    if (lane_id() == 0) {
        atomicAdd((unsigned long long*)&stats->rays, (unsigned long long)v[0]);
        atomicAdd((unsigned long long*)&stats->node_fetches, (unsigned long long)v[1]);
        atomicAdd((unsigned long long*)&stats->triangle_tests, (unsigned long long)v[2]);
    }
}

}  // namespace

// ---- host: what every launcher of a per-lane walk starts with ------------------------------------------------------
// what the launch of a per-lane walk takes from the context: filled by begin_walk, the last three by use_wide_nodes
struct walk_launch {
    uint32_t waves = 0;                     // the grid: one wave per workgroup, one deep stack slab per wave
    uint32_t* deep = nullptr;               // the deep stack slabs
    uint32_t lds = 0, deep_cap = 0;         // a lane's stack entries in LDS / in its wave's slab, as the four-wide walkers take them
    const lbvh_wide_node* wn = nullptr;
};

// use_wide_nodes, begin_walk and csr_offsets (below): one definition each in lbvh_walk.hip, beside the kernels they launch, which
// so exist once in the library; hidden: the library's dynamic symbols are include/'s and nothing else.
__attribute__((visibility("hidden"))) lbvh_status use_wide_nodes(lbvh_context* ctx, walk_launch* w);
__attribute__((visibility("hidden"))) lbvh_status begin_walk(lbvh_context* ctx, const lbvh_scene* h_scene, size_t count, const char* who,
                                                             bool wide, walk_launch* w, bool keep_list = false);

// LBVH_REQUIRE with the entry point's name (`who`, a variable of the caller) in front of the message, as the stale-scene message
// of begin_walk has it: the box casts and the region family
#define NAMED_REQUIRE(cond)                                                                                         \
    do {                                                                                                            \
        if (!(cond)) return (lbvh_status)lbvh_set_error(ctx, LBVH_ERR_INVALID_ARG, who, "invalid argument: " #cond); \
    } while (0)

// The one launch of a family that answers one record or flag per query, after the family's argument checks and begin_walk (`w`)
// and before its hipGetLastError: the four-wide walk `kernel<ANY, STATS>`, named by the family (lbvh_debug_ray_walker does not
// apply).  These walkers take the same arguments; ctx, count and ANY are the caller's.
#define PER_QUERY_WALK(kernel, d_queries, d_out)                                                                                   \
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (kernel<ANY, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_queries, (uint32_t)count, w.wn, \
                      ctx->fast_nodes, d_out, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats)

// The scan behind every CSR answer: the `slots` 32-bit counts a count walk left in slice 0 of the ray scratch (csr_counts) ->
// their slots + 1 exclusive 64-bit offsets in d_offsets_out, the grand total last.  The counts (4 bytes per slot) and the tile
// sums of the scan live where lbvh_trace_rays keeps its two live-ray lists: the ray scratch is sized for 8 bytes per slot there
// (begin_walk with the same `slots`), and the list is dropped anyway.  The tiles cover slots + 1 offsets, 8 bytes per tile sum:
// (slots / 1024 + 1) * 8 <= list_bytes(slots) = 4 * slots rounded up to 256, for every slots >= 1.  One tile needs no sums.
static inline uint32_t* csr_counts(lbvh_context* ctx, size_t slots) { return ray_list(ctx, slots, 0); }
__attribute__((visibility("hidden"))) void csr_offsets(lbvh_context* ctx, size_t slots, uint64_t* d_offsets_out);

// A CSR answer on the caller's buffers, after begin_walk: count_walk(counts) launches the family's walk in its counting form,
// the scan turns the counts into d_offsets, fill_walk() launches the filling form unless the call only counts.  All on the
// context's stream, no host wait.
template <class COUNT_WALK, class FILL_WALK>
static lbvh_status csr_query(lbvh_context* ctx, size_t count, uint64_t* d_offsets, uint64_t capacity, COUNT_WALK count_walk, FILL_WALK fill_walk)
{
    count_walk(csr_counts(ctx, count));
    csr_offsets(ctx, count, d_offsets);
    if (capacity != 0) fill_walk();
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}
