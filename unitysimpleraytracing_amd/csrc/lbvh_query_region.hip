// lbvh_query_region.hip — which triangles lie in a convex region of six planes (include/lbvh.h): one region per lane
// (lbvh_region_overlaps, lbvh_region_overlaps_any), few large regions spread over the device (lbvh_region_overlaps_large, with
// lbvh_debug_region_task_cap and lbvh_debug_region_task_cap_of), and the contour where a plane cuts the mesh (lbvh_plane_sections),
// which takes the large regions' task scheme, region_task_cap_of and region_offsets_kernel.  Each family's kernel, launcher and
// entry points together.  The walk's shared pieces: lbvh_walk.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "lbvh_walk.h"

namespace {

// ---- region queries: which triangles lie in a convex region of six planes (lbvh_region_overlaps, include/lbvh.h) ---------
// The frame of overlap_wide_kernel<BOX = true> with another slot test: a slot is entered iff for each of the six planes
// {nx, ny, nz, d} the box corner farthest along the normal is on the kept side, P = ((nx * X + ny * Y) + nz * Z) + d >= 0 with
// X = nx >= 0 ? hi.x : lo.x and so on (the conservative frustum test).  A leaf slot's box is the triangle's own, so a leaf slot
// that passes IS a TOUCHING candidate and, as for the box form, costs no triangle line: line - leaf_base is the original index.
// CONTAINED asks the same of the nearest corner (N, the other choice on every axis) at leaf slots only; N <= P, so the walk's
// pruning is the same for both modes (the argument is in the header).  Nothing shrinks: the first passing inner slot is entered,
// the others wait on the stack.  There is no inactive region: a NaN fails every comparison, so such a region leaves at the root.
// Registers: the 24 plane words stay in the lane; which corner feeds P is decided once per query (18 flags, far_x / far_y / far_z),
// not in every slot.  The sums cannot contract: the file is compiled with -ffp-contract=off.
// `contained` is a kernel argument, not a template parameter: one branch per leaf slot against twice the instantiations.
enum region_mode : int { kRegionCount = 0, kRegionFill = 1, kRegionAny = 2 };

__device__ __forceinline__ float pickf4(const float4 v, uint32_t k) { return k == 0u ? v.x : (k == 1u ? v.y : (k == 2u ? v.z : v.w)); }

__device__ __forceinline__ float plane_value(float nx, float ny, float nz, float d, float x, float y, float z)
{
    return ((nx * x + ny * y) + nz * z) + d;
}

template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void region_wide_kernel(const float4* __restrict__ regions, uint32_t total,      // six float4 per region
                                                         uint32_t contained,                       // LBVH_REGION_CONTAINED != 0
                                                         const lbvh_wide_node* __restrict__ wide, uint32_t leaf_base,
                                                         uint32_t* __restrict__ counts,            // kRegionCount: candidates of region k; kRegionAny: the flags
                                                         const uint64_t* __restrict__ offsets,     // kRegionFill: where segment k starts
                                                         uint32_t* __restrict__ tris, uint64_t capacity,
                                                         uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                         uint32_t lds_depth,              // <= kWideStackLds
                                                         uint32_t deep_cap,               // <= kWideStackDeep
                                                         uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    float4 pl[LBVH_REGION_PLANES];                                   // the planes, in registers (every index below is a constant)
    bool far_x[LBVH_REGION_PLANES], far_y[LBVH_REGION_PLANES], far_z[LBVH_REGION_PLANES];      // n >= 0: hi feeds P (and lo feeds N)
#pragma unroll
    for (int j = 0; j < LBVH_REGION_PLANES; j++) {
        pl[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        far_x[j] = far_y[j] = far_z[j] = false;
    }
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // kRegionFill: where this lane's next candidate goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    auto emit = [&](uint32_t tri) {
        if constexpr (MODE == kRegionFill) {
            if (pos < capacity) tris[pos] = tri;         // never a word at or beyond the capacity
            pos++;
        } else {
            n_found++;
        }
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
#pragma unroll
                    for (int j = 0; j < LBVH_REGION_PLANES; j++) {
                        pl[j] = regions[LBVH_REGION_PLANES * (size_t)k + j];
                        far_x[j] = pl[j].x >= 0.0f; far_y[j] = pl[j].y >= 0.0f; far_z[j] = pl[j].z >= 0.0f;      // true for -0, false for NaN
                    }
                    active = true;
                    sp = 0; node = 0;
                    if constexpr (MODE == kRegionFill) pos = offsets[k];
                    else n_found = 0;
                    if (STATS) n_queries++;
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && next >= end) break;
        if (active) {
            if (STATS) n_steps++;
            const float4* w = reinterpret_cast<const float4*>(&wide[node]);
            const float4 lox = w[0], loy = w[1], loz = w[2], hix = w[3], hiy = w[4], hiz = w[5];
            const uint4 ref = reinterpret_cast<const uint4*>(w)[6];
            bool h0 = ref.x != kWideEmpty, h1 = ref.y != kWideEmpty, h2 = ref.z != kWideEmpty, h3 = ref.w != kWideEmpty;
#pragma unroll
            for (int j = 0; j < LBVH_REGION_PLANES; j++) {
                const float4 x = far_x[j] ? hix : lox, y = far_y[j] ? hiy : loy, z = far_z[j] ? hiz : loz;
                h0 &= plane_value(pl[j].x, pl[j].y, pl[j].z, pl[j].w, x.x, y.x, z.x) >= 0.0f;
                h1 &= plane_value(pl[j].x, pl[j].y, pl[j].z, pl[j].w, x.y, y.y, z.y) >= 0.0f;
                h2 &= plane_value(pl[j].x, pl[j].y, pl[j].z, pl[j].w, x.z, y.z, z.z) >= 0.0f;
                h3 &= plane_value(pl[j].x, pl[j].y, pl[j].z, pl[j].w, x.w, y.w, z.w) >= 0.0f;
            }
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                if (contained != 0u) {
                    const float lx = pickf4(lox, k), ly = pickf4(loy, k), lz = pickf4(loz, k);
                    const float hx = pickf4(hix, k), hy = pickf4(hiy, k), hz = pickf4(hiz, k);
                    bool inside = true;
#pragma unroll
                    for (int j = 0; j < LBVH_REGION_PLANES; j++)
                        inside &= plane_value(pl[j].x, pl[j].y, pl[j].z, pl[j].w, far_x[j] ? lx : hx, far_y[j] ? ly : hy,
                                                       far_z[j] ? lz : hz) >= 0.0f;
                    if (!inside) continue;
                }
                emit((pick4(ref, k) & 0x7FFFFFFFu) - leaf_base);
                if constexpr (MODE == kRegionAny) { leaves = 0u; inner = 0u; sp = 0; }         // the first candidate ends the walk
            }
            if (inner != 0u) {
                node = pick4(ref, (uint32_t)__builtin_ctz(inner));
                inner &= inner - 1u;
                while (inner != 0u) {
                    push(pick4(ref, (uint32_t)__builtin_ctz(inner)));
                    inner &= inner - 1u;
                }
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                if constexpr (MODE != kRegionFill) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

}  // namespace

// lbvh_region_overlaps: a CSR answer; lbvh_region_overlaps_any: one launch, the flags are the walk's own output.  Four-wide walk only.
// (a rejection names the entry point, as the stale-scene message of begin_walk does)
template <bool ANY>
static lbvh_status region_queries(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity, uint32_t* d_flags, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_regions != nullptr && h_scene != nullptr && (ANY ? d_flags != nullptr : d_offsets != nullptr));
    NAMED_REQUIRE(mode <= LBVH_REGION_CONTAINED);
    NAMED_REQUIRE(d_tris != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_regions & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0 && ((uintptr_t)d_flags & 3) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const float4* q = (const float4*)d_regions;
    const uint32_t total = (uint32_t)count, leaf_base = ctx->fast_capacity;
    if constexpr (ANY) {
        LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_wide_kernel<kRegionAny, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, mode, w.wn, leaf_base,
                          d_flags, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        LBVH_HIP_TRY(ctx, hipGetLastError());
        return LBVH_OK;
    } else {
        return csr_query(
            ctx, count, d_offsets, capacity,
            [&](uint32_t* counts) {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_wide_kernel<kRegionCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, mode, w.wn, leaf_base,
                                  counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
            },
            [&] {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_wide_kernel<kRegionFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, mode, w.wn, leaf_base,
                                  (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_tris, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
            });
    }
}

extern "C" {

lbvh_status lbvh_region_overlaps(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                 uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return region_queries<false>(ctx, d_regions, count, mode, h_scene, d_offsets, d_tris, capacity, nullptr, "lbvh_region_overlaps");
}

lbvh_status lbvh_region_overlaps_any(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                     uint32_t* d_flags)
{
    return region_queries<true>(ctx, d_regions, count, mode, h_scene, nullptr, nullptr, 0, d_flags, "lbvh_region_overlaps_any");
}

}  // extern "C"

namespace {

// ---- few large regions, each spread over the device (lbvh_region_overlaps_large, include/lbvh.h) --------------------------
// A region's candidates are the union of the candidates below any frontier cut of the four-wide tree that the slot test reached
// (the header's monotonicity argument), so a region is cut into up to task_cap subtree TASKS and every task gets a lane:
// region_expand_kernel makes the frontier, region_task_wide_kernel — region_wide_kernel's frame over task slots — walks it, and
// the scan kernels of the overlap queries run over the per-task counts.  Region q owns slots [q * task_cap, (q + 1) * task_cap).
// The slot test below is region_wide_kernel's, expression for expression; that kernel keeps its own copy, its instruction stream
// is pinned (tools/isa_resources.py --compare).
constexpr uint32_t kRegionTaskCapMax = 65536u;        // tasks per region at most ...
constexpr uint32_t kRegionTaskSlots = 1u << 22;       // ... and task slots per call (DESIGN.md §30 has the measurement)

struct region_planes {
    float4 pl[LBVH_REGION_PLANES];
    bool far_x[LBVH_REGION_PLANES], far_y[LBVH_REGION_PLANES], far_z[LBVH_REGION_PLANES];      // n >= 0: hi feeds P (and lo feeds N)
};

__device__ __forceinline__ void load_region_planes(region_planes& r, const float4* __restrict__ regions, size_t q)
{
#pragma unroll
    for (int j = 0; j < LBVH_REGION_PLANES; j++) {
        r.pl[j] = regions[LBVH_REGION_PLANES * q + j];
        r.far_x[j] = r.pl[j].x >= 0.0f; r.far_y[j] = r.pl[j].y >= 0.0f; r.far_z[j] = r.pl[j].z >= 0.0f;      // true for -0, false for NaN
    }
}

// the slots of one wide node that pass the TOUCHING test (bit k: slot k)
__device__ __forceinline__ uint32_t region_slots_touching(const region_planes& r, const float4 lox, const float4 loy, const float4 loz,
                                                          const float4 hix, const float4 hiy, const float4 hiz, const uint4 ref)
{
    bool h0 = ref.x != kWideEmpty, h1 = ref.y != kWideEmpty, h2 = ref.z != kWideEmpty, h3 = ref.w != kWideEmpty;
#pragma unroll
    for (int j = 0; j < LBVH_REGION_PLANES; j++) {
        const float4 x = r.far_x[j] ? hix : lox, y = r.far_y[j] ? hiy : loy, z = r.far_z[j] ? hiz : loz;
        h0 &= plane_value(r.pl[j].x, r.pl[j].y, r.pl[j].z, r.pl[j].w, x.x, y.x, z.x) >= 0.0f;
        h1 &= plane_value(r.pl[j].x, r.pl[j].y, r.pl[j].z, r.pl[j].w, x.y, y.y, z.y) >= 0.0f;
        h2 &= plane_value(r.pl[j].x, r.pl[j].y, r.pl[j].z, r.pl[j].w, x.z, y.z, z.z) >= 0.0f;
        h3 &= plane_value(r.pl[j].x, r.pl[j].y, r.pl[j].z, r.pl[j].w, x.w, y.w, z.w) >= 0.0f;
    }
    return (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
}

// CONTAINED at leaf slot k: the nearest corner of every plane
__device__ __forceinline__ bool region_slot_contained(const region_planes& r, const float4 lox, const float4 loy, const float4 loz,
                                                      const float4 hix, const float4 hiy, const float4 hiz, uint32_t k)
{
    const float lx = pickf4(lox, k), ly = pickf4(loy, k), lz = pickf4(loz, k);
    const float hx = pickf4(hix, k), hy = pickf4(hiy, k), hz = pickf4(hiz, k);
    bool inside = true;
#pragma unroll
    for (int j = 0; j < LBVH_REGION_PLANES; j++)
        inside &= plane_value(r.pl[j].x, r.pl[j].y, r.pl[j].z, r.pl[j].w, r.far_x[j] ? lx : hx, r.far_y[j] ? ly : hy,
                              r.far_z[j] ? lz : hz) >= 0.0f;
    return inside;
}

// One workgroup per region opens the tree breadth first.  The frontier starts as {root} (entered without a test, as the walk
// enters it) and ping-pongs between the region's slice of `tasks` and of `twin`.  A round: every inner entry is replaced by its
// slots that pass the TOUCHING test — leaf slots only if they are candidates of the mode —, leaf entries are carried over; the
// next frontier is compacted by a workgroup prefix sum in entry and slot order, so its bytes do not depend on timing.  A round
// starts only if len + 3 * n_inner <= task_cap (each inner entry can grow by three), so no slice can overflow; the expansion ends
// there or when only leaves are left.  At the end the slice of `tasks` holds the frontier, then kWideEmpty up to task_cap.
// A region with a NaN fails every slot of the root and leaves an all-empty slice.  __syncthreads() is the only synchronisation.
template <bool STATS>
__global__ __launch_bounds__(256) void region_expand_kernel(const float4* __restrict__ regions, uint32_t contained,
                                                            const lbvh_wide_node* __restrict__ wide, uint32_t task_cap,
                                                            uint32_t* tasks, uint32_t* twin, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t wave = threadIdx.x / LBVH_WAVE;
    uint32_t* const mine = tasks + (size_t)blockIdx.x * task_cap;
    uint32_t* cur = mine;
    uint32_t* nxt = twin + (size_t)blockIdx.x * task_cap;
    region_planes r;
    load_region_planes(r, regions, blockIdx.x);
    uint32_t len = 1, n_inner = 1, n_steps = 0;
    if (threadIdx.x == 0) cur[0] = 0u;
    __syncthreads();
    while (n_inner != 0u && len + 3u * n_inner <= task_cap) {
        uint32_t out_len = 0, out_inner = 0;
        for (uint32_t base = 0; base < len; base += 256u) {
            const uint32_t i = base + threadIdx.x;
            uint32_t entry = kWideEmpty, keep = 0u, n_out = 0u, inner_out = 0u;
            uint4 ref = make_uint4(kWideEmpty, kWideEmpty, kWideEmpty, kWideEmpty);
            if (i < len) {
                entry = cur[i];
                if (entry & 0x80000000u) {
                    n_out = 1u;
                } else {
                    if (STATS) n_steps++;
                    const float4* w = reinterpret_cast<const float4*>(&wide[entry]);
                    const float4 lox = w[0], loy = w[1], loz = w[2], hix = w[3], hiy = w[4], hiz = w[5];
                    ref = reinterpret_cast<const uint4*>(w)[6];
                    const uint32_t hit = region_slots_touching(r, lox, loy, loz, hix, hiy, hiz, ref);
                    const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
                    uint32_t leaves = hit & leaf;
                    const uint32_t inner = hit & ~leaf;
                    keep = inner;
                    while (leaves != 0u) {
                        const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                        leaves &= leaves - 1u;
                        if (contained == 0u || region_slot_contained(r, lox, loy, loz, hix, hiy, hiz, k)) keep |= 1u << k;
                    }
                    n_out = (uint32_t)__popc(keep);
                    inner_out = (uint32_t)__popc(inner);
                }
            }
            // both counts in one scan: at most 4 x 256 each per chunk
            const uint32_t v = n_out | (inner_out << 16);
            const uint32_t incl = wave_inclusive_sum(v);
            if (lane_id() == LBVH_WAVE - 1) s_wave[wave] = incl;
            __syncthreads();
            const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
            __syncthreads();                                             // s_wave is written again in the next chunk
            uint32_t at = out_len + (((incl - v) + (wave > 0u ? w0 : 0u) + (wave > 1u ? w1 : 0u) + (wave > 2u ? w2 : 0u)) & 0xFFFFu);
            if (entry & 0x80000000u) {
                if (i < len) nxt[at] = entry;                            // (entry == kWideEmpty: a lane beyond the frontier)
            } else {
                while (keep != 0u) {
                    nxt[at++] = pick4(ref, (uint32_t)__builtin_ctz(keep));
                    keep &= keep - 1u;
                }
            }
            const uint32_t all = ((w0 + w1) + (w2 + w3));
            out_len += all & 0xFFFFu;
            out_inner += all >> 16;
        }
        __syncthreads();                                                 // the next round reads what this one wrote
        uint32_t* const t = cur; cur = nxt; nxt = t;
        len = out_len; n_inner = out_inner;
    }
    if (cur != mine)
        for (uint32_t i = threadIdx.x; i < len; i += 256u) mine[i] = cur[i];
    for (uint32_t i = len + threadIdx.x; i < task_cap; i += 256u) mine[i] = kWideEmpty;
    if (STATS) add_ray_stats(stats, 0u, n_steps, 0u);
}

// The frame of region_wide_kernel over task slots instead of regions.  A refilled lane reads slot k: kWideEmpty is no task (its
// count is 0), a leaf reference is a candidate the expansion accepted already and is emitted without a test, anything else is
// the node a walk with the planes of region k / task_cap starts from.  Fill mode: `offsets` are the 64-bit task offsets.
template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void region_task_wide_kernel(const float4* __restrict__ regions, uint32_t total,      // task slots
                                                              uint32_t task_cap, const uint32_t* __restrict__ tasks,
                                                              uint32_t contained,                       // LBVH_REGION_CONTAINED != 0
                                                              const lbvh_wide_node* __restrict__ wide, uint32_t leaf_base,
                                                              uint32_t* __restrict__ counts,            // kRegionCount: candidates of task k
                                                              const uint64_t* __restrict__ offsets,     // kRegionFill: where task k's candidates start
                                                              uint32_t* __restrict__ tris, uint64_t capacity,
                                                              uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                              uint32_t lds_depth,              // <= kWideStackLds
                                                              uint32_t deep_cap,               // <= kWideStackDeep
                                                              uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    static_assert(MODE == kRegionCount || MODE == kRegionFill, "the large form has no any mode");
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    region_planes r;                                                 // the planes, in registers (every index below is a constant)
#pragma unroll
    for (int j = 0; j < LBVH_REGION_PLANES; j++) {
        r.pl[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        r.far_x[j] = r.far_y[j] = r.far_z[j] = false;
    }
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // kRegionFill: where this lane's next candidate goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    auto emit = [&](uint32_t tri) {
        if constexpr (MODE == kRegionFill) {
            if (pos < capacity) tris[pos] = tri;         // never a word at or beyond the capacity
            pos++;
        } else {
            n_found++;
        }
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    const uint32_t task = tasks[k];
                    if (task == kWideEmpty) {
                        if constexpr (MODE == kRegionCount) counts[k] = 0u;
                    } else if (task & 0x80000000u) {
                        if (STATS) { n_queries++; n_tris++; }
                        if constexpr (MODE == kRegionFill) {
                            const uint64_t at = offsets[k];
                            if (at < capacity) tris[at] = (task & 0x7FFFFFFFu) - leaf_base;
                        } else {
                            counts[k] = 1u;
                        }
                    } else {
                        i = k;
                        load_region_planes(r, regions, k / task_cap);
                        active = true;
                        sp = 0; node = task;
                        if constexpr (MODE == kRegionFill) pos = offsets[k];
                        else n_found = 0;
                        if (STATS) n_queries++;
                    }
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && next >= end) break;
        if (active) {
            if (STATS) n_steps++;
            const float4* w = reinterpret_cast<const float4*>(&wide[node]);
            const float4 lox = w[0], loy = w[1], loz = w[2], hix = w[3], hiy = w[4], hiz = w[5];
            const uint4 ref = reinterpret_cast<const uint4*>(w)[6];
            const uint32_t hit = region_slots_touching(r, lox, loy, loz, hix, hiy, hiz, ref);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                if (contained != 0u && !region_slot_contained(r, lox, loy, loz, hix, hiy, hiz, k)) continue;
                emit((pick4(ref, k) & 0x7FFFFFFFu) - leaf_base);
            }
            if (inner != 0u) {
                node = pick4(ref, (uint32_t)__builtin_ctz(inner));
                inner &= inner - 1u;
                while (inner != 0u) {
                    push(pick4(ref, (uint32_t)__builtin_ctz(inner)));
                    inner &= inner - 1u;
                }
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                if constexpr (MODE == kRegionCount) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// d_offsets of the large form: every region's first task offset, and the grand total behind the last slot
__global__ __launch_bounds__(256) void region_offsets_kernel(const uint64_t* __restrict__ task_offsets, uint32_t task_cap, uint32_t count,
                                                             uint64_t* __restrict__ offsets)            // count + 1 words
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q <= count) offsets[q] = task_offsets[(size_t)q * task_cap];
}

}  // namespace

// tasks per region of lbvh_region_overlaps_large: the largest power of two not above min(kRegionTaskCapMax, kRegionTaskSlots / count),
// or what lbvh_debug_region_task_cap asked for, within the same slot budget
static uint32_t region_task_cap_of(uint32_t forced, size_t count)
{
    if (count == 0 || count > LBVH_REGION_LARGE_MAX_COUNT) return 0u;
    const uint32_t budget = kRegionTaskSlots / (uint32_t)count;       // >= 64
    if (forced != 0u) return std::min(forced, budget);
    uint32_t cap = kRegionTaskCapMax;
    while (cap > budget) cap >>= 1;
    return cap;
}

// lbvh_region_overlaps_large: region_queries<false>'s shape over count * task_cap task slots — expansion -> task count walk -> the
// scan over the per-task counts into the task offsets -> d_offsets picked from them -> task fill walk.  The ray scratch is sized
// for the slots; the task array, its twin and the slots + 1 task offsets live in a context buffer of their own.
static lbvh_status region_queries_large(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                        uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_regions != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(mode <= LBVH_REGION_CONTAINED);
    NAMED_REQUIRE(d_tris != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_regions & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0);
    NAMED_REQUIRE(count <= LBVH_REGION_LARGE_MAX_COUNT);
    const uint32_t task_cap = region_task_cap_of(ctx->region_task_cap, count);
    const size_t slots = count * (size_t)task_cap;                    // <= kRegionTaskSlots
    walk_launch w;
    lbvh_status rc = begin_walk(ctx, h_scene, slots, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const size_t slice = list_bytes(slots);
    rc = (lbvh_status)lbvh_reserve(ctx, &ctx->region_tasks, &ctx->region_tasks_bytes, 2 * slice + (slots + 1) * sizeof(uint64_t));
    if (rc != LBVH_OK) return rc;
    uint32_t* tasks = (uint32_t*)ctx->region_tasks;
    uint32_t* twin = (uint32_t*)((char*)ctx->region_tasks + slice);
    uint64_t* task_offsets = (uint64_t*)((char*)ctx->region_tasks + 2 * slice);
    const float4* q = (const float4*)d_regions;
    const uint32_t total = (uint32_t)slots, leaf_base = ctx->fast_capacity;
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_expand_kernel<STATS>), dim3((uint32_t)count), dim3(256), q, mode, w.wn, task_cap, tasks, twin,
                      ctx->ray_stats);
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_task_wide_kernel<kRegionCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, task_cap,
                      (const uint32_t*)tasks, mode, w.wn, leaf_base, csr_counts(ctx, slots), (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0,
                      w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    csr_offsets(ctx, slots, task_offsets);
    LBVH_LAUNCH(ctx, region_offsets_kernel, dim3((uint32_t)(count / 256 + 1)), dim3(256), (const uint64_t*)task_offsets, task_cap, (uint32_t)count,
                d_offsets);
    if (capacity != 0)
        LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (region_task_wide_kernel<kRegionFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, task_cap,
                          (const uint32_t*)tasks, mode, w.wn, leaf_base, (uint32_t*)nullptr, (const uint64_t*)task_offsets, d_tris, capacity, w.deep,
                          w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

extern "C" {

lbvh_status lbvh_region_overlaps_large(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                       uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return region_queries_large(ctx, d_regions, count, mode, h_scene, d_offsets, d_tris, capacity, "lbvh_region_overlaps_large");
}

lbvh_status lbvh_debug_region_task_cap(lbvh_context* ctx, uint32_t cap)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, cap == 0u || (cap >= 4u && cap <= kRegionTaskCapMax));
    ctx->region_task_cap = cap;
    return LBVH_OK;
}

uint32_t lbvh_debug_region_task_cap_of(uint32_t cap, size_t count) { return region_task_cap_of(cap, count); }

}  // extern "C"

namespace {

// ---- plane sections: the contour where a plane cuts the mesh (lbvh_plane_sections, include/lbvh.h) ------------------------
// The frame of lbvh_region_overlaps_large with a plane as the query: plane_expand_kernel cuts every plane's walk into up to
// task_cap subtree tasks, plane_task_wide_kernel walks them one per lane, the overlap queries' scan kernels run over the per-task
// counts and region_offsets_kernel picks d_offsets.  A slot is entered iff the plane cuts its box: P >= 0 && N <= 0, P and N the
// farthest and the nearest corner along n — region_wide_kernel's two corner values of ONE plane, so the plane is 4 VGPRs and three
// corner choices made once.  Unlike a region's, a passing leaf slot is no candidate yet: the triangle's line is read and the three
// vertices are put to the plane (rule 2 of the header), and the fill walk writes the 32-byte record as two 16-byte stores.  The
// expansion reads no triangle line: a leaf slot stays in the frontier iff its box passes, and the task walks decide.
// The region kernels above keep their own copies of the frame; their instruction streams are pinned.
enum plane_mode : int { kPlaneCount = 0, kPlaneFill = 1 };

struct section_plane {
    float4 pl;
    bool far_x, far_y, far_z;                  // n >= 0: hi feeds P (and lo feeds N)
};

__device__ __forceinline__ void load_section_plane(section_plane& s, const float4* __restrict__ planes, size_t q)
{
    s.pl = planes[q];
    s.far_x = s.pl.x >= 0.0f; s.far_y = s.pl.y >= 0.0f; s.far_z = s.pl.z >= 0.0f;      // true for -0, false for NaN
}

// the slots of one wide node whose box the plane cuts (bit k: slot k); a NaN fails both comparisons
__device__ __forceinline__ uint32_t plane_slots_cut(const section_plane& s, const float4 lox, const float4 loy, const float4 loz,
                                                    const float4 hix, const float4 hiy, const float4 hiz, const uint4 ref)
{
    const float4 px = s.far_x ? hix : lox, py = s.far_y ? hiy : loy, pz = s.far_z ? hiz : loz;
    const float4 nx = s.far_x ? lox : hix, ny = s.far_y ? loy : hiy, nz = s.far_z ? loz : hiz;
    const float4 p = s.pl;
    const bool h0 = ref.x != kWideEmpty && plane_value(p.x, p.y, p.z, p.w, px.x, py.x, pz.x) >= 0.0f &&
                    plane_value(p.x, p.y, p.z, p.w, nx.x, ny.x, nz.x) <= 0.0f;
    const bool h1 = ref.y != kWideEmpty && plane_value(p.x, p.y, p.z, p.w, px.y, py.y, pz.y) >= 0.0f &&
                    plane_value(p.x, p.y, p.z, p.w, nx.y, ny.y, nz.y) <= 0.0f;
    const bool h2 = ref.z != kWideEmpty && plane_value(p.x, p.y, p.z, p.w, px.z, py.z, pz.z) >= 0.0f &&
                    plane_value(p.x, p.y, p.z, p.w, nx.z, ny.z, nz.z) <= 0.0f;
    const bool h3 = ref.w != kWideEmpty && plane_value(p.x, p.y, p.z, p.w, px.w, py.w, pz.w) >= 0.0f &&
                    plane_value(p.x, p.y, p.z, p.w, nx.w, ny.w, nz.w) <= 0.0f;
    return (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
}

// the crossing of an edge from its end on the positive side (vp, value sp) to its other end (vm, value sm), per component:
// one subtraction, one multiplication, one addition — a function of the two ends only, whichever way the edge runs
__device__ __forceinline__ float crossing_of(float vp, float vm, float t) { return vp + (vm - vp) * t; }

// Rule 2 and the record of the header for the triangle line (t0 = {a, original index}, t1 = e1, t2 = e2): false iff the three
// vertices lie on one side.  RECORD = false only decides (the count walk); both forms take the decision from the same three values.
template <bool RECORD>
__device__ __forceinline__ bool plane_section_of(const float4 p, const float4 t0, const float4 t1, const float4 t2, float4& rec0, float4& rec1)
{
    const float v1x = t0.x + t1.x, v1y = t0.y + t1.y, v1z = t0.z + t1.z;
    const float v2x = t0.x + t2.x, v2y = t0.y + t2.y, v2z = t0.z + t2.z;
    const float s0 = plane_value(p.x, p.y, p.z, p.w, t0.x, t0.y, t0.z);
    const float s1 = plane_value(p.x, p.y, p.z, p.w, v1x, v1y, v1z);
    const float s2 = plane_value(p.x, p.y, p.z, p.w, v2x, v2y, v2z);
    const bool b0 = s0 >= 0.0f, b1 = s1 >= 0.0f, b2 = s2 >= 0.0f;                       // true for -0, false for NaN
    if (b0 == b1 && b1 == b2) return false;
    if constexpr (RECORD) {
        // of E0 = V0 -> V1, E1 = V1 -> V2, E2 = V2 -> V0 one runs from the positive side to the other (it gives p0) and one back (p1)
        const uint32_t down = (b0 && !b1) ? 0u : ((b1 && !b2) ? 1u : 2u);
        const uint32_t up = (!b0 && b1) ? 0u : ((!b1 && b2) ? 1u : 2u);
        // the positive end of `down` is its start V_down, of `up` its end V_(up + 1); the other end is the next / the previous vertex
        const float dpx = down == 0u ? t0.x : (down == 1u ? v1x : v2x), dmx = down == 0u ? v1x : (down == 1u ? v2x : t0.x);
        const float dpy = down == 0u ? t0.y : (down == 1u ? v1y : v2y), dmy = down == 0u ? v1y : (down == 1u ? v2y : t0.y);
        const float dpz = down == 0u ? t0.z : (down == 1u ? v1z : v2z), dmz = down == 0u ? v1z : (down == 1u ? v2z : t0.z);
        const float dsp = down == 0u ? s0 : (down == 1u ? s1 : s2), dsm = down == 0u ? s1 : (down == 1u ? s2 : s0);
        const float upx = up == 0u ? v1x : (up == 1u ? v2x : t0.x), umx = up == 0u ? t0.x : (up == 1u ? v1x : v2x);
        const float upy = up == 0u ? v1y : (up == 1u ? v2y : t0.y), umy = up == 0u ? t0.y : (up == 1u ? v1y : v2y);
        const float upz = up == 0u ? v1z : (up == 1u ? v2z : t0.z), umz = up == 0u ? t0.z : (up == 1u ? v1z : v2z);
        const float usp = up == 0u ? s1 : (up == 1u ? s2 : s0), usm = up == 0u ? s0 : (up == 1u ? s1 : s2);
        const float td = dsp / (dsp - dsm), tu = usp / (usp - usm);
        rec0 = make_float4(crossing_of(dpx, dmx, td), crossing_of(dpy, dmy, td), crossing_of(dpz, dmz, td), t0.w);      // .w: the ORIGINAL index
        const uint32_t edges = (1u << down) | (1u << up) | (down << 8) | (up << 12) | ((b0 ? 1u : 0u) << 16) | ((b1 ? 1u : 0u) << 17) |
                               ((b2 ? 1u : 0u) << 18);
        rec1 = make_float4(crossing_of(upx, umx, tu), crossing_of(upy, umy, tu), crossing_of(upz, umz, tu), __uint_as_float(edges));
    }
    return true;
}

// region_expand_kernel with the plane's slot test: one workgroup per plane opens the tree breadth first, the frontier ping-pongs
// between the plane's slices of `tasks` and `twin`, a round starts only if len + 3 * n_inner <= task_cap, the next frontier is
// compacted by a workgroup prefix sum in entry and slot order.  A leaf slot is kept iff its box passes; no triangle line is read.
// At the end the slice of `tasks` holds the frontier, then kWideEmpty up to task_cap.  A plane with a NaN fails every slot of the
// root and leaves an all-empty slice.  __syncthreads() is the only synchronisation.
template <bool STATS>
__global__ __launch_bounds__(256) void plane_expand_kernel(const float4* __restrict__ planes, const lbvh_wide_node* __restrict__ wide,
                                                           uint32_t task_cap, uint32_t* tasks, uint32_t* twin, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t wave = threadIdx.x / LBVH_WAVE;
    uint32_t* const mine = tasks + (size_t)blockIdx.x * task_cap;
    uint32_t* cur = mine;
    uint32_t* nxt = twin + (size_t)blockIdx.x * task_cap;
    section_plane s;
    load_section_plane(s, planes, blockIdx.x);
    uint32_t len = 1, n_inner = 1, n_steps = 0;
    if (threadIdx.x == 0) cur[0] = 0u;
    __syncthreads();
    while (n_inner != 0u && len + 3u * n_inner <= task_cap) {
        uint32_t out_len = 0, out_inner = 0;
        for (uint32_t base = 0; base < len; base += 256u) {
            const uint32_t i = base + threadIdx.x;
            uint32_t entry = kWideEmpty, keep = 0u, n_out = 0u, inner_out = 0u;
            uint4 ref = make_uint4(kWideEmpty, kWideEmpty, kWideEmpty, kWideEmpty);
            if (i < len) {
                entry = cur[i];
                if (entry & 0x80000000u) {
                    n_out = 1u;
                } else {
                    if (STATS) n_steps++;
                    const float4* w = reinterpret_cast<const float4*>(&wide[entry]);
                    const float4 lox = w[0], loy = w[1], loz = w[2], hix = w[3], hiy = w[4], hiz = w[5];
                    ref = reinterpret_cast<const uint4*>(w)[6];
                    keep = plane_slots_cut(s, lox, loy, loz, hix, hiy, hiz, ref);
                    const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
                    n_out = (uint32_t)__popc(keep);
                    inner_out = (uint32_t)__popc(keep & ~leaf);
                }
            }
            // both counts in one scan: at most 4 x 256 each per chunk
            const uint32_t v = n_out | (inner_out << 16);
            const uint32_t incl = wave_inclusive_sum(v);
            if (lane_id() == LBVH_WAVE - 1) s_wave[wave] = incl;
            __syncthreads();
            const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
            __syncthreads();                                             // s_wave is written again in the next chunk
            uint32_t at = out_len + (((incl - v) + (wave > 0u ? w0 : 0u) + (wave > 1u ? w1 : 0u) + (wave > 2u ? w2 : 0u)) & 0xFFFFu);
            if (entry & 0x80000000u) {
                if (i < len) nxt[at] = entry;                            // (entry == kWideEmpty: a lane beyond the frontier)
            } else {
                while (keep != 0u) {
                    nxt[at++] = pick4(ref, (uint32_t)__builtin_ctz(keep));
                    keep &= keep - 1u;
                }
            }
            const uint32_t all = ((w0 + w1) + (w2 + w3));
            out_len += all & 0xFFFFu;
            out_inner += all >> 16;
        }
        __syncthreads();                                                 // the next round reads what this one wrote
        uint32_t* const t = cur; cur = nxt; nxt = t;
        len = out_len; n_inner = out_inner;
    }
    if (cur != mine)
        for (uint32_t i = threadIdx.x; i < len; i += 256u) mine[i] = cur[i];
    for (uint32_t i = len + threadIdx.x; i < task_cap; i += 256u) mine[i] = kWideEmpty;
    if (STATS) add_ray_stats(stats, 0u, n_steps, 0u);
}

// The frame of region_task_wide_kernel.  A refilled lane reads slot k: kWideEmpty is no task (its count is 0); a leaf reference is
// a triangle whose box the expansion passed — its line is read and rule 2 decides here, it is no candidate yet —; anything else is
// the node a walk with plane k / task_cap starts from.  Fill mode: `offsets` are the 64-bit task offsets, and a record is two
// 16-byte stores at the task's own position, never at or beyond `capacity`.
template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void plane_task_wide_kernel(const float4* __restrict__ planes, uint32_t total,      // task slots
                                                             uint32_t task_cap, const uint32_t* __restrict__ tasks,
                                                             const lbvh_wide_node* __restrict__ wide,
                                                             const lbvh_fast_node* __restrict__ lines,
                                                             uint32_t* __restrict__ counts,            // kPlaneCount: candidates of task k
                                                             const uint64_t* __restrict__ offsets,     // kPlaneFill: where task k's records start
                                                             float4* __restrict__ records, uint64_t capacity,
                                                             uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                             uint32_t lds_depth,              // <= kWideStackLds
                                                             uint32_t deep_cap,               // <= kWideStackDeep
                                                             uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    static_assert(MODE == kPlaneCount || MODE == kPlaneFill, "count or fill");
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    section_plane s;                                                 // the plane, in registers
    s.pl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s.far_x = s.far_y = s.far_z = false;
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // kPlaneFill: where this lane's next record goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    // the triangle line `line` put to the plane: counted, or its record written at `at` (never at or beyond the capacity)
    auto test = [&](uint32_t line, uint64_t& at, uint32_t& found) {
        float4 t0, t1, t2, rec0, rec1;
        unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
        if (STATS) n_tris++;
        if (!plane_section_of<MODE == kPlaneFill>(s.pl, t0, t1, t2, rec0, rec1)) return;
        if constexpr (MODE == kPlaneFill) {
            if (at < capacity) { records[2 * at] = rec0; records[2 * at + 1] = rec1; }
            at++;
        } else {
            found++;
        }
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    const uint32_t task = tasks[k];
                    if (task == kWideEmpty) {
                        if constexpr (MODE == kPlaneCount) counts[k] = 0u;
                    } else if (task & 0x80000000u) {
                        if (STATS) n_queries++;
                        load_section_plane(s, planes, k / task_cap);
                        uint64_t at = 0;
                        uint32_t found = 0u;
                        if constexpr (MODE == kPlaneFill) at = offsets[k];
                        test(task & 0x7FFFFFFFu, at, found);
                        if constexpr (MODE == kPlaneCount) counts[k] = found;
                    } else {
                        i = k;
                        load_section_plane(s, planes, k / task_cap);
                        active = true;
                        sp = 0; node = task;
                        if constexpr (MODE == kPlaneFill) pos = offsets[k];
                        else n_found = 0;
                        if (STATS) n_queries++;
                    }
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && next >= end) break;
        if (active) {
            if (STATS) n_steps++;
            const float4* w = reinterpret_cast<const float4*>(&wide[node]);
            const float4 lox = w[0], loy = w[1], loz = w[2], hix = w[3], hiy = w[4], hiz = w[5];
            const uint4 ref = reinterpret_cast<const uint4*>(w)[6];
            const uint32_t hit = plane_slots_cut(s, lox, loy, loz, hix, hiy, hiz, ref);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                test(pick4(ref, k) & 0x7FFFFFFFu, pos, n_found);
            }
            if (inner != 0u) {
                node = pick4(ref, (uint32_t)__builtin_ctz(inner));
                inner &= inner - 1u;
                while (inner != 0u) {
                    push(pick4(ref, (uint32_t)__builtin_ctz(inner)));
                    inner &= inner - 1u;
                }
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                if constexpr (MODE == kPlaneCount) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

}  // namespace

// lbvh_plane_sections: region_queries_large's shape with a plane as the query and a 32-byte record as the answer — expansion ->
// task count walk -> the scan over the per-task counts -> d_offsets picked from the task offsets -> task fill walk.  The same
// task-cap rule (lbvh_debug_region_task_cap applies) and the same context scratch.
static lbvh_status plane_sections(lbvh_context* ctx, const lbvh_plane* d_planes, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                  lbvh_plane_segment* d_segments, uint64_t capacity, const char* who)
{
    static_assert(sizeof(lbvh_plane) == sizeof(float4) && sizeof(lbvh_plane_segment) == 2 * sizeof(float4), "one and two float4");
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_planes != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_segments != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_planes & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_segments & 15) == 0);
    NAMED_REQUIRE(count <= LBVH_PLANE_SECTIONS_MAX_COUNT);
    const uint32_t task_cap = region_task_cap_of(ctx->region_task_cap, count);
    const size_t slots = count * (size_t)task_cap;                    // <= kRegionTaskSlots
    walk_launch w;
    lbvh_status rc = begin_walk(ctx, h_scene, slots, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const size_t slice = list_bytes(slots);
    rc = (lbvh_status)lbvh_reserve(ctx, &ctx->region_tasks, &ctx->region_tasks_bytes, 2 * slice + (slots + 1) * sizeof(uint64_t));
    if (rc != LBVH_OK) return rc;
    uint32_t* tasks = (uint32_t*)ctx->region_tasks;
    uint32_t* twin = (uint32_t*)((char*)ctx->region_tasks + slice);
    uint64_t* task_offsets = (uint64_t*)((char*)ctx->region_tasks + 2 * slice);
    const float4* q = (const float4*)d_planes;
    const uint32_t total = (uint32_t)slots;
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (plane_expand_kernel<STATS>), dim3((uint32_t)count), dim3(256), q, w.wn, task_cap, tasks, twin,
                      ctx->ray_stats);
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (plane_task_wide_kernel<kPlaneCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, task_cap,
                      (const uint32_t*)tasks, w.wn, ctx->fast_nodes, csr_counts(ctx, slots), (const uint64_t*)nullptr, (float4*)nullptr, (uint64_t)0,
                      w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    csr_offsets(ctx, slots, task_offsets);
    LBVH_LAUNCH(ctx, region_offsets_kernel, dim3((uint32_t)(count / 256 + 1)), dim3(256), (const uint64_t*)task_offsets, task_cap, (uint32_t)count,
                d_offsets);
    if (capacity != 0)
        LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (plane_task_wide_kernel<kPlaneFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, task_cap,
                          (const uint32_t*)tasks, w.wn, ctx->fast_nodes, (uint32_t*)nullptr, (const uint64_t*)task_offsets, (float4*)d_segments,
                          capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

extern "C" {

lbvh_status lbvh_plane_sections(lbvh_context* ctx, const lbvh_plane* d_planes, size_t count, const lbvh_scene* h_scene,
                                uint64_t* d_offsets, lbvh_plane_segment* d_segments, uint64_t capacity)
{
    return plane_sections(ctx, d_planes, count, h_scene, d_offsets, d_segments, capacity, "lbvh_plane_sections");
}

}  // extern "C"
