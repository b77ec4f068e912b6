// lbvh_walk.hip — the launches every per-lane walker shares (lbvh_walk.h): the four-wide form of the derived tree, the prologue of
// every entry point that walks it, the scan behind every CSR answer, and the test hooks of the walk.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "lbvh_walk.h"

namespace {

struct wide_slot { float mn[3], mx[3]; uint32_t ref; };

__device__ __forceinline__ float half_area(const wide_slot& b)
{
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    return dx * dy + dy * dz + dz * dx;
}

__device__ __forceinline__ void children_of(const lbvh_fast_node* __restrict__ nodes, uint32_t i, wide_slot& l, wide_slot& r)
{
    const float4* q = reinterpret_cast<const float4*>(&nodes[i]);
    const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    l.mn[0] = q0.x; l.mn[1] = q0.y; l.mn[2] = q0.z; l.mx[0] = q1.x; l.mx[1] = q1.y; l.mx[2] = q1.z; l.ref = __float_as_uint(q0.w);
    r.mn[0] = q2.x; r.mn[1] = q2.y; r.mn[2] = q2.z; r.mx[0] = q3.x; r.mx[1] = q3.y; r.mx[2] = q3.z; r.ref = __float_as_uint(q1.w);
}

// one thread per binary node: its two children, then twice the internal child with the largest surface opened
__global__ __launch_bounds__(256) void collapse_wide_kernel(const lbvh_fast_node* __restrict__ nodes, uint32_t n_internal,
                                                            lbvh_wide_node* __restrict__ wide)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_internal) return;
    wide_slot s[4];
    children_of(nodes, i, s[0], s[1]);
    s[2].ref = kWideEmpty; s[3].ref = kWideEmpty;
#pragma unroll
    for (int k = 2; k < 4; k++)
#pragma unroll
        for (int a = 0; a < 3; a++) { s[k].mn[a] = 0.0f; s[k].mx[a] = 0.0f; }
#pragma unroll
    for (int round = 0; round < 2; round++) {
        int open = -1;
        float open_area = -1.0f;
#pragma unroll
        for (int k = 0; k < 2 + round; k++) {
            const float a = half_area(s[k]);
            if (!(s[k].ref & 0x80000000u) && (open < 0 || a > open_area)) { open = k; open_area = a; }
        }
        if (open < 0) break;
        uint32_t parent = 0;
#pragma unroll
        for (int k = 0; k < 2 + round; k++)
            if (k == open) parent = s[k].ref;
        wide_slot l, r;
        children_of(nodes, parent, l, r);
#pragma unroll
        for (int k = 0; k < 2 + round; k++)
            if (k == open) s[k] = l;
        s[2 + round] = r;
    }
    lbvh_wide_node out;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int a = 0; a < 3; a++) { out.lo[a][k] = s[k].mn[a]; out.hi[a][k] = s[k].mx[a]; }
        out.ref[k] = s[k].ref;
        out.pad[k] = 0u;
    }
    float4* dst = reinterpret_cast<float4*>(&wide[i]);
    const float4* src = reinterpret_cast<const float4*>(&out);
#pragma unroll
    for (int k = 0; k < 8; k++) dst[k] = src[k];
}

// The scan of the counts into the 64-bit offsets: tiles of 1024 counts (256 threads x one 16-byte load), (1) a sum per tile,
// (2) one workgroup scans the tile sums in place, (3) every tile scans its own counts on top of its prefix and writes
// offsets[first .. first + 1024) — offsets[total] = the grand total included, so the tiles cover total + 1 outputs.
constexpr uint32_t kScanTile = 1024;

__device__ __forceinline__ uint64_t wave_inclusive_sum_u64(uint64_t v)
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (int d = 1; d < LBVH_WAVE; d <<= 1) {
        const uint64_t o = __shfl_up(v, d, LBVH_WAVE);
        if (lane >= (uint32_t)d) v += o;
    }
    return v;
}

// the four counts of a thread of a tile; counts at or beyond `total` read as 0
__device__ __forceinline__ uint4 load_tile_counts(const uint32_t* __restrict__ counts, uint64_t first, uint32_t total)
{
    uint4 c = make_uint4(0u, 0u, 0u, 0u);
    if (first + 3 < total) c = reinterpret_cast<const uint4*>(counts)[first >> 2];
    else {
        if (first < total) c.x = counts[first];
        if (first + 1 < total) c.y = counts[first + 1];
        if (first + 2 < total) c.z = counts[first + 2];
    }
    return c;
}

__global__ __launch_bounds__(256) void overlap_tile_sums_kernel(const uint32_t* __restrict__ counts, uint32_t total, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t s_wave[4];
    const uint4 c = load_tile_counts(counts, (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u, total);
    const uint64_t incl = wave_inclusive_sum_u64(((uint64_t)c.x + c.y) + ((uint64_t)c.z + c.w));
    if (lane_id() == LBVH_WAVE - 1) s_wave[threadIdx.x / LBVH_WAVE] = incl;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ __launch_bounds__(1024) void overlap_scan_sums_kernel(uint64_t* __restrict__ sums, uint32_t n_tiles)
{
    __shared__ uint64_t s_wave[16];
    const uint32_t wave = threadIdx.x / LBVH_WAVE;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += 1024u) {
        const uint32_t t = base + threadIdx.x;
        const uint64_t v = t < n_tiles ? sums[t] : 0;
        const uint64_t incl = wave_inclusive_sum_u64(v);
        if (lane_id() == LBVH_WAVE - 1) s_wave[wave] = incl;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint64_t s = s_wave[k];
            if (k < wave) before += s;
            all += s;
        }
        if (t < n_tiles) sums[t] = carry + before + (incl - v);
        carry += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void overlap_offsets_kernel(const uint32_t* __restrict__ counts, uint32_t total,
                                                              const uint64_t* __restrict__ tile_prefix,   // nullptr: one tile
                                                              uint64_t* __restrict__ offsets)             // total + 1 words
{
    __shared__ uint64_t s_wave[4];
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + threadIdx.x * 4u;
    const uint4 c = load_tile_counts(counts, first, total);
    const uint64_t mine = ((uint64_t)c.x + c.y) + ((uint64_t)c.z + c.w);
    const uint64_t incl = wave_inclusive_sum_u64(mine);
    const uint32_t wave = threadIdx.x / LBVH_WAVE;
    if (lane_id() == LBVH_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint64_t o0 = (tile_prefix ? tile_prefix[blockIdx.x] : 0) + (incl - mine);
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++)
        if (k < wave) o0 += s_wave[k];
    const uint64_t o1 = o0 + c.x, o2 = o1 + c.y, o3 = o2 + c.z;
    if (first + 3 <= total && ((uintptr_t)offsets & 15) == 0) {
        ulonglong2* dst = reinterpret_cast<ulonglong2*>(offsets + first);
        dst[0] = make_ulonglong2(o0, o1);
        dst[1] = make_ulonglong2(o2, o3);
    } else {
        if (first <= total) offsets[first] = o0;
        if (first + 1 <= total) offsets[first + 1] = o1;
        if (first + 2 <= total) offsets[first + 2] = o2;
        if (first + 3 <= total) offsets[first + 3] = o3;
    }
}

}  // namespace

// the four-wide form of the derived tree, made on first use after a rebuild and shared by the ray and the point walkers, and the
// stack split clamped to what those walkers have room for
lbvh_status use_wide_nodes(lbvh_context* ctx, walk_launch* w)
{
    if (!ctx->wide_valid) {
        const uint32_t n_internal = ctx->fast_src.n - 1;
        const int rc = lbvh_reserve(ctx, &ctx->wide_nodes, &ctx->wide_nodes_bytes, (size_t)n_internal * sizeof(lbvh_wide_node));
        if (rc != LBVH_OK) return (lbvh_status)rc;
        LBVH_LAUNCH(ctx, collapse_wide_kernel, dim3((n_internal + 255) / 256), dim3(256), ctx->fast_nodes, n_internal,
                    (lbvh_wide_node*)ctx->wide_nodes);
        ctx->wide_valid = true;
    }
    w->lds = std::min<uint32_t>(ctx->ray_stack_lds, kWideStackLds);
    w->deep_cap = std::min<uint32_t>(ctx->ray_stack_deep, kWideStackDeep);
    w->wn = (const lbvh_wide_node*)ctx->wide_nodes;
    return LBVH_OK;
}

// The prologue of every entry point that walks the derived scene one ray or query per lane, after the entry point's own argument
// checks: h_scene must be what the derived scene was built from (`who`: the entry point's name in the message), the ray scratch
// holds `count` lanes' worth, and `w` is what the launches take.
// The scratch is laid out as for lbvh_trace_rays whatever the caller, [two live-ray counters (256 B) | live-ray list 0 | live-ray
// list 1 | deep stack slabs of the launch's waves] (ray_scratch_bytes_for): the queries over plain rays, points and spheres use
// the slabs only (the overlap queries also the lists' space), so the live-path list a bounce may have left there is dropped —
// except for keep_list (lbvh_path_bounce, which goes on from that list) while the scratch stays where it was.
// wide: the four-wide walk is the only one the caller has.  launch_ray_walk's callers pass false: it asks for the wide nodes itself,
// after their own launches, where its walker switch takes that walk.
lbvh_status begin_walk(lbvh_context* ctx, const lbvh_scene* h_scene, size_t count, const char* who, bool wide, walk_launch* w, bool keep_list)
{
    {
        const int frc = lbvh_require_fast(ctx, *h_scene, who);
        if (frc != LBVH_OK) return frc;
    }
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    void* before = ctx->ray_scratch;
    const int rc = lbvh_reserve(ctx, &ctx->ray_scratch, &ctx->ray_scratch_bytes, ray_scratch_bytes_for(count));
    if (rc != LBVH_OK) return rc;
    if (!keep_list || ctx->ray_scratch != before) ctx->ray_list.valid = false;
    // (lbvh_debug_ray_waves can only lower the grid: the slabs stay sized by ray_waves_of(count), one per launched wave and more)
    w->waves = ray_waves_of(count);
    if (ctx->ray_max_waves != 0u) w->waves = std::min(w->waves, ctx->ray_max_waves);
    w->deep = deep_stacks(ctx, count);
    return wide ? use_wide_nodes(ctx, w) : LBVH_OK;
}

// the scan behind every CSR answer (lbvh_walk.h says where the counts and the tile sums live)
void csr_offsets(lbvh_context* ctx, size_t slots, uint64_t* d_offsets_out)
{
    const uint32_t total = (uint32_t)slots, n_tiles = total / kScanTile + 1u;
    const uint32_t* counts = csr_counts(ctx, slots);
    uint64_t* tile_sums = n_tiles > 1u ? (uint64_t*)ray_list(ctx, slots, 1) : nullptr;
    if (tile_sums) {
        LBVH_LAUNCH(ctx, overlap_tile_sums_kernel, dim3(n_tiles), dim3(256), counts, total, tile_sums);
        LBVH_LAUNCH(ctx, overlap_scan_sums_kernel, dim3(1), dim3(1024), tile_sums, n_tiles);
    }
    LBVH_LAUNCH(ctx, overlap_offsets_kernel, dim3(n_tiles), dim3(256), counts, total, (const uint64_t*)tile_sums, d_offsets_out);
}

extern "C" {

lbvh_status lbvh_debug_ray_walker(lbvh_context* ctx, uint32_t walker)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, walker <= 2u);
    ctx->ray_walker = walker;
    return LBVH_OK;
}

lbvh_status lbvh_debug_ray_stack_split(lbvh_context* ctx, uint32_t lds_entries)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, lds_entries >= 1 && lds_entries <= (uint32_t)kRayStackLds);
    ctx->ray_stack_lds = lds_entries;
    return LBVH_OK;
}

lbvh_status lbvh_debug_ray_waves(lbvh_context* ctx, uint32_t max_waves)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, max_waves <= kRayWaves);
    ctx->ray_max_waves = max_waves;
    return LBVH_OK;
}

lbvh_status lbvh_ray_stats_target(lbvh_context* ctx, lbvh_ray_stats* d_stats)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, ((uintptr_t)d_stats & 7) == 0);
    ctx->ray_stats = d_stats;
    return LBVH_OK;
}

lbvh_status lbvh_debug_ray_stack_limit(lbvh_context* ctx, uint32_t deep_entries)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    ctx->ray_stack_deep = deep_entries == 0u ? 0xFFFFFFFFu : deep_entries;       // the kernels clamp it to their slab's size
    return LBVH_OK;
}

}  // extern "C"
