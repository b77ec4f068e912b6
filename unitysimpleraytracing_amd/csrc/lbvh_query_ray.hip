// lbvh_query_ray.hip — queries over plain rays beyond the closest hit (include/lbvh.h): the first k hits (lbvh_trace_k_closest),
// every hit as a CSR list (lbvh_gather_hits), crossing parities of points (lbvh_point_crossings).  Each family's kernel, launcher
// and entry point together; the walk's shared pieces: lbvh_walk.h; the scan that gather_hits_wide_kernel's comment calls "the
// scan above" (the three overlap_* kernels behind every CSR answer): lbvh_walk.hip, reached through csr_query.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "lbvh_walk.h"

namespace {

// lbvh_trace_k_closest: the walk of trace_rays_wide_kernel<true, kClosest> with "closest so far" replaced by "k-th closest so far",
// and the per-lane list of k_closest_wide_kernel: three arrays [slot][lane] of t bits, triangle index and the index of the
// triangle's line, `cap` slots per lane, dynamic LDS sized at the launch from k (768 * k bytes per wave).  (best_t, best_tri) is the
// pruning bound: (T, 0) while fewer than k candidates are held — the state the closest walk starts in, so t == T is never taken —,
// then the list's last entry; a leaf is taken by the closest walk's own comparison against it and inserted by shifting the entries
// that sort after it.  Boxes are skipped on their ENTRY distance only, strictly beyond the bound.  With k = 1 every decision is
// the closest walk's.  u and v are not carried: when a ray's walk ends, ray_fast_triangle is evaluated once more on the stored
// line of each survivor — the same operations on the same values, hence the same words — and the row is written, padded with
// miss records.
template <bool STATS>
__global__ __launch_bounds__(64) void k_hits_wide_kernel(const lbvh_ray* __restrict__ rays, uint32_t total, uint32_t cap,
                                                         const lbvh_wide_node* __restrict__ wide,
                                                         const lbvh_fast_node* __restrict__ lines,
                                                         lbvh_hit* __restrict__ out,               // [total][cap]
                                                         uint32_t* __restrict__ found_out,         // [total] or nullptr
                                                         uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                         uint32_t lds_depth,              // <= kWideStackLds
                                                         uint32_t deep_cap,               // <= kWideStackDeep
                                                         uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    extern __shared__ uint32_t s_list[];                 // [3][cap][64]: t bits | triangle index | line index
    const uint32_t lane = threadIdx.x;
    uint32_t* const l_t = s_list + lane;
    uint32_t* const l_tri = l_t + cap * LBVH_WAVE;
    uint32_t* const l_line = l_tri + cap * LBVH_WAVE;
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_rays = 0, n_steps = 0, n_tris = 0;
    const float4 miss_record = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);

    bool active = false;
    uint32_t i = 0;
    ray_t ray = {};
    float lo = 0.0f, best_t = LBVH_MAX_FLOAT;
    uint32_t best_tri = 0, held = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong row: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float4* r = reinterpret_cast<const float4*>(&rays[k]);
                    const float4 o = r[0], d = r[1];
                    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
                    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
                    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
                    lo = o.w;
                    best_t = fminf(d.w, LBVH_MAX_FLOAT);         // T: candidates lie in (t_min, T)
                    best_tri = 0; held = 0; sp = 0; node = 0;
                    active = o.w < d.w;                          // load_plain_ray's rule: false for NaN bounds too
                    if (!active) {                               // no candidates, no walk: the whole row is miss records
                        float4* row = reinterpret_cast<float4*>(out) + (size_t)k * cap;
                        for (uint32_t j = 0; j < cap; j++) row[j] = miss_record;
                        if (found_out) found_out[k] = 0u;
                    }
                    if (STATS && active) n_rays++;
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
            float t0, t1, t2, t3;
            const bool h0 = wide_box(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, ray, t0) && !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, ray, t1) && !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, ray, t2) && !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, ray, t3) && !(t3 > best_t) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), v0, v1, v2);
                float u = 0.0f, v = 0.0f;
                const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                const uint32_t tri = __float_as_uint(v0.w);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // (best_t, best_tri) is (T, 0) until k are held: dist == T is never taken.  Then it is the k-th held: the candidate
                // must sort before it, ties by the lower triangle index
                if (dist > lo && hit_counts(dist, entry) && (dist < best_t || (dist == best_t && tri < best_tri))) {
                    uint32_t j = min(held, cap - 1u);    // the slot that becomes free: the end of the list, or its dropped last entry
                    while (j != 0u) {
                        const float tj = __uint_as_float(l_t[(j - 1u) * LBVH_WAVE]);
                        const uint32_t ij = l_tri[(j - 1u) * LBVH_WAVE];
                        if (!(dist < tj || (dist == tj && tri < ij))) break;
                        l_t[j * LBVH_WAVE] = __float_as_uint(tj);
                        l_tri[j * LBVH_WAVE] = ij;
                        l_line[j * LBVH_WAVE] = l_line[(j - 1u) * LBVH_WAVE];
                        j--;
                    }
                    l_t[j * LBVH_WAVE] = __float_as_uint(dist);
                    l_tri[j * LBVH_WAVE] = tri;
                    l_line[j * LBVH_WAVE] = line;
                    held = min(held + 1u, cap);
                    if (held == cap) {
                        best_t = __uint_as_float(l_t[(cap - 1u) * LBVH_WAVE]);
                        best_tri = l_tri[(cap - 1u) * LBVH_WAVE];
                    }
                }
            }
            // nodes to enter, ordered by entry distance: the order key is the distance's bit pattern (non-negative floats
            // order like integers) with the slot number in its two lowest bits.  (best_t may have shrunk in the leaf loop since
            // h0 .. h3 were formed: the entry distances are compared with it once more)
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(t0 > best_t) ? ((__float_as_uint(fmaxf(t0, 0.0f)) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(t1 > best_t) ? ((__float_as_uint(fmaxf(t1, 0.0f)) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(t2 > best_t) ? ((__float_as_uint(fmaxf(t2, 0.0f)) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(t3 > best_t) ? ((__float_as_uint(fmaxf(t3, 0.0f)) & ~3u) | 3u) : none;
            {   // five compare-exchanges
                uint32_t a, b;
                a = min(k0, k1); b = max(k0, k1); k0 = a; k1 = b;
                a = min(k2, k3); b = max(k2, k3); k2 = a; k3 = b;
                a = min(k0, k2); b = max(k0, k2); k0 = a; k2 = b;
                a = min(k1, k3); b = max(k1, k3); k1 = a; k3 = b;
                a = min(k1, k2); b = max(k1, k2); k1 = a; k2 = b;
            }
            if (k0 != none) {
                if (k3 != none) push(pick4(ref, k3 & 3u));       // farthest first: the nearest waiting sibling is popped first
                if (k2 != none) push(pick4(ref, k2 & 3u));
                if (k1 != none) push(pick4(ref, k1 & 3u));
                node = pick4(ref, k0 & 3u);
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                // the row: the survivors in order, t, u and v from their lines again, then miss records
                float4* row = reinterpret_cast<float4*>(out) + (size_t)i * cap;
                for (uint32_t j = 0; j < held; j++) {
                    float4 v0, v1, v2;
                    unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[l_line[j * LBVH_WAVE]]), v0, v1, v2);
                    float u = 0.0f, v = 0.0f;
                    const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                    row[j] = make_float4(dist, v0.w, u, v);
                }
                for (uint32_t j = held; j < cap; j++) row[j] = miss_record;
                if (found_out) found_out[i] = held;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_rays, n_steps, n_tris);
}

}  // namespace

extern "C" {

// the four-wide walk only (lbvh_debug_ray_walker does not apply), one launch; the per-lane lists are dynamic LDS sized from k
lbvh_status lbvh_trace_k_closest(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, uint32_t k, const lbvh_scene* h_scene,
                                 lbvh_hit* d_hits, uint32_t* d_found)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_rays != nullptr && h_scene != nullptr && d_hits != nullptr);
    LBVH_REQUIRE(ctx, k >= 1u && k <= (uint32_t)LBVH_K_CLOSEST_MAX);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_hits & 15) == 0 && ((uintptr_t)d_found & 3) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_trace_k_closest", true, &w);
    if (rc != LBVH_OK) return rc;
    const size_t list_lds = (size_t)3 * k * LBVH_WAVE * sizeof(uint32_t);       // 768 bytes per slot: 24 KiB at k = 32
    LBVH_LAUNCH_STATS_SHMEM(ctx, ctx->ray_stats, k_hits_wide_kernel<STATS>, dim3(w.waves), dim3(LBVH_WAVE), list_lds, d_rays, (uint32_t)count, k,
                            w.wn, ctx->fast_nodes, d_hits, d_found, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

}  // extern "C"

namespace {

// ---- every hit along a ray as a CSR list (lbvh_gather_hits, include/lbvh.h) --------------------------------------------
// The frame of overlap_wide_kernel (count walk, the scan above, fill walk: the same kernel, the same decisions, so a segment can
// never outgrow its slot) around the ray arithmetic of trace_rays_wide_kernel<true, kCount>: load_plain_ray's activity test and T,
// the slab tests against the FIXED bound T, ray_fast_triangle, hit_counts(dist, entry) and lo < dist < T.  Nothing shrinks and no
// order is promised, so the ordering network of the ray walkers is not needed: the first passing inner slot is entered, the
// others wait on the stack.  A candidate's record is the float4 put_hit would write were it the nearest: {dist, tri, u, v}.
// A kernel of its own and not a fourth walk_query: a new parameter would move the arguments of every other instantiation.
template <bool FILL, bool STATS>
__global__ __launch_bounds__(64) void gather_hits_wide_kernel(const lbvh_ray* __restrict__ rays, uint32_t total,
                                                              const lbvh_wide_node* __restrict__ wide,
                                                              const lbvh_fast_node* __restrict__ lines,
                                                              uint32_t* __restrict__ counts,            // !FILL: candidates of ray k
                                                              const uint64_t* __restrict__ offsets,     // FILL: where segment k starts
                                                              lbvh_hit* __restrict__ hits, uint64_t capacity,
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
    uint32_t n_rays = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t ray = {};
    float lo = 0.0f, T = LBVH_MAX_FLOAT;
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // FILL: where this lane's next record goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short segment: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float4* r = reinterpret_cast<const float4*>(&rays[k]);
                    const float4 o = r[0], d = r[1];
                    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
                    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
                    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
                    lo = o.w;
                    T = fminf(d.w, LBVH_MAX_FLOAT);              // candidates lie in (t_min, T)
                    active = o.w < d.w;                          // load_plain_ray's rule: false for NaN bounds too
                    sp = 0; node = 0;
                    if constexpr (FILL) { if (active) pos = offsets[k]; }      // (reloaded at every refill: a lane serves many rays)
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_rays++;
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
            float t0, t1, t2, t3;
            const bool h0 = wide_box(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, ray, t0) && !(t0 > T) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, ray, t1) && !(t1 > T) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, ray, t2) && !(t2 > T) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, ray, t3) && !(t3 > T) && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                float u = 0.0f, v = 0.0f;
                const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                if (dist > lo && hit_counts(dist, entry) && dist < T) {
                    if constexpr (FILL) {
                        if (pos < capacity) reinterpret_cast<float4*>(hits)[pos] = make_float4(dist, v0.w, u, v);   // never at or beyond the capacity
                        pos++;
                    } else {
                        n_found++;
                    }
                }
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
                if constexpr (!FILL) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_rays, n_steps, n_tris);
}

}  // namespace

extern "C" {

// a CSR answer of hit records.  Four-wide walk only.
lbvh_status lbvh_gather_hits(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                             lbvh_hit* d_hits, uint64_t capacity)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_rays != nullptr && h_scene != nullptr && d_offsets != nullptr);
    LBVH_REQUIRE(ctx, d_hits != nullptr || capacity == 0);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_hits & 15) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_gather_hits", true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (gather_hits_wide_kernel<false, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_rays, total, w.wn, ctx->fast_nodes,
                              counts, (const uint64_t*)nullptr, (lbvh_hit*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (gather_hits_wide_kernel<true, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_rays, total, w.wn, ctx->fast_nodes,
                              (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_hits, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        });
}

}  // extern "C"

namespace {

// ---- crossing parities of points along fixed directions (lbvh_point_crossings, include/lbvh.h) -------------------------
// The directions travel by value in the kernel's arguments; a lane reads the one it walks next from there.
struct crossing_dirs { float d[LBVH_CROSSING_MAX_DIRS][3]; };

// One POINT per lane over the four-wide nodes, in the frame of trace_rays_wide_kernel<PLAIN> (persistent waves, lanes refilled
// from the wave's run of consecutive points, LDS + device-memory stack).  The lane walks the rays {p, t_min = 0, dirs[j],
// T = LBVH_MAX_FLOAT} for j = 0 .. n_dirs - 1 one after the other: the count walk of the ray walkers (best_t stays T, every
// candidate adds one, the walk ends with an empty stack), each finished count's lowest bit kept in a register and the point's
// word stored once, after its last direction.  No ray is written to memory.  The children to enter are taken in slot order: a
// count does not depend on the order, and at most three siblings wait per level as in the other walks.
// amdgpu_waves_per_eu(8): without it the lane-indexed direction and the point / direction / parity registers took 66 VGPRs
// (7 waves per SIMD) and the walk was slower than lbvh_count_hits on the same rays written out
template <bool STATS>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void point_crossings_wide_kernel(const lbvh_point_query* __restrict__ points, uint32_t total,
                                                                  const crossing_dirs dirs, uint32_t n_dirs,
                                                                  const lbvh_wide_node* __restrict__ wide,
                                                                  const lbvh_fast_node* __restrict__ lines, uint32_t* __restrict__ parity,
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
    uint32_t n_rays = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0, j = 0, bits = 0, n_hit = 0;          // point, direction, parities so far, candidates of direction j so far
    ray_t ray = {};
    uint32_t sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong count: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    auto aim = [&](uint32_t jj) {                        // direction jj from the lane's point: a fresh walk
        ray.dx = dirs.d[jj][0]; ray.dy = dirs.d[jj][1]; ray.dz = dirs.d[jj][2];
        ray.ix = 1.0f / ray.dx; ray.iy = 1.0f / ray.dy; ray.iz = 1.0f / ray.dz;
        sp = 0; node = 0; n_hit = 0;
        if (STATS) n_rays++;
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float4 p = reinterpret_cast<const float4*>(points)[k];     // max_dist2 (.w) is not read
                    ray.ox = p.x; ray.oy = p.y; ray.oz = p.z;
                    j = 0; bits = 0;
                    aim(0u);
                    active = true;
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
            float t0, t1, t2, t3;
            // T = min(+inf, LBVH_MAX_FLOAT): a box entered beyond it holds no candidate
            const bool h0 = wide_box(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, ray, t0) && !(t0 > LBVH_MAX_FLOAT) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, ray, t1) && !(t1 > LBVH_MAX_FLOAT) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, ray, t2) && !(t2 > LBVH_MAX_FLOAT) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, ray, t3) && !(t3 > LBVH_MAX_FLOAT) && ref.w != kWideEmpty;
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                float u = 0.0f, v = 0.0f;
                const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                if (dist > 0.0f && hit_counts(dist, entry) && dist < LBVH_MAX_FLOAT) n_hit++;
            }
            // nodes to enter, in slot order: the first is walked next, the others wait
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t go = none;
            if (h0 && !(ref.x >> 31)) go = ref.x;
            if (h1 && !(ref.y >> 31)) { if (go != none) push(go); go = ref.y; }
            if (h2 && !(ref.z >> 31)) { if (go != none) push(go); go = ref.z; }
            if (h3 && !(ref.w >> 31)) { if (go != none) push(go); go = ref.w; }
            if (go != none) {
                node = go;
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                bits |= (n_hit & 1u) << j;
                j++;
                if (j < n_dirs) {
                    aim(j);
                } else {
                    parity[i] = bits;
                    active = false;
                }
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_rays, n_steps, n_tris);
}

}  // namespace

extern "C" {

// the four-wide walk only (lbvh_debug_ray_walker does not apply), the directions by value in the arguments
lbvh_status lbvh_point_crossings(lbvh_context* ctx, const lbvh_point_query* d_points, size_t count, const float* h_dirs, uint32_t n_dirs,
                                 const lbvh_scene* h_scene, uint32_t* d_parity)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_points != nullptr && h_dirs != nullptr && h_scene != nullptr && d_parity != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_points & 15) == 0 && ((uintptr_t)d_parity & 3) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    LBVH_REQUIRE(ctx, n_dirs >= 1u && n_dirs <= (uint32_t)LBVH_CROSSING_MAX_DIRS);
    crossing_dirs dirs = {};
    for (uint32_t j = 0; j < n_dirs; j++) {
        const float x = h_dirs[3 * j], y = h_dirs[3 * j + 1], z = h_dirs[3 * j + 2];
        LBVH_REQUIRE(ctx, std::isfinite(x) && std::isfinite(y) && std::isfinite(z));
        LBVH_REQUIRE(ctx, x != 0.0f || y != 0.0f || z != 0.0f);
        dirs.d[j][0] = x; dirs.d[j][1] = y; dirs.d[j][2] = z;
    }
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_point_crossings", true, &w);
    if (rc != LBVH_OK) return rc;
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, point_crossings_wide_kernel<STATS>, dim3(w.waves), dim3(LBVH_WAVE), d_points, (uint32_t)count, dirs,
                      n_dirs, w.wn, ctx->fast_nodes, d_parity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

}  // extern "C"
