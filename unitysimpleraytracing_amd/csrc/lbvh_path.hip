// lbvh_path.hip — SURVEY 8(f) rank 3: rigid per-body animation, arbitrary-ray traversal and the bounce
// step of a 1-spp path tracer (BASELINE configs[4]).  No reference counterpart: the reference traces
// primary rays of a static mesh only.  Definitions: include/lbvh.h; bit-exact checker: oracle/.
// Strict fp32 (-ffp-contract=off), no device trig, counter-based RNG.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "lbvh_common.h"
#include "lbvh_rt.h"
#include "lbvh_walk.h"

namespace {

// ---- animation --------------------------------------------------------------------------------------
// One thread per 16-byte quarter-row of a triangle (8 of them per 128-byte record): a wave's load and its store cover 1 KB of
// consecutive bytes.  (One thread per triangle touched 64 different lines with every one of its 8 loads and 8 stores: 74 us per
// million triangles against the 45 us the 256 MB take at the copy rate.)
__global__ __launch_bounds__(256) void animate_kernel(const lbvh_triangle* __restrict__ rest, uint32_t n,
                                                      const uint32_t* __restrict__ body, const float4* __restrict__ centres,
                                                      float c, float s, lbvh_triangle* __restrict__ out)
{
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = (uint32_t)(g >> 3), k = (uint32_t)g & 7u;
    if (i >= n) return;
    float4 p = reinterpret_cast<const float4*>(rest)[g];
    if (k < 3u) {                                        // positions a, b, c
        const float4 ctr = centres[body[i]];
        const float x = p.x - ctr.x, z = p.z - ctr.z;
        p.x = (c * x + s * z) + ctr.x;                   // rotation about Y through the body centre
        p.z = (c * z - s * x) + ctr.z;
    } else if (k >= 5u) {                                // normals (k = 3, 4: uv, copied)
        const float nx = p.x, nz = p.z;
        p.x = c * nx + s * nz;
        p.z = c * nz - s * nx;
    }
    reinterpret_cast<float4*>(out)[g] = p;
}

// ---- camera rays -> path states ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void path_begin_kernel(lbvh_camera cam, lbvh_path_state* __restrict__ states)
{
    const uint32_t x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= (uint32_t)cam.screen_width || y >= (uint32_t)cam.screen_height) return;
    const ray_t r = make_ray(cam, x, y);
    float4* o = reinterpret_cast<float4*>(&states[(size_t)y * cam.screen_width + x]);
    o[0] = make_float4(r.ox, r.oy, r.oz, __uint_as_float(1u));
    o[1] = make_float4(r.dx, r.dy, r.dz, 0.0f);
    o[2] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// ---- arbitrary rays: one ray per lane over the derived traversal scene -----------------------------------
// Secondary rays are incoherent, so the packet walk of lbvh_trace.hip does not apply: every lane walks on its
// own (64-byte fused nodes, near child first, boxes beyond the best hit skipped) with a stack of its own, laid out
// [entry][lane].  One wave per workgroup, no barriers.  The stack split, the grid, the lane refill and the four-wide node: lbvh_walk.h.
// Live rays only: alive_rays_kernel writes the miss record of every dead ray and compacts the indices of the live
// ones (after the first bounce more than half of a frame's paths have left the scene).  (Sorting the live rays by direction octant + Morton code of the origin on top of this was
// measured: the sort costs 0.15 ms per bounce and the walk does not get faster.  Measured again in round 5 on the four-wide
// walkers with counters, profiles/r5/c_ray_sort_between_bounces.txt: HBM-side fetch -17 %, L2 misses -15 %, walk time 1.206 ->
// 1.201 ms — the walk waits for its rays' dependent line fetches at full occupancy, not for bandwidth.)
__global__ __launch_bounds__(256) void alive_rays_kernel(const lbvh_path_state* __restrict__ states, size_t count,
                                                         uint32_t* __restrict__ n_alive, uint32_t* __restrict__ list,
                                                         lbvh_hit* __restrict__ hits)
{
    __shared__ uint32_t s_n, s_base;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    bool alive = false;
    if (i < count) {
        alive = reinterpret_cast<const uint32_t*>(&states[i])[3] != 0u;
        if (!alive) reinterpret_cast<float4*>(hits)[i] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
    }
    const uint64_t m = __ballot(alive);
    uint32_t wave_ofs = 0;
    if (lane_id() == 0 && m) wave_ofs = atomicAdd(&s_n, (uint32_t)__popcll(m));
    wave_ofs = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_ofs);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) s_base = __hip_atomic_fetch_add(n_alive, s_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (alive) list[s_base + wave_ofs + mbcnt64(m)] = (uint32_t)i;
}

// The three walkers below serve two ray sources and three queries (template arguments PLAIN, Q):
//   PLAIN = false: path states, the live ones listed in `list` (*n_alive of them), one t_min for all (lbvh_trace_rays, the bounces)
//   PLAIN = true:  lbvh_ray records, ray k of the call to the lane directly (n_alive = the count), per-ray [t_min, t_max);
//                  a ray with !(t_min < t_max) gets its result when it is loaded and leaves the lane idle for the next refill
//   Q = kClosest:  the closest candidate's lbvh_hit; kAny: a uint32_t flag, 1 as soon as any candidate is accepted (the
//                  closest-hit walk cut off there: the same near-first order, the rest of that step's leaves skipped);
//   kCount:        a uint32_t, the number of candidates (plain rays only): best_t stays T, every accepted candidate adds one and
//                  the walk ends with an empty stack.  Boxes are skipped as in the other two, when missed or entered beyond T,
//                  never on their exit distance (a candidate's t may lie beyond its own box's exit)
enum walk_query : int { kClosest = 0, kAny = 1, kCount = 2 };
template <bool PLAIN> using walk_src = std::conditional_t<PLAIN, lbvh_ray, lbvh_path_state>;
template <bool PLAIN> using walk_total = std::conditional_t<PLAIN, uint32_t, const uint32_t* __restrict__>;
template <int Q> using walk_out = std::conditional_t<Q != kClosest, uint32_t, lbvh_hit>;
__device__ __forceinline__ uint32_t walk_count(uint32_t count) { return count; }
__device__ __forceinline__ uint32_t walk_count(const uint32_t* n_alive) { return *n_alive; }

// plain ray k into the lane (lo = t_min, best_t = T): false (result written, lane stays idle) for an inactive ray
template <int Q>
__device__ __forceinline__ bool load_plain_ray(const lbvh_ray* __restrict__ rays, uint32_t k, ray_t& ray, float& lo, float& best_t,
                                               walk_out<Q>* __restrict__ out)
{
    const float4* r = reinterpret_cast<const float4*>(&rays[k]);
    const float4 o = r[0], d = r[1];
    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
    lo = o.w;
    best_t = fminf(d.w, LBVH_MAX_FLOAT);                 // T: candidates lie in (t_min, T)
    if (o.w < d.w) return true;                          // false for NaN bounds too
    if constexpr (Q != kClosest) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
    return false;
}

// a finished closest-hit walk's record; a plain ray that accepted nothing still holds best_t = min(t_max, MAX_FLOAT): the miss
// record instead (a lane mask, `took`, says which: the bound itself would take one more VGPR for the whole walk)
template <bool PLAIN>
__device__ __forceinline__ void put_hit(lbvh_hit* __restrict__ hits, size_t i, float best_t, bool took, uint32_t best_tri, float best_u, float best_v)
{
    float4 out;
    out.x = PLAIN && !took ? LBVH_MAX_FLOAT : best_t;
    out.y = __uint_as_float(best_tri);
    out.z = best_u;
    out.w = best_v;
    reinterpret_cast<float4*>(hits)[i] = out;
}

template <bool PLAIN, int Q>
__global__ __launch_bounds__(64) void trace_rays_kernel(const walk_src<PLAIN>* __restrict__ states, walk_total<PLAIN> n_alive,
                                                        const uint32_t* __restrict__ list, float t_min,
                                                        const lbvh_fast_node* __restrict__ nodes,
                                                        const lbvh_fast_tri* __restrict__ tris, walk_out<Q>* __restrict__ hits,
                                                        uint32_t* __restrict__ deep,     // [gridDim.x][kRayStackDeep][64]
                                                        uint32_t lds_depth,              // <= kRayStackLds
                                                        uint32_t deep_cap,               // <= kRayStackDeep (lbvh_debug_ray_stack_limit lowers it)
                                                        uint32_t* __restrict__ fault)    // mapped host word: a stack that ran out says so here
{
    constexpr bool ANY = Q == kAny, COUNT = Q == kCount;
    __shared__ uint32_t s_stack[kRayStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kRayStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t total = walk_count(n_alive);
    // at least 32 rays per wave: with fewer live rays than lanes on the chip, half-filled waves on every wave slot hide more
    // latency than full waves on half of them (4 bounces: 1.487 -> 1.443 ms; 64: 1.487, 16: 1.449, 96 / 128 / 192: 1.71 / 1.91 / 2.43)
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;                      // scalar: next unclaimed entry of this wave's run
    if (next >= total) return;
    const uint32_t end = min(next + run, total);

    bool active = false;
    size_t i = 0;
    ray_t ray = {};
    float lo = t_min;                                    // the ray's t_min (plain rays: best_t starts at min(t_max, MAX_FLOAT))
    bool took = false;                                   // plain rays: a candidate was accepted (else best_t is still that bound)
    float best_t = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    uint32_t n_hit = 0;                                  // COUNT: candidates accepted so far
    for (;;) {
        // refill idle lanes from the chunk
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    if constexpr (PLAIN) {
                        i = k;
                        active = load_plain_ray<Q>(states, k, ray, lo, best_t, hits);
                        best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                        sp = 0; node = 0;
                        if constexpr (COUNT) n_hit = 0;
                    } else {
                        i = list[k];
                        const float4* st = reinterpret_cast<const float4*>(&states[i]);
                        const float4 o = st[0], d = st[1];
                        ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
                        ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
                        ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
                        best_t = LBVH_MAX_FLOAT; best_tri = 0; best_u = 0.0f; best_v = 0.0f;
                        sp = 0; node = 0;
                        active = true;
                    }
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && (!PLAIN || next >= end)) break;      // (plain rays: a whole refill can be inactive rays)
        if (active) {
            const float4* nb = reinterpret_cast<const float4*>(&nodes[node]);
            const float4 lmin = nb[0], lmax = nb[1], rmin = nb[2], rmax = nb[3];
            const uint32_t lref = __float_as_uint(lmin.w), rref = __float_as_uint(lmax.w);
            float tl, tr;
            bool hit_l = ray_box(lmin, lmax, ray, tl) && !(tl > best_t);
            bool hit_r = ray_box(rmin, rmax, ray, tr) && !(tr > best_t);
            bool found = false;                          // ANY: a candidate was accepted
#pragma unroll
            for (int side = 0; side < 2; side++) {
                const bool h = side == 0 ? hit_l : hit_r;
                const uint32_t ref = side == 0 ? lref : rref;
                if (h && (ref & 0x80000000u) && !found) {
                    float4 v0, v1, v2;
                    unpack_fast_triangle(reinterpret_cast<const float4*>(&nodes[ref & 0x7FFFFFFFu]), v0, v1, v2);   // a triangle line
                    float u = 0.0f, v = 0.0f;
                    const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                    const uint32_t tri = __float_as_uint(v0.w);
                    if constexpr (COUNT) {
                        if (dist > lo && hit_counts(dist, side == 0 ? tl : tr) && dist < best_t) n_hit++;
                    } else if (dist > lo && hit_counts(dist, side == 0 ? tl : tr) && (dist < best_t || (dist == best_t && tri < best_tri))) {
                        if constexpr (ANY) found = true;
                        else { best_t = dist; best_tri = tri; best_u = u; best_v = v; took = true; }
                    }
                }
            }
            const bool go_l = hit_l && !(lref & 0x80000000u) && !(tl > best_t);
            const bool go_r = hit_r && !(rref & 0x80000000u) && !(tr > best_t);
            if (ANY && found) {
                if constexpr (ANY) hits[i] = 1u;
                active = false;
            } else if (go_l && go_r) {
                const bool l_near = tl <= tr;
                node = l_near ? lref : rref;
                const uint32_t far = l_near ? rref : lref;
                if (sp < lds_depth) { s_stack[sp][lane] = far; sp++; }
                else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = far; sp++; }
                else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // never on this library's trees (see kWideStackDeep)
            } else if (go_l) {
                node = lref;
            } else if (go_r) {
                node = rref;
            } else if (sp != 0) {
                sp--;
                node = sp < lds_depth ? s_stack[sp][lane] : my_deep[(sp - lds_depth) * LBVH_WAVE];
            } else {
                if constexpr (COUNT) hits[i] = n_hit;
                else if constexpr (ANY) hits[i] = 0u;
                else put_hit<PLAIN>(hits, i, best_t, took, best_tri, best_u, best_v);
                active = false;
            }
        }
    }
}

// Same frame as trace_rays_kernel (lane refill from the wave's run of live rays, LDS + device-memory stack).
template <bool PLAIN, int Q, bool STATS>
__global__ __launch_bounds__(64) void trace_rays_wide_kernel(const walk_src<PLAIN>* __restrict__ states, walk_total<PLAIN> n_alive,
                                                             const uint32_t* __restrict__ list, float t_min,
                                                             const lbvh_wide_node* __restrict__ wide,
                                                             const lbvh_fast_node* __restrict__ lines, walk_out<Q>* __restrict__ hits,
                                                             uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                             uint32_t lds_depth,              // <= kWideStackLds
                                                             uint32_t deep_cap,               // <= kWideStackDeep
                                                             uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    constexpr bool ANY = Q == kAny, COUNT = Q == kCount;
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t total = walk_count(n_alive);
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_rays = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    size_t i = 0;
    ray_t ray = {};
    float lo = t_min;
    bool took = false;
    float best_t = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    uint32_t n_hit = 0;                                  // COUNT: candidates accepted so far
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong hit: report it.  Cannot happen on this library's trees (a radix
        // tree over unique 32-bit keys is <= 32 levels deep, 3 waiting siblings per level); lbvh_debug_ray_stack_limit provokes it
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    if constexpr (PLAIN) {
                        i = k;
                        active = load_plain_ray<Q>(states, k, ray, lo, best_t, hits);
                        best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                        sp = 0; node = 0;
                        if constexpr (COUNT) n_hit = 0;
                        if (STATS && active) n_rays++;
                    } else {
                        i = list[k];
                        const float4* st = reinterpret_cast<const float4*>(&states[i]);
                        const float4 o = st[0], d = st[1];
                        ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
                        ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
                        ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
                        best_t = LBVH_MAX_FLOAT; best_tri = 0; best_u = 0.0f; best_v = 0.0f;
                        sp = 0; node = 0;
                        active = true;
                        if (STATS) n_rays++;
                    }
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && (!PLAIN || next >= end)) break;
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
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                float u = 0.0f, v = 0.0f;
                const float dist = ray_fast_triangle(ray, v0, v1, v2, u, v);
                const uint32_t tri = __float_as_uint(v0.w);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // ties go to the lower triangle index, whatever order the leaves are met in (as in the packet walk)
                if constexpr (COUNT) {
                    if (dist > lo && hit_counts(dist, entry) && dist < best_t) n_hit++;
                } else if (dist > lo && hit_counts(dist, entry) && (dist < best_t || (dist == best_t && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else { best_t = dist; best_tri = tri; best_u = u; best_v = v; took = true; }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) hits[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by entry distance: the order key is the distance's bit pattern (non-negative floats
            // order like integers) with the slot number in its two lowest bits
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(t0 > best_t) ? ((__float_as_uint(fmaxf(t0, 0.0f)) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(t1 > best_t) ? ((__float_as_uint(fmaxf(t1, 0.0f)) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(t2 > best_t) ? ((__float_as_uint(fmaxf(t2, 0.0f)) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(t3 > best_t) ? ((__float_as_uint(fmaxf(t3, 0.0f)) & ~3u) | 3u) : none;
            {   // five compare-exchanges (a count does not need the order; kept: the same three waiting siblings per level at most)
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
                if constexpr (COUNT) hits[i] = n_hit;
                else if constexpr (ANY) hits[i] = 0u;
                else put_hit<PLAIN>(hits, i, best_t, took, best_tri, best_u, best_v);
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_rays, n_steps, n_tris);
}

// The same walk for launches whose time is the chain of their longest rays (the later bounces of a frame: a few hundred
// thousand live rays, most of the chip idle for most of the launch): the next node is chosen BEFORE the step's triangles are
// tested and requested together with the first triangle line, so the two fetches of a step are in flight at once.  84 VGPRs
// (5 waves per SIMD instead of 8): the price where every wave slot is needed, none where they are not.
template <bool PLAIN, int Q, bool STATS>
__global__ __launch_bounds__(64) void trace_rays_wide_chain_kernel(const walk_src<PLAIN>* __restrict__ states, walk_total<PLAIN> n_alive,
                                                             const uint32_t* __restrict__ list, float t_min,
                                                             const lbvh_wide_node* __restrict__ wide,
                                                             const lbvh_fast_node* __restrict__ lines, walk_out<Q>* __restrict__ hits,
                                                             uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                             uint32_t lds_depth,              // <= kWideStackLds
                                                             uint32_t deep_cap,               // <= kWideStackDeep
                                                             uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    constexpr bool ANY = Q == kAny, COUNT = Q == kCount;
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t total = walk_count(n_alive);
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_rays = 0, n_steps = 0, n_tris = 0;

    bool active = false, have = false;      // have: the registers below hold this lane's node
    uint32_t i = 0;                          // (lbvh_trace_rays: count <= 2^32 - 1)
    ray_t ray = {};
    float lo = t_min;
    bool took = false;
    float best_t = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    uint32_t n_hit = 0;                      // COUNT: candidates accepted so far
    float4 lox = {}, loy = {}, loz = {}, hix = {}, hiy = {}, hiz = {};
    uint4 ref = {};
    auto push = [&](uint32_t r) {
        if (sp < lds_depth) { s_stack[sp][lane] = r; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = r; sp++; }
        // a dropped entry would be a silently wrong hit: report it.  Cannot happen on this library's trees (a radix
        // tree over unique 32-bit keys is <= 32 levels deep, 3 waiting siblings per level); lbvh_debug_ray_stack_limit provokes it
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    // A step: box tests on the node fetched during the previous step, the next node chosen (against the best hit so far),
    // then the first leaf's triangle line AND the next node requested together, the triangle tests while both are on their
    // way.  The two fetches of a step overlap instead of following each other; what a leaf hit would have pruned from the
    // choice is met by the next step's box tests (its children then fail `entry <= best`).
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    if constexpr (PLAIN) {
                        i = k;
                        active = load_plain_ray<Q>(states, k, ray, lo, best_t, hits);
                        best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                        sp = 0; node = 0;
                        have = false;
                        if constexpr (COUNT) n_hit = 0;
                        if (STATS && active) n_rays++;
                    } else {
                        i = list[k];
                        const float4* st = reinterpret_cast<const float4*>(&states[i]);
                        const float4 o = st[0], d = st[1];
                        ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
                        ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
                        ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
                        best_t = LBVH_MAX_FLOAT; best_tri = 0; best_u = 0.0f; best_v = 0.0f;
                        sp = 0; node = 0;
                        active = true; have = false;
                        if (STATS) n_rays++;
                    }
                }
            }
            next += (uint32_t)__popcll(idle);
        }
        if (!__any(active) && (!PLAIN || next >= end)) break;
        uint32_t leaves = 0u;
        uint4 leaf_ref = {};
        float4 leaf_entry = {};
        bool fetch = active, done = false;
        if (active && have) {
            float t0, t1, t2, t3;
            const bool h0 = wide_box(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, ray, t0) && !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, ray, t1) && !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, ray, t2) && !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, ray, t3) && !(t3 > best_t) && ref.w != kWideEmpty;
            leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                     (h3 && (ref.w >> 31) ? 8u : 0u);
            leaf_ref = ref;
            leaf_entry = make_float4(t0, t1, t2, t3);
            // nodes to enter, ordered by entry distance: the order key is the distance's bit pattern (non-negative floats
            // order like integers) with the slot number in its two lowest bits
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) ? ((__float_as_uint(fmaxf(t0, 0.0f)) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) ? ((__float_as_uint(fmaxf(t1, 0.0f)) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) ? ((__float_as_uint(fmaxf(t2, 0.0f)) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) ? ((__float_as_uint(fmaxf(t3, 0.0f)) & ~3u) | 3u) : none;
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
                fetch = false;
                done = true;              // after this step's leaves
            }
        }
        // the first leaf's line, then the next node: requested back to back
        // (a triangle line: {v0, index} | e2.x in dword 7 | {e1, e2.y} | e2.z in dword 15)
        float4 q0 = {}, q1 = {}, q2 = {}, q3 = {};
        if (leaves != 0u) {
            const float4* line = reinterpret_cast<const float4*>(&lines[pick4(leaf_ref, (uint32_t)__builtin_ctz(leaves)) & 0x7FFFFFFFu]);
            q0 = line[0]; q1 = line[1]; q2 = line[2]; q3 = line[3];
        }
        if (fetch) {
            if (STATS) n_steps++;
            const float4* w = reinterpret_cast<const float4*>(&wide[node]);
            lox = w[0]; loy = w[1]; loz = w[2]; hix = w[3]; hiy = w[4]; hiz = w[5];
            ref = reinterpret_cast<const uint4*>(w)[6];
            have = true;
        }
        bool found = false;                          // ANY: a candidate was accepted
        while (leaves != 0u) {
            const uint32_t slot = (uint32_t)__builtin_ctz(leaves);
            const float entry = slot == 0u ? leaf_entry.x : (slot == 1u ? leaf_entry.y : (slot == 2u ? leaf_entry.z : leaf_entry.w));
            leaves &= leaves - 1u;
            if (STATS) n_tris++;
            float u = 0.0f, v = 0.0f;
            const float dist = ray_triangle_edges(ray, q0, q2.x, q2.y, q2.z, q1.w, q2.w, q3.w, u, v);
            const uint32_t tri = __float_as_uint(q0.w);
            // ties go to the lower triangle index, whatever order the leaves are met in (as in the packet walk)
            if constexpr (COUNT) {
                if (dist > lo && hit_counts(dist, entry) && dist < best_t) n_hit++;
            } else if (dist > lo && hit_counts(dist, entry) && (dist < best_t || (dist == best_t && tri < best_tri))) {
                if constexpr (ANY) { found = true; break; }
                else { best_t = dist; best_tri = tri; best_u = u; best_v = v; took = true; }
            }
            if (leaves != 0u) {
                const float4* line = reinterpret_cast<const float4*>(&lines[pick4(leaf_ref, (uint32_t)__builtin_ctz(leaves)) & 0x7FFFFFFFu]);
                q0 = line[0]; q1 = line[1]; q2 = line[2]; q3 = line[3];
            }
        }
        if (ANY && found) {
            if constexpr (ANY) hits[i] = 1u;
            active = false;
        } else if (done) {
            if constexpr (COUNT) hits[i] = n_hit;
            else if constexpr (ANY) hits[i] = 0u;
            else put_hit<PLAIN>(hits, i, best_t, took, best_tri, best_u, best_v);
            active = false;
        }
    }
    if (STATS) add_ray_stats(stats, n_rays, n_steps, n_tris);
}

// ---- point queries: nearest triangle / anything within a distance (include/lbvh.h) -----------------------------------
// squared fp32 distance of p to a box: per axis g = max(max(lo - p, p - hi), 0), (gx*gx + gy*gy) + gz*gz.  Monotone: it grows
// from a box to any box inside it (subtraction, max, products of non-negatives and sums are monotone in fp32).
__device__ __forceinline__ float point_box2(float lx, float ly, float lz, float hx, float hy, float hz, float px, float py, float pz)
{
    const float gx = fmaxf(fmaxf(lx - px, px - hx), 0.0f);
    const float gy = fmaxf(fmaxf(ly - py, py - hy), 0.0f);
    const float gz = fmaxf(fmaxf(lz - pz, pz - hz), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// squared fp32 distance of p to the triangle {a, e1, e2} of a derived-scene line and the barycentrics of its closest point:
// the region test of Ericson, Real-Time Collision Detection 5.1.5, in the operation order lbvh.h writes down.  The four cases
// that divide share one division (numerator 1 for the face case): the same operations on the same values as the definition.
__device__ __forceinline__ float point_triangle2(float px, float py, float pz, const float4 t0, const float4 e1, const float4 e2,
                                                 float& u_out, float& v_out)
{
    const float apx = px - t0.x, apy = py - t0.y, apz = pz - t0.z;
    const float d1 = dot3(e1.x, e1.y, e1.z, apx, apy, apz), d2 = dot3(e2.x, e2.y, e2.z, apx, apy, apz);
    const float a11 = dot3(e1.x, e1.y, e1.z, e1.x, e1.y, e1.z), a12 = dot3(e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
    const float a22 = dot3(e2.x, e2.y, e2.z, e2.x, e2.y, e2.z);
    const float d3 = d1 - a11, d4 = d2 - a12, d5 = d1 - a12, d6 = d2 - a22;
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    float u, v;
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; }                          // vertex a
    else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; }                       // vertex b
    else {
        const bool ab = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
        const bool cc = !ab && d6 >= 0.0f && d5 <= d6;
        const bool ac = !ab && !cc && vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
        const bool bc = !ab && !cc && !ac && va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f;
        const float num = ab ? d1 : (ac ? d2 : (bc ? d43 : 1.0f));
        const float den = ab ? d1 - d3 : (ac ? d2 - d6 : (bc ? d43 + d56 : (va + vb) + vc));
        const float q = num / den;
        if (ab) { u = q; v = 0.0f; }
        else if (cc) { u = 0.0f; v = 1.0f; }                                       // vertex c
        else if (ac) { u = 0.0f; v = q; }
        else if (bc) { u = 1.0f - q; v = q; }
        else { u = vb * q; v = vc * q; }                                           // face
    }
    const float rx = apx - (e1.x * u + e2.x * v), ry = apy - (e1.y * u + e2.y * v), rz = apz - (e1.z * u + e2.z * v);
    u_out = u;
    v_out = v;
    return dot3(rx, ry, rz, rx, ry, rz);
}

// query k into the lane (best = R): false (none-record / 0 written, lane stays idle) for an inactive query, and for a point
// with a NaN coordinate, whose every dist2 is NaN: no candidate by definition, but its box distances would all read 0
template <bool ANY>
__device__ __forceinline__ bool load_point_query(const lbvh_point_query* __restrict__ queries, uint32_t k, float& px, float& py, float& pz,
                                                 float& best, std::conditional_t<ANY, uint32_t, lbvh_closest_point>* __restrict__ out)
{
    const float4 q = reinterpret_cast<const float4*>(queries)[k];
    px = q.x; py = q.y; pz = q.z;
    best = fminf(q.w, LBVH_MAX_FLOAT);
    if (q.w > 0.0f && (q.x == q.x && q.y == q.y && q.z == q.z)) return true;      // false for a NaN radius too
    if constexpr (ANY) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
    return false;
}

// One query per lane over the four-wide nodes, in the frame of trace_rays_wide_kernel<PLAIN> (persistent waves, lanes refilled from
// the wave's run of consecutive queries, LDS + device-memory stack).  Per step one node line: four box distances, slots beyond
// `best` dropped, leaf slots tested, the other slots entered nearest first.  A candidate is a triangle with dist2 < R that is not
// in front of its own box (!(dist2 < box2 of its leaf slot)): box2 grows from a box to any box inside it, so a subtree skipped
// because box2 > best holds no candidate at or below best and the record does not depend on the order of the walk.
// ANY: a flag, the walk cut off at its first candidate (best stays R).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void point_query_wide_kernel(const lbvh_point_query* __restrict__ queries, uint32_t total,
                                                              const lbvh_wide_node* __restrict__ wide,
                                                              const lbvh_fast_node* __restrict__ lines,
                                                              std::conditional_t<ANY, uint32_t, lbvh_closest_point>* __restrict__ out,
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

    bool active = false, took = false;
    uint32_t i = 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    float best = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_point_query<ANY>(queries, k, px, py, pz, best, out);
                    best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_queries++;
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
            const float b0 = point_box2(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, px, py, pz);
            const float b1 = point_box2(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, px, py, pz);
            const float b2 = point_box2(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, px, py, pz);
            const float b3 = point_box2(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, px, py, pz);
            const bool h0 = !(b0 > best) && ref.x != kWideEmpty, h1 = !(b1 > best) && ref.y != kWideEmpty;
            const bool h2 = !(b2 > best) && ref.z != kWideEmpty, h3 = !(b3 > best) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                float u = 0.0f, v = 0.0f;
                const float dist2 = point_triangle2(px, py, pz, v0, v1, v2, u, v);
                const uint32_t tri = __float_as_uint(v0.w);
                const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                // best starts at R and best_tri at 0: dist2 == R is never taken.  Ties go to the lower triangle index.
                if (!(dist2 < own) && (dist2 < best || (dist2 == best && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else { best = dist2; best_tri = tri; best_u = u; best_v = v; took = true; }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by box distance: the order key is the distance's bit pattern (non-negative floats order
            // like integers) with the slot number in its two lowest bits.  (`best` may have shrunk in the leaf loop since h0 .. h3
            // were formed: the box distances are compared with it once more)
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(b0 > best) ? ((__float_as_uint(b0) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(b1 > best) ? ((__float_as_uint(b1) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(b2 > best) ? ((__float_as_uint(b2) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(b3 > best) ? ((__float_as_uint(b3) & ~3u) | 3u) : none;
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
                if constexpr (ANY) out[i] = 0u;
                else reinterpret_cast<float4*>(out)[i] = make_float4(took ? best : LBVH_MAX_FLOAT, __uint_as_float(best_tri), best_u, best_v);
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- sphere casts: first contact of a moving sphere (include/lbvh.h, lbvh_sphere_cast) ---------------------------------
// The time at which the sphere of radius r whose centre moves along the ray touches the triangle {a, e1, e2} of a derived-scene
// line, +inf if it never does: the features of lbvh.h in its order (start overlap, face, three edges, three vertices), a later
// one taken only when strictly less, every operation the header's.  m = origin - P, dot(m, d) and dot(m, m) are formed once per
// vertex and serve its edge and its vertex sphere; a11 / a12 / a22 are point_triangle2's (the same expressions: the compiler
// forms them once); each quadratic divides once.
__device__ __forceinline__ float sphere_triangle_time(const ray_t& c, float r, const float4 a, const float4 e1, const float4 e2)
{
    const float inf = __builtin_inff();
    const float R2 = r * r, dd = dot3(c.dx, c.dy, c.dz, c.dx, c.dy, c.dz);
    float u0, v0;
    if (point_triangle2(c.ox, c.oy, c.oz, a, e1, e2, u0, v0) <= R2) return 0.0f;
    float t = inf;
    auto take = [&](bool valid, float cand) { if (valid && cand >= 0.0f && cand < t) t = cand; };
    const float a11 = dot3(e1.x, e1.y, e1.z, e1.x, e1.y, e1.z), a12 = dot3(e1.x, e1.y, e1.z, e2.x, e2.y, e2.z);
    const float a22 = dot3(e2.x, e2.y, e2.z, e2.x, e2.y, e2.z);
    const float max_ = c.ox - a.x, may = c.oy - a.y, maz = c.oz - a.z;
    {   // face
        const float nx = e1.y * e2.z - e1.z * e2.y, ny = e1.z * e2.x - e1.x * e2.z, nz = e1.x * e2.y - e1.y * e2.x;
        const float h = r * sqrtf(dot3(nx, ny, nz, nx, ny, nz));
        float s = dot3(max_, may, maz, nx, ny, nz), dn = dot3(c.dx, c.dy, c.dz, nx, ny, nz);
        const float sg = s >= 0.0f ? 1.0f : -1.0f;
        s = s * sg;
        dn = dn * sg;
        const float tf = (h - s) / dn;
        const float qx = (c.ox + c.dx * tf) - a.x, qy = (c.oy + c.dy * tf) - a.y, qz = (c.oz + c.dz * tf) - a.z;
        const float d1 = dot3(e1.x, e1.y, e1.z, qx, qy, qz), d2 = dot3(e2.x, e2.y, e2.z, qx, qy, qz);
        const float det = a11 * a22 - a12 * a12;
        const float u = (a22 * d1 - a12 * d2) / det, v = (a11 * d2 - a12 * d1) / det;
        take(s > h && dn < 0.0f && u >= 0.0f && v >= 0.0f && u + v <= 1.0f, tf);
    }
    const float bx = a.x + e1.x, by = a.y + e1.y, bz = a.z + e1.z;
    const float cx = a.x + e2.x, cy = a.y + e2.y, cz = a.z + e2.z;
    const float e3x = e2.x - e1.x, e3y = e2.y - e1.y, e3z = e2.z - e1.z;
    const float mbx = c.ox - bx, mby = c.oy - by, mbz = c.oz - bz;
    const float mcx = c.ox - cx, mcy = c.oy - cy, mcz = c.oz - cz;
    const float mda = dot3(max_, may, maz, c.dx, c.dy, c.dz), mma = dot3(max_, may, maz, max_, may, maz);
    const float mdb = dot3(mbx, mby, mbz, c.dx, c.dy, c.dz), mmb = dot3(mbx, mby, mbz, mbx, mby, mbz);
    const float mdc = dot3(mcx, mcy, mcz, c.dx, c.dy, c.dz), mmc = dot3(mcx, mcy, mcz, mcx, mcy, mcz);
    auto edge = [&](float mx, float my, float mz, float md, float mm, float ex, float ey, float ez, float ee) {
        const float me = dot3(mx, my, mz, ex, ey, ez), de = dot3(c.dx, c.dy, c.dz, ex, ey, ez);
        const float A = ee * dd - de * de;
        const float B = ee * md - de * me;
        const float Cq = ee * (mm - R2) - me * me;
        const float disc = B * B - A * Cq;
        const float te = (-B - sqrtf(disc)) / A;
        const float se = me + te * de;
        take(A > 0.0f && disc >= 0.0f && 0.0f <= se && se <= ee, te);
    };
    edge(max_, may, maz, mda, mma, e1.x, e1.y, e1.z, a11);
    edge(max_, may, maz, mda, mma, e2.x, e2.y, e2.z, a22);
    edge(mbx, mby, mbz, mdb, mmb, e3x, e3y, e3z, dot3(e3x, e3y, e3z, e3x, e3y, e3z));
    auto vertex = [&](float B, float mm) {
        const float Cq = mm - R2;
        const float disc = B * B - dd * Cq;
        take(disc >= 0.0f, (-B - sqrtf(disc)) / dd);
    };
    vertex(mda, mma);
    vertex(mdb, mmb);
    vertex(mdc, mmc);
    return t;
}

// cast k into the lane (best_t = T): false (miss record / 0 written, lane stays idle) for an inactive cast.  !RECORD (the cast-all
// walk, whose inactive casts have an empty segment): nothing is written and `out` is not read
template <bool ANY, bool RECORD = true>
__device__ __forceinline__ bool load_sphere_cast(const lbvh_sphere_ray* __restrict__ casts, uint32_t k, ray_t& ray, float& r, float& best_t,
                                                 std::conditional_t<ANY, uint32_t, lbvh_hit>* __restrict__ out)
{
    const float inf = __builtin_inff();
    const float4* q = reinterpret_cast<const float4*>(&casts[k]);
    const float4 o = q[0], d = q[1];
    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
    r = o.w;
    best_t = fminf(d.w, LBVH_MAX_FLOAT);                 // T: candidates have t < T
    if (o.w > 0.0f && o.w < inf && d.w > 0.0f && (o.x == o.x && o.y == o.y && o.z == o.z) &&
        fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf && dot3(d.x, d.y, d.z, d.x, d.y, d.z) > 0.0f) return true;
    if constexpr (!RECORD) return false;
    else if constexpr (ANY) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
    return false;
}

// One cast per lane over the four-wide nodes, in the frame of trace_rays_wide_kernel<PLAIN> (persistent waves, lanes refilled from
// the wave's run of consecutive casts, LDS + device-memory stack, leaf slots first, inner slots entered nearest entry first).  The
// four slot boxes are grown by the lane's radius (lo - r, hi + r: monotone, so a grown box contains the grown boxes of everything
// below it) before the slab test; a slot is skipped when the ray misses its grown box or enters it beyond best_t, strictly, never
// on its exit distance.  A candidate is a triangle with a time t < T that is not in front of its own grown box (hit_counts), so
// the record does not depend on the order of the walk.  u and v are point_triangle2's at c(t), formed when a candidate is taken.
// ANY: a flag, the walk cut off at its first candidate (best_t stays T).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void sphere_cast_wide_kernel(const lbvh_sphere_ray* __restrict__ casts, uint32_t total,
                                                              const lbvh_wide_node* __restrict__ wide,
                                                              const lbvh_fast_node* __restrict__ lines,
                                                              std::conditional_t<ANY, uint32_t, lbvh_hit>* __restrict__ out,
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false, took = false;
    uint32_t i = 0;
    ray_t ray = {};
    float r = 0.0f;
    float best_t = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_sphere_cast<ANY>(casts, k, ray, r, best_t, out);
                    best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_casts++;
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
            const bool h0 = wide_box(lox.x - r, loy.x - r, loz.x - r, hix.x + r, hiy.x + r, hiz.x + r, ray, t0) && !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y - r, loy.y - r, loz.y - r, hix.y + r, hiy.y + r, hiz.y + r, ray, t1) && !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z - r, loy.z - r, loz.z - r, hix.z + r, hiy.z + r, hiz.z + r, ray, t2) && !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w - r, loy.w - r, loz.w - r, hix.w + r, hiy.w + r, hiz.w + r, ray, t3) && !(t3 > best_t) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                const float t = sphere_triangle_time(ray, r, v0, v1, v2);
                const uint32_t tri = __float_as_uint(v0.w);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // best_t starts at T and best_tri at 0: t == T is never taken.  Ties go to the lower triangle index.
                if (hit_counts(t, entry) && (t < best_t || (t == best_t && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else {
                        best_t = t; best_tri = tri; took = true;
                        point_triangle2(ray.ox + ray.dx * t, ray.oy + ray.dy * t, ray.oz + ray.dz * t, v0, v1, v2, best_u, best_v);
                    }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by entry distance: the order key is the distance's bit pattern (non-negative floats
            // order like integers) with the slot number in its two lowest bits
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
                if constexpr (ANY) out[i] = 0u;
                else put_hit<true>(out, i, best_t, took, best_tri, best_u, best_v);
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// ---- capsule casts: first contact of a moving capsule (include/lbvh.h, lbvh_capsule_cast) -------------------------------
// A capsule (axis [p, p + h], radius r) touches a triangle exactly when the sphere (p, r) touches the prism "triangle + segment
// [0, -h]", whose surface is eight triangles: the header's derived triangles.  Vertex id 0 .. 5 = A, B, C, A', B', C' of the
// header: A = a, B = a + e1, C = a + e2 and X' = X - h, every one per component in fp32.
__device__ __forceinline__ void capsule_vertex(uint32_t id, const float4 a, const float4 e1, const float4 e2, float hx, float hy, float hz,
                                               float& x, float& y, float& z)
{
    const uint32_t base = id >= 3u ? id - 3u : id;
    const float ex = base == 1u ? e1.x : e2.x, ey = base == 1u ? e1.y : e2.y, ez = base == 1u ? e1.z : e2.z;
    x = base == 0u ? a.x : a.x + ex;
    y = base == 0u ? a.y : a.y + ey;
    z = base == 0u ? a.z : a.z + ez;
    if (id >= 3u) { x = x - hx; y = y - hy; z = z - hz; }
}

// derived triangle j of the header as {P, Q - P, R - P}; j = 0 is the line as stored.  One nibble per j and corner:
// (P, Q, R) = (A, B, C) (A', B', C') (A, B, A') (B', A', B) (B, C, B') (C', B', C) (C, A, C') (A', C', A)
__device__ __forceinline__ void capsule_triangle(uint32_t j, const float4 a, const float4 e1, const float4 e2, float hx, float hy, float hz,
                                                 float4& p, float4& q1, float4& q2)
{
    const uint32_t sh = 4u * j;
    float px, py, pz, qx, qy, qz, rx, ry, rz;
    capsule_vertex((0x32514030u >> sh) & 7u, a, e1, e2, hx, hy, hz, px, py, pz);
    capsule_vertex((0x50423141u >> sh) & 7u, a, e1, e2, hx, hy, hz, qx, qy, qz);
    capsule_vertex((0x05241352u >> sh) & 7u, a, e1, e2, hx, hy, hz, rx, ry, rz);
    const bool own = j == 0u;
    p = make_float4(px, py, pz, 0.0f);
    q1 = make_float4(own ? e1.x : qx - px, own ? e1.y : qy - py, own ? e1.z : qz - pz, 0.0f);
    q2 = make_float4(own ? e2.x : rx - px, own ? e2.y : ry - py, own ? e2.z : rz - pz, 0.0f);
}

// The header's time of a capsule with one scene triangle, +inf if it has none: the least sphere_triangle_time over the derived
// triangles j = 0 .. 7 in that order, a later one taken only when strictly less (so the loop may stop at the first zero), then the
// pierce of the axis through the face.  `which` = the winning j, 8 for the pierce, whose parameter is `t_p`.  One copy of the
// sphere test in a loop that is not unrolled, the corners selected by j: eight inlined copies do not fit the register file.
__device__ __forceinline__ float capsule_triangle_time(const ray_t& c, float r, float hx, float hy, float hz, const float4 a, const float4 e1,
                                                       const float4 e2, uint32_t& which, float& t_p)
{
    float t = __builtin_inff();
    which = 0u;
#pragma nounroll
    for (uint32_t j = 0; j < 8u; j++) {
        float4 p, q1, q2;
        capsule_triangle(j, a, e1, e2, hx, hy, hz, p, q1, q2);
        const float tj = sphere_triangle_time(c, r, p, q1, q2);
        if (tj < t) { t = tj; which = j; }
        if (t == 0.0f) return t;
    }
    ray_t ax;
    ax.ox = c.ox; ax.oy = c.oy; ax.oz = c.oz;
    ax.dx = hx; ax.dy = hy; ax.dz = hz;
    ax.ix = 0.0f; ax.iy = 0.0f; ax.iz = 0.0f;            // (not read by the triangle test)
    float u = 0.0f, v = 0.0f;
    const float tp = ray_triangle_edges(ax, a, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, u, v);
    if (0.0f <= tp && tp <= 1.0f) { t = 0.0f; which = 8u; t_p = tp; }
    return t;
}

// (u, v) of a taken candidate: s, the axis parameter of the touching point, from point_triangle2 at c(t) on the winning derived
// triangle (0 on the triangle itself, 1 on its shifted copy, v' or 1 - v' on a side, t_p for the pierce), then point_triangle2 of
// c(t) + h*s on the scene triangle
__device__ __forceinline__ void capsule_contact(const ray_t& c, float t, float hx, float hy, float hz, const float4 a, const float4 e1,
                                                const float4 e2, uint32_t which, float t_p, float& u_out, float& v_out)
{
    const float cx = c.ox + c.dx * t, cy = c.oy + c.dy * t, cz = c.oz + c.dz * t;
    float s = which == 8u ? t_p : (which == 1u ? 1.0f : 0.0f);
    if (which >= 2u && which < 8u) {
        float4 p, q1, q2;
        capsule_triangle(which, a, e1, e2, hx, hy, hz, p, q1, q2);
        float u1, v1;
        point_triangle2(cx, cy, cz, p, q1, q2, u1, v1);
        s = (which & 1u) ? 1.0f - v1 : v1;
    }
    point_triangle2(cx + hx * s, cy + hy * s, cz + hz * s, a, e1, e2, u_out, v_out);
}

// cast k into the lane (best_t = T): false (miss record / 0 written, lane stays idle; !RECORD: nothing written) for an inactive cast
template <bool ANY, bool RECORD = true>
__device__ __forceinline__ bool load_capsule_cast(const lbvh_capsule_ray* __restrict__ casts, uint32_t k, ray_t& ray, float& r, float& hx,
                                                  float& hy, float& hz, float& best_t,
                                                  std::conditional_t<ANY, uint32_t, lbvh_hit>* __restrict__ out)
{
    const float inf = __builtin_inff();
    const float4* q = reinterpret_cast<const float4*>(&casts[k]);
    const float4 o = q[0], d = q[1], h = q[2];
    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
    r = o.w;
    hx = h.x; hy = h.y; hz = h.z;
    best_t = fminf(d.w, LBVH_MAX_FLOAT);                 // T: candidates have t < T
    if (o.w > 0.0f && o.w < inf && d.w > 0.0f && (o.x == o.x && o.y == o.y && o.z == o.z) &&
        fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf && dot3(d.x, d.y, d.z, d.x, d.y, d.z) > 0.0f &&
        fabsf(h.x) < inf && fabsf(h.y) < inf && fabsf(h.z) < inf) return true;
    if constexpr (!RECORD) return false;
    else if constexpr (ANY) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
    return false;
}

// One cast per lane in the frame of sphere_cast_wide_kernel.  The four slot boxes are grown by the sweep of the axis and the radius,
// (lo - max(h, 0)) - r and (hi - min(h, 0)) + r — two operations per bound, both monotone in lo / hi, so a grown box contains the
// grown boxes of everything below it and the record does not depend on the order of the walk, as there.  At a leaf the triangle
// line is read once and the eight derived triangles are formed from it in registers; s, (u', v') and (u, v) only for a candidate
// that is taken.
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void capsule_cast_wide_kernel(const lbvh_capsule_ray* __restrict__ casts, uint32_t total,
                                                               const lbvh_wide_node* __restrict__ wide,
                                                               const lbvh_fast_node* __restrict__ lines,
                                                               std::conditional_t<ANY, uint32_t, lbvh_hit>* __restrict__ out,
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false, took = false;
    uint32_t i = 0;
    ray_t ray = {};
    float r = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;
    float best_t = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_capsule_cast<ANY>(casts, k, ray, r, hx, hy, hz, best_t, out);
                    best_tri = 0; best_u = 0.0f; best_v = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_casts++;
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
            // max(h, 0) and min(h, 0) are formed here from h, which the leaf test needs anyway: held through the walk they are six
            // more registers and the record form drops from four waves per SIMD to three
            const float px = fmaxf(hx, 0.0f), py = fmaxf(hy, 0.0f), pz = fmaxf(hz, 0.0f);
            const float nx = fminf(hx, 0.0f), ny = fminf(hy, 0.0f), nz = fminf(hz, 0.0f);
            float t0, t1, t2, t3;
            const bool h0 = wide_box((lox.x - px) - r, (loy.x - py) - r, (loz.x - pz) - r, (hix.x - nx) + r, (hiy.x - ny) + r, (hiz.x - nz) + r, ray, t0) &&
                            !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box((lox.y - px) - r, (loy.y - py) - r, (loz.y - pz) - r, (hix.y - nx) + r, (hiy.y - ny) + r, (hiz.y - nz) + r, ray, t1) &&
                            !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box((lox.z - px) - r, (loy.z - py) - r, (loz.z - pz) - r, (hix.z - nx) + r, (hiy.z - ny) + r, (hiz.z - nz) + r, ray, t2) &&
                            !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box((lox.w - px) - r, (loy.w - py) - r, (loz.w - pz) - r, (hix.w - nx) + r, (hiy.w - ny) + r, (hiz.w - nz) + r, ray, t3) &&
                            !(t3 > best_t) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                uint32_t which;
                float t_p = 0.0f;
                const float t = capsule_triangle_time(ray, r, hx, hy, hz, v0, v1, v2, which, t_p);
                const uint32_t tri = __float_as_uint(v0.w);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // best_t starts at T and best_tri at 0: t == T is never taken.  Ties go to the lower triangle index.
                if (hit_counts(t, entry) && (t < best_t || (t == best_t && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else {
                        best_t = t; best_tri = tri; took = true;
                        capsule_contact(ray, t, hx, hy, hz, v0, v1, v2, which, t_p, best_u, best_v);
                    }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by entry distance (the order key of sphere_cast_wide_kernel)
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
                if constexpr (ANY) out[i] = 0u;
                else put_hit<true>(out, i, best_t, took, best_tri, best_u, best_v);
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// ---- box casts: first contact of a moving oriented box (include/lbvh.h, lbvh_box_cast) ----------------------------------
// the three half-axis vectors of a cast: the box is { centre + s0*x + s1*y + s2*z : |s_i| <= 1 }
struct box_axes { float xx, xy, xz, yx, yy, yz, zx, zy, zz; };

// The header's time of a box with one scene triangle, +inf if it has none: the swept separating-axis test over the thirteen axes
// L_j = cross(P_j, Q_j) in the header's order, `axis` = the j that set the time (LBVH_BOX_AXIS_START: overlapping at the start).
// One copy of the axis body in a loop that is not unrolled, P_j and Q_j picked by j from a nibble table (j is the same in every
// lane: the picks are selects on a scalar condition).  P: 0 1 2 = the box's x y z, 3 = e1; Q: the same and 4 = e2, 5 = e2 - e1.
// The loop leaves as soon as enter > exit or enter > bound.  Neither changes a record: enter only grows and exit only shrinks
// from axis to axis (a value replaces them only through a strict comparison, so neither is ever a NaN), hence enter > exit after
// some axis is enter > exit after all thirteen, no time; and a time is the final enter >= this enter > bound, where bound is the
// lane's best_t (T until a candidate is taken), which the candidate test t < best_t || (t == best_t && ...) refuses.
// Axis j of the header, L = cross(P_j, Q_j), and on it the triangle's interval [lo, hi] from the box's centre (m = a - centre,
// e3 = e2 - e1) and the box's half width rb: the part of the axis body that lbvh_box_cast and lbvh_obb_overlaps share.
__device__ __forceinline__ void box_axis_spans(uint32_t j, float mx, float my, float mz, const box_axes& b, const float4 e1, const float4 e2,
                                               float e3x, float e3y, float e3z, float& lx, float& ly, float& lz, float& lo, float& hi, float& rb)
{
    const uint32_t pi = (uint32_t)(0x2221110000213ull >> (4u * j)) & 7u;
    const uint32_t qi = (uint32_t)(0x5435435431024ull >> (4u * j)) & 7u;
    const float px = pi == 0u ? b.xx : (pi == 1u ? b.yx : (pi == 2u ? b.zx : e1.x));
    const float py = pi == 0u ? b.xy : (pi == 1u ? b.yy : (pi == 2u ? b.zy : e1.y));
    const float pz = pi == 0u ? b.xz : (pi == 1u ? b.yz : (pi == 2u ? b.zz : e1.z));
    const float qx = qi == 0u ? b.xx : (qi == 1u ? b.yx : (qi == 2u ? b.zx : (qi == 3u ? e1.x : (qi == 4u ? e2.x : e3x))));
    const float qy = qi == 0u ? b.xy : (qi == 1u ? b.yy : (qi == 2u ? b.zy : (qi == 3u ? e1.y : (qi == 4u ? e2.y : e3y))));
    const float qz = qi == 0u ? b.xz : (qi == 1u ? b.yz : (qi == 2u ? b.zz : (qi == 3u ? e1.z : (qi == 4u ? e2.z : e3z))));
    lx = py * qz - pz * qy; ly = pz * qx - px * qz; lz = px * qy - py * qx;
    const float p0 = dot3(mx, my, mz, lx, ly, lz);
    const float p1 = p0 + dot3(e1.x, e1.y, e1.z, lx, ly, lz), p2 = p0 + dot3(e2.x, e2.y, e2.z, lx, ly, lz);
    lo = fminf(p0, fminf(p1, p2)); hi = fmaxf(p0, fmaxf(p1, p2));
    rb = (fabsf(dot3(b.xx, b.xy, b.xz, lx, ly, lz)) + fabsf(dot3(b.yx, b.yy, b.yz, lx, ly, lz))) +
         fabsf(dot3(b.zx, b.zy, b.zz, lx, ly, lz));
}

__device__ __forceinline__ float box_triangle_time(const ray_t& c, const box_axes& b, const float4 a, const float4 e1, const float4 e2,
                                                   float bound, uint32_t& axis)
{
    const float inf = __builtin_inff();
    const float mx = a.x - c.ox, my = a.y - c.oy, mz = a.z - c.oz;
    const float e3x = e2.x - e1.x, e3y = e2.y - e1.y, e3z = e2.z - e1.z;
    float enter = 0.0f, exit = inf;
    axis = LBVH_BOX_AXIS_START;
#pragma nounroll
    for (uint32_t j = 0; j < 13u; j++) {
        float lx, ly, lz, lo, hi, rb;
        box_axis_spans(j, mx, my, mz, b, e1, e2, e3x, e3y, e3z, lx, ly, lz, lo, hi, rb);
        const float v = dot3(c.dx, c.dy, c.dz, lx, ly, lz);
        const float under = lo - rb, over = hi + rb;
        if (v > 0.0f || v < 0.0f) {
            const float tin = (v > 0.0f ? under : over) / v, tout = (v > 0.0f ? over : under) / v;
            if (tin > enter) { enter = tin; axis = j; }
            if (tout < exit) exit = tout;
        } else if (!(lo <= rb && -rb <= hi)) return inf;     // v = 0 (or a NaN): apart on this axis for ever
        if (enter > exit || enter > bound) return inf;
    }
    return enter;
}

// cast k into the lane (best_t = T): false (miss record / 0 written, lane stays idle; !RECORD: nothing written) for an inactive cast
template <bool ANY, bool RECORD = true>
__device__ __forceinline__ bool load_box_cast(const lbvh_box_ray* __restrict__ casts, uint32_t k, ray_t& ray, box_axes& b, float& best_t,
                                              std::conditional_t<ANY, uint32_t, lbvh_box_hit>* __restrict__ out)
{
    const float inf = __builtin_inff();
    const float4* q = reinterpret_cast<const float4*>(&casts[k]);
    const float4 o = q[0], d = q[1], x = q[2], y = q[3], z = q[4];
    ray.ox = o.x; ray.oy = o.y; ray.oz = o.z;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
    b.xx = x.x; b.xy = x.y; b.xz = x.z;
    b.yx = y.x; b.yy = y.y; b.yz = y.z;
    b.zx = z.x; b.zy = z.y; b.zz = z.z;
    best_t = fminf(o.w, LBVH_MAX_FLOAT);                 // T: candidates have t < T
    const float det = dot3(x.x, x.y, x.z, y.y * z.z - y.z * z.y, y.z * z.x - y.x * z.z, y.x * z.y - y.y * z.x);
    if (o.w > 0.0f && (o.x == o.x && o.y == o.y && o.z == o.z) &&
        fabsf(d.x) < inf && fabsf(d.y) < inf && fabsf(d.z) < inf && dot3(d.x, d.y, d.z, d.x, d.y, d.z) > 0.0f &&
        fabsf(x.x) < inf && fabsf(x.y) < inf && fabsf(x.z) < inf && fabsf(y.x) < inf && fabsf(y.y) < inf && fabsf(y.z) < inf &&
        fabsf(z.x) < inf && fabsf(z.y) < inf && fabsf(z.z) < inf && fabsf(det) < inf && det != 0.0f) return true;
    if constexpr (!RECORD) return false;
    else if constexpr (ANY) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), __uint_as_float(0u), __uint_as_float(0u));
    return false;
}

// One cast per lane in the frame of capsule_cast_wide_kernel.  The four slot boxes are grown by g, the half extent of the cast's
// box along each world axis ((|x_k| + |y_k|) + |z_k|): lo - g and hi + g, one operation per bound and monotone in lo / hi, so a
// grown box contains the grown boxes of everything below it and the record does not depend on the order of the walk, as there.
// A slot is skipped when the ray of the centre misses its grown box or enters it beyond best_t, strictly, never on an exit
// distance.  The record is {t, tri, axis, 0}; ANY: a flag, the walk cut off at its first candidate (best_t stays T).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void box_cast_wide_kernel(const lbvh_box_ray* __restrict__ casts, uint32_t total,
                                                           const lbvh_wide_node* __restrict__ wide,
                                                           const lbvh_fast_node* __restrict__ lines,
                                                           std::conditional_t<ANY, uint32_t, lbvh_box_hit>* __restrict__ out,
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false, took = false;
    uint32_t i = 0;
    ray_t ray = {};
    box_axes b = {};
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    float best_t = LBVH_MAX_FLOAT;
    uint32_t best_tri = 0, best_axis = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_box_cast<ANY>(casts, k, ray, b, best_t, out);
                    gx = (fabsf(b.xx) + fabsf(b.yx)) + fabsf(b.zx);
                    gy = (fabsf(b.xy) + fabsf(b.yy)) + fabsf(b.zy);
                    gz = (fabsf(b.xz) + fabsf(b.yz)) + fabsf(b.zz);
                    best_tri = 0; best_axis = 0; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_casts++;
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
            const bool h0 = wide_box(lox.x - gx, loy.x - gy, loz.x - gz, hix.x + gx, hiy.x + gy, hiz.x + gz, ray, t0) && !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y - gx, loy.y - gy, loz.y - gz, hix.y + gx, hiy.y + gy, hiz.y + gz, ray, t1) && !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z - gx, loy.z - gy, loz.z - gz, hix.z + gx, hiy.z + gy, hiz.z + gz, ray, t2) && !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w - gx, loy.w - gy, loz.w - gz, hix.w + gx, hiy.w + gy, hiz.w + gz, ray, t3) && !(t3 > best_t) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                uint32_t axis;
                const float t = box_triangle_time(ray, b, v0, v1, v2, best_t, axis);
                const uint32_t tri = __float_as_uint(v0.w);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // best_t starts at T and best_tri at 0: t == T is never taken.  Ties go to the lower triangle index.
                if (hit_counts(t, entry) && (t < best_t || (t == best_t && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else { best_t = t; best_tri = tri; best_axis = axis; took = true; }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by entry distance (the order key of sphere_cast_wide_kernel)
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(t0 > best_t) ? ((__float_as_uint(fmaxf(t0, 0.0f)) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(t1 > best_t) ? ((__float_as_uint(fmaxf(t1, 0.0f)) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(t2 > best_t) ? ((__float_as_uint(fmaxf(t2, 0.0f)) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(t3 > best_t) ? ((__float_as_uint(fmaxf(t3, 0.0f)) & ~3u) | 3u) : none;
            {   // five compare-exchanges
                uint32_t a, c;
                a = min(k0, k1); c = max(k0, k1); k0 = a; k1 = c;
                a = min(k2, k3); c = max(k2, k3); k2 = a; k3 = c;
                a = min(k0, k2); c = max(k0, k2); k0 = a; k2 = c;
                a = min(k1, k3); c = max(k1, k3); k1 = a; k3 = c;
                a = min(k1, k2); c = max(k1, k2); k1 = a; k2 = c;
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
                if constexpr (ANY) out[i] = 0u;
                else reinterpret_cast<float4*>(out)[i] = make_float4(took ? best_t : LBVH_MAX_FLOAT, __uint_as_float(best_tri),
                                                                     __uint_as_float(best_axis), __uint_as_float(0u));
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// lbvh_k_closest_points: the walk of point_query_wide_kernel<false> with "best so far" replaced by "k-th best so far".  Each lane
// keeps the k best candidates met so far, sorted by (dist2, tri), in LDS: three arrays [slot][lane] of dist2, triangle index and
// the index of the triangle's line in the derived scene — 12 bytes per slot, `cap` slots per lane, sized at the launch from k
// (dynamic LDS: 768 * k bytes per wave), so a wave's access to one slot touches 64 consecutive words and a small k keeps the
// occupancy of the plain walk.  `best` / `best_tri` are the pruning bound: (R, 0) while fewer than k are held — the state the plain
// walk starts in —, then the list's last entry; a leaf is taken by the plain walk's own comparison against them and inserted by
// shifting the entries that sort after it.  With k = 1 every decision is the plain walk's.  u and v are not carried: when the walk
// of a query ends, point_triangle2 is evaluated once more on the stored line of each survivor — the same operations on the same
// values, hence the same words — and the row is written, padded with none-records.
template <bool STATS>
__global__ __launch_bounds__(64) void k_closest_wide_kernel(const lbvh_point_query* __restrict__ queries, uint32_t total, uint32_t cap,
                                                            const lbvh_wide_node* __restrict__ wide,
                                                            const lbvh_fast_node* __restrict__ lines,
                                                            lbvh_closest_point* __restrict__ out,      // [total][cap]
                                                            uint32_t* __restrict__ found_out,          // [total] or nullptr
                                                            uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                            uint32_t lds_depth,              // <= kWideStackLds
                                                            uint32_t deep_cap,               // <= kWideStackDeep
                                                            uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    extern __shared__ uint32_t s_list[];                 // [3][cap][64]: dist2 bits | triangle index | line index
    const uint32_t lane = threadIdx.x;
    uint32_t* const l_dist = s_list + lane;
    uint32_t* const l_tri = l_dist + cap * LBVH_WAVE;
    uint32_t* const l_line = l_tri + cap * LBVH_WAVE;
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;
    const float4 none_record = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);

    bool active = false;
    uint32_t i = 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    float best = LBVH_MAX_FLOAT;
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
                    const float4 q = reinterpret_cast<const float4*>(queries)[k];
                    px = q.x; py = q.y; pz = q.z;
                    best = fminf(q.w, LBVH_MAX_FLOAT);
                    best_tri = 0; held = 0; sp = 0; node = 0;
                    active = q.w > 0.0f && (q.x == q.x && q.y == q.y && q.z == q.z);      // load_point_query's rule
                    if (!active) {                       // no candidates, no walk: the whole row is none-records
                        float4* row = reinterpret_cast<float4*>(out) + (size_t)k * cap;
                        for (uint32_t j = 0; j < cap; j++) row[j] = none_record;
                        if (found_out) found_out[k] = 0u;
                    }
                    if (STATS && active) n_queries++;
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
            const float b0 = point_box2(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, px, py, pz);
            const float b1 = point_box2(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, px, py, pz);
            const float b2 = point_box2(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, px, py, pz);
            const float b3 = point_box2(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, px, py, pz);
            const bool h0 = !(b0 > best) && ref.x != kWideEmpty, h1 = !(b1 > best) && ref.y != kWideEmpty;
            const bool h2 = !(b2 > best) && ref.z != kWideEmpty, h3 = !(b3 > best) && ref.w != kWideEmpty;
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
                const float dist2 = point_triangle2(px, py, pz, v0, v1, v2, u, v);
                const uint32_t tri = __float_as_uint(v0.w);
                const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                // (best, best_tri) is (R, 0) until k are held: dist2 == R is never taken.  Then it is the k-th held: the candidate
                // must sort before it, ties by the lower triangle index
                if (!(dist2 < own) && (dist2 < best || (dist2 == best && tri < best_tri))) {
                    uint32_t j = min(held, cap - 1u);    // the slot that becomes free: the end of the list, or its dropped last entry
                    while (j != 0u) {
                        const float dj = __uint_as_float(l_dist[(j - 1u) * LBVH_WAVE]);
                        const uint32_t tj = l_tri[(j - 1u) * LBVH_WAVE];
                        if (!(dist2 < dj || (dist2 == dj && tri < tj))) break;
                        l_dist[j * LBVH_WAVE] = __float_as_uint(dj);
                        l_tri[j * LBVH_WAVE] = tj;
                        l_line[j * LBVH_WAVE] = l_line[(j - 1u) * LBVH_WAVE];
                        j--;
                    }
                    l_dist[j * LBVH_WAVE] = __float_as_uint(dist2);
                    l_tri[j * LBVH_WAVE] = tri;
                    l_line[j * LBVH_WAVE] = line;
                    held = min(held + 1u, cap);
                    if (held == cap) {
                        best = __uint_as_float(l_dist[(cap - 1u) * LBVH_WAVE]);
                        best_tri = l_tri[(cap - 1u) * LBVH_WAVE];
                    }
                }
            }
            // nodes to enter, ordered by box distance: the order key is the distance's bit pattern (non-negative floats order
            // like integers) with the slot number in its two lowest bits.  (`best` may have shrunk in the leaf loop since h0 .. h3
            // were formed: the box distances are compared with it once more)
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(b0 > best) ? ((__float_as_uint(b0) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(b1 > best) ? ((__float_as_uint(b1) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(b2 > best) ? ((__float_as_uint(b2) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(b3 > best) ? ((__float_as_uint(b3) & ~3u) | 3u) : none;
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
                // the row: the survivors in order, u and v from their lines again, then none-records
                float4* row = reinterpret_cast<float4*>(out) + (size_t)i * cap;
                for (uint32_t j = 0; j < held; j++) {
                    float4 v0, v1, v2;
                    unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[l_line[j * LBVH_WAVE]]), v0, v1, v2);
                    float u = 0.0f, v = 0.0f;
                    const float dist2 = point_triangle2(px, py, pz, v0, v1, v2, u, v);
                    row[j] = make_float4(dist2, v0.w, u, v);
                }
                for (uint32_t j = held; j < cap; j++) row[j] = none_record;
                if (found_out) found_out[i] = held;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- overlap queries: every triangle in a box / within a distance, as a CSR list (include/lbvh.h) -----------------------
// The first queries whose output length is not known at the call: a COUNT walk writes one 32-bit count per query into the ray
// scratch, three small kernels scan the counts into the caller's 64-bit offsets, and a FILL walk — the same kernel, the same
// decisions — stores candidate j of query k at offsets[k] + j while that is below the capacity.
//   BOX:  the query is an lbvh_aabb; a slot is entered iff the two boxes overlap (closed intervals, six comparisons, nothing to
//         round).  A leaf slot's box is the triangle's own AABB and its reference is LEAF | leaf_base + ORIGINAL index
//         (lbvh_build.hip tree_body), so a candidate costs no triangle line at all.
//   !BOX: the query is an lbvh_point_query; the walk of point_query_wide_kernel with the bound fixed at R: slots with box2 > R are
//         skipped, a leaf is a candidate iff dist2 < R && !(dist2 < box2 of its slot) — lbvh_within_distance's predicate.
// Nothing shrinks, so the slots need no order: the first passing inner slot is entered, the others wait on the stack.
__device__ __forceinline__ bool point_query_active(const float4 q) { return q.w > 0.0f && (q.x == q.x && q.y == q.y && q.z == q.z); }

// query k into the lane: BOX (ax, ay, az) = min, (bx, by, bz) = max; !BOX (ax, ay, az) = p, bx = R.  false: no candidates, no walk
template <bool BOX>
__device__ __forceinline__ bool load_overlap_query(const float4* __restrict__ queries, uint32_t k, float& ax, float& ay, float& az,
                                                   float& bx, float& by, float& bz)
{
    if constexpr (BOX) {
        const float4 lo = queries[2 * (size_t)k], hi = queries[2 * (size_t)k + 1];
        ax = lo.x; ay = lo.y; az = lo.z;
        bx = hi.x; by = hi.y; bz = hi.z;
        return ax <= bx && ay <= by && az <= bz;             // false when a bound is NaN
    } else {
        const float4 q = queries[k];
        ax = q.x; ay = q.y; az = q.z;
        bx = fminf(q.w, LBVH_MAX_FLOAT); by = 0.0f; bz = 0.0f;
        return point_query_active(q);
    }
}

__device__ __forceinline__ bool boxes_overlap(float qlx, float qly, float qlz, float qhx, float qhy, float qhz,
                                              float lx, float ly, float lz, float hx, float hy, float hz)
{
    return qlx <= hx && lx <= qhx && qly <= hy && ly <= qhy && qlz <= hz && lz <= qhz;
}

template <bool BOX, bool FILL, bool STATS>
__global__ __launch_bounds__(64) void overlap_wide_kernel(const float4* __restrict__ queries, uint32_t total,
                                                          const lbvh_wide_node* __restrict__ wide,
                                                          const lbvh_fast_node* __restrict__ lines, uint32_t leaf_base,
                                                          uint32_t* __restrict__ counts,            // !FILL: candidates of query k
                                                          const uint64_t* __restrict__ offsets,     // FILL: where segment k starts
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
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // FILL: where this lane's next candidate goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    auto emit = [&](uint32_t tri) {
        if constexpr (FILL) {
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
                    active = load_overlap_query<BOX>(queries, k, ax, ay, az, bx, by, bz);
                    sp = 0; node = 0;
                    if constexpr (FILL) { if (active) pos = offsets[k]; }
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_queries++;
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
            bool h0, h1, h2, h3;
            float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;
            if constexpr (BOX) {
                h0 = boxes_overlap(ax, ay, az, bx, by, bz, lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x) && ref.x != kWideEmpty;
                h1 = boxes_overlap(ax, ay, az, bx, by, bz, lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y) && ref.y != kWideEmpty;
                h2 = boxes_overlap(ax, ay, az, bx, by, bz, lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z) && ref.z != kWideEmpty;
                h3 = boxes_overlap(ax, ay, az, bx, by, bz, lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w) && ref.w != kWideEmpty;
            } else {
                b0 = point_box2(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, ax, ay, az);
                b1 = point_box2(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, ax, ay, az);
                b2 = point_box2(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, ax, ay, az);
                b3 = point_box2(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, ax, ay, az);
                h0 = !(b0 > bx) && ref.x != kWideEmpty; h1 = !(b1 > bx) && ref.y != kWideEmpty;
                h2 = !(b2 > bx) && ref.z != kWideEmpty; h3 = !(b3 > bx) && ref.w != kWideEmpty;
            }
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                if constexpr (BOX) {
                    emit(line - leaf_base);
                } else {
                    float4 v0, v1, v2;
                    unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), v0, v1, v2);
                    float u = 0.0f, v = 0.0f;
                    const float dist2 = point_triangle2(ax, ay, az, v0, v1, v2, u, v);
                    const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                    if (dist2 < bx && !(dist2 < own)) emit(__float_as_uint(v0.w));
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
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- every contact of a sweep as a CSR list (lbvh_sphere_cast_all / lbvh_capsule_cast_all / lbvh_box_cast_all, include/lbvh.h) --
// The frame of gather_hits_wide_kernel (count walk, scan, fill walk: the same kernel, the same decisions; persistent waves, lane
// refill, LDS + device-memory stack, leaf slots first, the first passing inner slot entered and the others pushed) around the
// arithmetic of the three cast kernels: load_*_cast's activity test and T, the shape's own grown-box slab test (the cast kernel's
// expressions, the same operations per bound) against the FIXED bound T, and the shape's time of contact — sphere_triangle_time,
// capsule_triangle_time, box_triangle_time with T where the cast passes its shrinking best_t.  A candidate is what the cast kernel
// accepts while its best is still (T, 0): hit_counts(t, entry) && t < T.  The count walk decides on t and the entry alone; the fill
// walk makes the same decision and forms the rest of the record — u / v by point_triangle2 at c(t) (sphere) or capsule_contact
// (capsule), the axis word (box) — only for an accepted candidate: the float4 the cast would write were that candidate the nearest.
enum cast_shape : int { kCastSphere = 0, kCastCapsule = 1, kCastBox = 2 };
template <int SHAPE>
using cast_ray = std::conditional_t<SHAPE == kCastSphere, lbvh_sphere_ray, std::conditional_t<SHAPE == kCastCapsule, lbvh_capsule_ray, lbvh_box_ray>>;

template <int SHAPE, bool FILL, bool STATS>
__global__ __launch_bounds__(64) void cast_gather_wide_kernel(const cast_ray<SHAPE>* __restrict__ casts, uint32_t total,
                                                              const lbvh_wide_node* __restrict__ wide,
                                                              const lbvh_fast_node* __restrict__ lines,
                                                              uint32_t* __restrict__ counts,            // !FILL: candidates of cast k
                                                              const uint64_t* __restrict__ offsets,     // FILL: where segment k starts
                                                              float4* __restrict__ hits, uint64_t capacity,     // lbvh_hit / lbvh_box_hit records
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t ray = {};
    float r = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;     // sphere: r; capsule: r and the axis
    box_axes b = {};                                     // box: the half-axis vectors and g, the half extent per world axis
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    float T = LBVH_MAX_FLOAT;
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
                    if constexpr (SHAPE == kCastSphere) active = load_sphere_cast<false, false>(casts, k, ray, r, T, nullptr);
                    else if constexpr (SHAPE == kCastCapsule) active = load_capsule_cast<false, false>(casts, k, ray, r, hx, hy, hz, T, nullptr);
                    else {
                        active = load_box_cast<false, false>(casts, k, ray, b, T, nullptr);
                        gx = (fabsf(b.xx) + fabsf(b.yx)) + fabsf(b.zx);
                        gy = (fabsf(b.xy) + fabsf(b.yy)) + fabsf(b.zy);
                        gz = (fabsf(b.xz) + fabsf(b.yz)) + fabsf(b.zz);
                    }
                    sp = 0; node = 0;
                    if constexpr (FILL) { if (active) pos = offsets[k]; }      // (reloaded at every refill: a lane serves many casts)
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_casts++;
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
            // the slab test of one slot's grown box: the expressions of the shape's cast kernel
            auto grown = [&](float lx, float ly, float lz, float ux, float uy, float uz, float& t) {
                if constexpr (SHAPE == kCastSphere) return wide_box(lx - r, ly - r, lz - r, ux + r, uy + r, uz + r, ray, t);
                else if constexpr (SHAPE == kCastCapsule) {
                    // max(h, 0) and min(h, 0) formed here, not held through the walk (capsule_cast_wide_kernel)
                    const float px = fmaxf(hx, 0.0f), py = fmaxf(hy, 0.0f), pz = fmaxf(hz, 0.0f);
                    const float nx = fminf(hx, 0.0f), ny = fminf(hy, 0.0f), nz = fminf(hz, 0.0f);
                    return wide_box((lx - px) - r, (ly - py) - r, (lz - pz) - r, (ux - nx) + r, (uy - ny) + r, (uz - nz) + r, ray, t);
                } else return wide_box(lx - gx, ly - gy, lz - gz, ux + gx, uy + gy, uz + gz, ray, t);
            };
            float t0, t1, t2, t3;
            const bool h0 = grown(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, t0) && !(t0 > T) && ref.x != kWideEmpty;
            const bool h1 = grown(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, t1) && !(t1 > T) && ref.y != kWideEmpty;
            const bool h2 = grown(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, t2) && !(t2 > T) && ref.z != kWideEmpty;
            const bool h3 = grown(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, t3) && !(t3 > T) && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                uint32_t which = 0u;                     // capsule: the winning derived triangle; box: the axis
                float t_p = 0.0f, t;
                if constexpr (SHAPE == kCastSphere) t = sphere_triangle_time(ray, r, v0, v1, v2);
                else if constexpr (SHAPE == kCastCapsule) t = capsule_triangle_time(ray, r, hx, hy, hz, v0, v1, v2, which, t_p);
                else t = box_triangle_time(ray, b, v0, v1, v2, T, which);      // its early out takes the fixed bound
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                if (hit_counts(t, entry) && t < T) {
                    if constexpr (FILL) {
                        if (pos < capacity) {                                   // never at or beyond the capacity
                            float4 rec = make_float4(t, v0.w, __uint_as_float(which), __uint_as_float(0u));
                            if constexpr (SHAPE == kCastSphere)
                                point_triangle2(ray.ox + ray.dx * t, ray.oy + ray.dy * t, ray.oz + ray.dz * t, v0, v1, v2, rec.z, rec.w);
                            else if constexpr (SHAPE == kCastCapsule) capsule_contact(ray, t, hx, hy, hz, v0, v1, v2, which, t_p, rec.z, rec.w);
                            hits[pos] = rec;
                        }
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
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// ---- triangle queries: which scene triangles a triangle intersects (lbvh_triangle_intersections, include/lbvh.h) ----------
// The narrow phase behind lbvh_box_overlaps, in the frame of overlap_wide_kernel<BOX = true>: the query's box is the exact min / max
// of its three vertices, a slot is entered iff the two boxes overlap (the same six comparisons), and at a leaf slot — whose box is
// the triangle's own — the triangle line is read and the pair is a candidate iff one of six ray_triangle_edges calls gives
// 0 <= t <= 1: the three query edges against the scene triangle, then the three scene edges (the edge list of lbvh_sphere_cast)
// against the query triangle, first pass wins.  kTriCount and kTriFill are the two walks of the CSR protocol; kTriAny stops a lane
// at its first candidate.
// Registers: a lane keeps the nine coordinates, the box and `skip` (16 VGPRs) and forms the edge vectors at the leaf — nine
// subtractions per tested triangle against nine more registers held through the whole walk (DESIGN §28 has the counts).  Leaf tests
// are not deferred: a leaf slot is tested where it is met, as in every other walker here.
enum tri_query_mode : int { kTriCount = 0, kTriFill = 1, kTriAny = 2 };

// ray (P, D) against the triangle (v0, e1, e2): ray_triangle_edges as the ray walkers call it, then 0 <= t <= 1 (false for a NaN t
// and for the miss value LBVH_MAX_FLOAT)
__device__ __forceinline__ bool edge_pierces(float px, float py, float pz, float dx, float dy, float dz, const float4 v0, float e1x, float e1y,
                                             float e1z, float e2x, float e2y, float e2z)
{
    ray_t r;
    r.ox = px; r.oy = py; r.oz = pz;
    r.dx = dx; r.dy = dy; r.dz = dz;
    r.ix = 0.0f; r.iy = 0.0f; r.iz = 0.0f;               // (not read by the triangle test)
    float u = 0.0f, v = 0.0f;
    const float t = ray_triangle_edges(r, v0, e1x, e1y, e1z, e2x, e2y, e2z, u, v);
    return 0.0f <= t && t <= 1.0f;
}

// the six edge tests of include/lbvh.h in its order; (ax ..) (bx ..) (cx ..) the query's vertices, (t0, t1, t2) the scene triangle's line
__device__ __forceinline__ bool triangles_pierce(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                 const float4 t0, const float4 t1, const float4 t2)
{
    // One copy of the test in a loop that is not unrolled, its operands selected by j: six inlined copies took 102 - 108 VGPRs
    // (4 waves per SIMD).  j = 0, 1, 2: the ray (a, b - a), (b, c - b), (c, a - c) against (v0, e1, e2); j = 3, 4, 5: the ray
    // (v0, e1), (v0, e2), (v0 + e1, e2 - e1) against (a, b - a, c - a).  Every difference is the one fp32 operation of the header.
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
#pragma nounroll
    for (uint32_t j = 0; j < 6u; j++) {
        const bool query_edge = j < 3u;
        float px, py, pz, dx, dy, dz;
        if (j == 0u) { px = ax; py = ay; pz = az; dx = abx; dy = aby; dz = abz; }
        else if (j == 1u) { px = bx; py = by; pz = bz; dx = cx - bx; dy = cy - by; dz = cz - bz; }
        else if (j == 2u) { px = cx; py = cy; pz = cz; dx = ax - cx; dy = ay - cy; dz = az - cz; }
        else if (j == 3u) { px = t0.x; py = t0.y; pz = t0.z; dx = t1.x; dy = t1.y; dz = t1.z; }
        else if (j == 4u) { px = t0.x; py = t0.y; pz = t0.z; dx = t2.x; dy = t2.y; dz = t2.z; }
        else { px = t0.x + t1.x; py = t0.y + t1.y; pz = t0.z + t1.z; dx = t2.x - t1.x; dy = t2.y - t1.y; dz = t2.z - t1.z; }
        const float4 v = query_edge ? t0 : make_float4(ax, ay, az, 0.0f);
        if (edge_pierces(px, py, pz, dx, dy, dz, v, query_edge ? t1.x : abx, query_edge ? t1.y : aby, query_edge ? t1.z : abz,
                         query_edge ? t2.x : acx, query_edge ? t2.y : acy, query_edge ? t2.z : acz))
            return true;
    }
    return false;
}

template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void triangle_query_wide_kernel(const float4* __restrict__ queries, uint32_t total,     // three float4 per query
                                                                 const lbvh_wide_node* __restrict__ wide,
                                                                 const lbvh_fast_node* __restrict__ lines,
                                                                 uint32_t* __restrict__ counts,            // kTriCount: candidates of query k; kTriAny: the flags
                                                                 const uint64_t* __restrict__ offsets,     // kTriFill: where segment k starts
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
    uint32_t i = 0, skip = kWideEmpty;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
    float lx = 0.0f, ly = 0.0f, lz = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;      // the query's box
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // kTriFill: where this lane's next candidate goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float inf = __builtin_inff();
                    const float4 qa = queries[3 * (size_t)k], qb = queries[3 * (size_t)k + 1], qc = queries[3 * (size_t)k + 2];
                    ax = qa.x; ay = qa.y; az = qa.z; skip = __float_as_uint(qa.w);
                    bx = qb.x; by = qb.y; bz = qb.z;
                    cx = qc.x; cy = qc.y; cz = qc.z;
                    lx = fminf(fminf(ax, bx), cx); ly = fminf(fminf(ay, by), cy); lz = fminf(fminf(az, bz), cz);
                    hx = fmaxf(fmaxf(ax, bx), cx); hy = fmaxf(fmaxf(ay, by), cy); hz = fmaxf(fmaxf(az, bz), cz);
                    active = fabsf(ax) < inf && fabsf(ay) < inf && fabsf(az) < inf && fabsf(bx) < inf && fabsf(by) < inf && fabsf(bz) < inf &&
                             fabsf(cx) < inf && fabsf(cy) < inf && fabsf(cz) < inf;         // all nine finite (false for NaN)
                    sp = 0; node = 0;
                    if constexpr (MODE == kTriFill) { if (active) pos = offsets[k]; }
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_queries++;
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
            const bool h0 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x) && ref.x != kWideEmpty;
            const bool h1 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y) && ref.y != kWideEmpty;
            const bool h2 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z) && ref.z != kWideEmpty;
            const bool h3 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w) && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 t0, t1, t2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
                const uint32_t tri = __float_as_uint(t0.w);
                if (tri == skip) continue;
                if (STATS) n_tris++;
                if (!triangles_pierce(ax, ay, az, bx, by, bz, cx, cy, cz, t0, t1, t2)) continue;
                if constexpr (MODE == kTriFill) {
                    if (pos < capacity) tris[pos] = tri;         // never a word at or beyond the capacity
                    pos++;
                } else {
                    n_found++;
                    if constexpr (MODE == kTriAny) { leaves = 0u; inner = 0u; sp = 0; }       // the first candidate ends the walk
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
                if constexpr (MODE != kTriFill) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- triangle casts: where a moving triangle first hits the mesh (lbvh_triangle_cast, include/lbvh.h) ----------------------
// The header's time of the query triangle (a, b, c) moving along d with one scene triangle line (t0, t1, t2), LBVH_MAX_FLOAT if it
// has none.  ONE copy of the Moeller-Trumbore body in a loop that is not unrolled, over 21 tests: the six start tests of
// triangles_pierce (they count only where `start` says the own box overlaps the query's), then the fifteen features.  The ray
// (P, D) and the target (V, E1, E2) of test j are picked by selects on j from five tables of 3-bit fields; nothing is indexed, so
// nothing goes to scratch.
//   P:  0 a   1 b   2 c   3 v0   4 v0 + e1   5 v0 + e2
//   D:  0 b - a   1 c - b   2 a - c   3 e1   4 e2   5 e2 - e1   6 d   7 -d
//   V:  0 v0   1 a   2 v0 + e1
//   E1: 0 e1   1 b - a   2 e2   3 e2 - e1
//   E2: 0 e2   1 c - a   2 -(b - a)   3 -(c - b)   4 -(a - c)
// `first` is 0, or 6 where no lane of the wave at this leaf has a start overlap to test (the same for every lane).  Tests 12 .. 20
// (features 6 .. 14) are the parallelogram mode of ray_triangle_edges; its u is the position on the scene edge.
__device__ __forceinline__ float triangle_cast_time(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                    float dx, float dy, float dz, const float4 t0, const float4 t1, const float4 t2,
                                                    bool start, uint32_t first, uint32_t& feature, float& w)
{
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
    const float cax = ax - cx, cay = ay - cy, caz = az - cz;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float v1x = t0.x + t1.x, v1y = t0.y + t1.y, v1z = t0.z + t1.z;
    const float v2x = t0.x + t2.x, v2y = t0.y + t2.y, v2z = t0.z + t2.z;
    const float e3x = t2.x - t1.x, e3y = t2.y - t1.y, e3z = t2.z - t1.z;
    float best = LBVH_MAX_FLOAT;
    feature = 0u;
    w = 0.0f;
#pragma nounroll
    for (uint32_t j = first; j < 21u; j++) {
        const uint32_t pi = (uint32_t)(0x2489200b1a223688ull >> (3u * j)) & 7u;
        const uint32_t di = (uint32_t)(0x6db6db6ffedac688ull >> (3u * j)) & 7u;
        const uint32_t vi = (uint32_t)(0x2010080248009200ull >> (3u * j)) & 7u;
        const uint32_t fi = (uint32_t)(0x341a0d0248009200ull >> (3u * j)) & 7u;
        const uint32_t gi = (uint32_t)(0x491b692248009200ull >> (3u * j)) & 7u;
#define TRI_CAST_PICK6(i, s0, s1, s2, s3, s4, s5) ((i) == 0u ? (s0) : ((i) == 1u ? (s1) : ((i) == 2u ? (s2) : ((i) == 3u ? (s3) : ((i) == 4u ? (s4) : (s5))))))
        ray_t r;
        r.ox = TRI_CAST_PICK6(pi, ax, bx, cx, t0.x, v1x, v2x);
        r.oy = TRI_CAST_PICK6(pi, ay, by, cy, t0.y, v1y, v2y);
        r.oz = TRI_CAST_PICK6(pi, az, bz, cz, t0.z, v1z, v2z);
        r.dx = di == 6u ? dx : (di == 7u ? -dx : TRI_CAST_PICK6(di, abx, bcx, cax, t1.x, t2.x, e3x));
        r.dy = di == 6u ? dy : (di == 7u ? -dy : TRI_CAST_PICK6(di, aby, bcy, cay, t1.y, t2.y, e3y));
        r.dz = di == 6u ? dz : (di == 7u ? -dz : TRI_CAST_PICK6(di, abz, bcz, caz, t1.z, t2.z, e3z));
        r.ix = 0.0f; r.iy = 0.0f; r.iz = 0.0f;           // (not read by the triangle test)
        const float4 v = make_float4(vi == 0u ? t0.x : (vi == 1u ? ax : v1x), vi == 0u ? t0.y : (vi == 1u ? ay : v1y),
                                     vi == 0u ? t0.z : (vi == 1u ? az : v1z), 0.0f);
        const float fx = fi == 0u ? t1.x : (fi == 1u ? abx : (fi == 2u ? t2.x : e3x));
        const float fy = fi == 0u ? t1.y : (fi == 1u ? aby : (fi == 2u ? t2.y : e3y));
        const float fz = fi == 0u ? t1.z : (fi == 1u ? abz : (fi == 2u ? t2.z : e3z));
        const float gx = TRI_CAST_PICK6(gi, t2.x, acx, -abx, -bcx, -cax, 0.0f);
        const float gy = TRI_CAST_PICK6(gi, t2.y, acy, -aby, -bcy, -cay, 0.0f);
        const float gz = TRI_CAST_PICK6(gi, t2.z, acz, -abz, -bcz, -caz, 0.0f);
#undef TRI_CAST_PICK6
        const bool quad = j >= 12u;
        float u = 0.0f, vv = 0.0f;
        const float t = ray_triangle_edges<true>(r, v, fx, fy, fz, gx, gy, gz, u, vv, quad);
        if (j < 6u) {
            if (start && 0.0f <= t && t <= 1.0f) { feature = 16u | j; return 0.0f; }      // in overlap at the start: +0, w = +0
        } else if (t >= 0.0f && t < best) {              // false for a NaN; a rejected test has LBVH_MAX_FLOAT and replaces nothing
            best = t; feature = j - 6u; w = quad ? u : 0.0f;
        }
    }
    return best;
}

// cast k into the lane (best_t = T): false (miss record / 0 written, lane stays idle) for an inactive cast; !RECORD (the cast-all
// walks): nothing is written
template <bool ANY, bool RECORD = true>
__device__ __forceinline__ bool load_triangle_cast(const lbvh_tri_ray* __restrict__ casts, uint32_t k, float4& qa, float4& qb, float4& qc,
                                                   ray_t& ray, float& best_t, std::conditional_t<ANY, uint32_t, lbvh_tri_cast_hit>* __restrict__ out)
{
    const float inf = __builtin_inff();
    const float4* q = reinterpret_cast<const float4*>(&casts[k]);
    qa = q[0]; qb = q[1]; qc = q[2];
    const float4 d = q[3];
    ray.ox = qa.x; ray.oy = qa.y; ray.oz = qa.z;
    ray.dx = d.x; ray.dy = d.y; ray.dz = d.z;
    ray.ix = 1.0f / d.x; ray.iy = 1.0f / d.y; ray.iz = 1.0f / d.z;
    best_t = fminf(qb.w, LBVH_MAX_FLOAT);                // T: candidates have t < T
    if (qb.w > 0.0f && fabsf(qa.x) < inf && fabsf(qa.y) < inf && fabsf(qa.z) < inf && fabsf(qb.x) < inf && fabsf(qb.y) < inf &&
        fabsf(qb.z) < inf && fabsf(qc.x) < inf && fabsf(qc.y) < inf && fabsf(qc.z) < inf && fabsf(d.x) < inf && fabsf(d.y) < inf &&
        fabsf(d.z) < inf && dot3(d.x, d.y, d.z, d.x, d.y, d.z) > 0.0f) return true;
    if constexpr (!RECORD) return false;
    else if constexpr (ANY) out[k] = 0u;
    else reinterpret_cast<float4*>(out)[k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), __uint_as_float(0u), 0.0f);
    return false;
}

// One cast per lane in the frame of box_cast_wide_kernel, the ray that of vertex a.  The four slot boxes are grown by the query's
// extent relative to a: lo - max(b - a, c - a, 0) and hi - min(b - a, c - a, 0) per axis, one operation per bound and monotone in
// lo / hi, so a grown box contains the grown boxes of everything below it and the record does not depend on the order of the walk,
// as there.  A slot is skipped when the ray misses its grown box or enters it beyond best_t, strictly, never on an exit distance.
// A leaf slot's box before it is grown is the triangle's own: it decides with the query's exact box whether the start tests count.
// The record is {t, tri, feature, w}; ANY: a flag, the walk cut off at its first candidate (best_t stays T).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void triangle_cast_wide_kernel(const lbvh_tri_ray* __restrict__ casts, uint32_t total,
                                                                const lbvh_wide_node* __restrict__ wide,
                                                                const lbvh_fast_node* __restrict__ lines,
                                                                std::conditional_t<ANY, uint32_t, lbvh_tri_cast_hit>* __restrict__ out,
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false, took = false;
    uint32_t i = 0;
    ray_t ray = {};
    float4 qa = {}, qb = {}, qc = {};                    // the three vertices; qa.w = skip
    float ux = 0.0f, uy = 0.0f, uz = 0.0f, ox = 0.0f, oy = 0.0f, oz = 0.0f;      // what a box's lower / upper bounds lose
    float best_t = LBVH_MAX_FLOAT, best_w = 0.0f;
    uint32_t best_tri = 0, best_feature = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_triangle_cast<ANY>(casts, k, qa, qb, qc, ray, best_t, out);
                    const float h1x = qb.x - qa.x, h1y = qb.y - qa.y, h1z = qb.z - qa.z;
                    const float h2x = qc.x - qa.x, h2y = qc.y - qa.y, h2z = qc.z - qa.z;
                    ux = fmaxf(fmaxf(h1x, h2x), 0.0f); uy = fmaxf(fmaxf(h1y, h2y), 0.0f); uz = fmaxf(fmaxf(h1z, h2z), 0.0f);
                    ox = fminf(fminf(h1x, h2x), 0.0f); oy = fminf(fminf(h1y, h2y), 0.0f); oz = fminf(fminf(h1z, h2z), 0.0f);
                    best_tri = 0; best_feature = 0; best_w = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_casts++;
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
            const bool h0 = wide_box(lox.x - ux, loy.x - uy, loz.x - uz, hix.x - ox, hiy.x - oy, hiz.x - oz, ray, t0) && !(t0 > best_t) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y - ux, loy.y - uy, loz.y - uz, hix.y - ox, hiy.y - oy, hiz.y - oz, ray, t1) && !(t1 > best_t) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z - ux, loy.z - uy, loz.z - uz, hix.z - ox, hiy.z - oy, hiz.z - oz, ray, t2) && !(t2 > best_t) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w - ux, loy.w - uy, loz.w - uz, hix.w - ox, hiy.w - oy, hiz.w - oz, ray, t3) && !(t3 > best_t) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                const uint32_t tri = __float_as_uint(v0.w);
                if (tri == __float_as_uint(qa.w)) continue;          // `skip`
                if (STATS) n_tris++;
                // rule (2) of lbvh_triangle_intersections: the triangle's own box (the slot's, not grown) against the query's exact box
                const bool start = boxes_overlap(fminf(fminf(qa.x, qb.x), qc.x), fminf(fminf(qa.y, qb.y), qc.y), fminf(fminf(qa.z, qb.z), qc.z),
                                                 fmaxf(fmaxf(qa.x, qb.x), qc.x), fmaxf(fmaxf(qa.y, qb.y), qc.y), fmaxf(fmaxf(qa.z, qb.z), qc.z),
                                                 k == 0u ? lox.x : (k == 1u ? lox.y : (k == 2u ? lox.z : lox.w)),
                                                 k == 0u ? loy.x : (k == 1u ? loy.y : (k == 2u ? loy.z : loy.w)),
                                                 k == 0u ? loz.x : (k == 1u ? loz.y : (k == 2u ? loz.z : loz.w)),
                                                 k == 0u ? hix.x : (k == 1u ? hix.y : (k == 2u ? hix.z : hix.w)),
                                                 k == 0u ? hiy.x : (k == 1u ? hiy.y : (k == 2u ? hiy.z : hiy.w)),
                                                 k == 0u ? hiz.x : (k == 1u ? hiz.y : (k == 2u ? hiz.z : hiz.w)));
                uint32_t feature;
                float fw;
                const float t = triangle_cast_time(qa.x, qa.y, qa.z, qb.x, qb.y, qb.z, qc.x, qc.y, qc.z, ray.dx, ray.dy, ray.dz, v0, v1, v2,
                                                   start, __any(start) ? 0u : 6u, feature, fw);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                // best_t starts at T and best_tri at 0: t == T is never taken.  Ties go to the lower triangle index.
                if (hit_counts(t, entry) && (t < best_t || (t == best_t && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else { best_t = t; best_tri = tri; best_feature = feature; best_w = fw; took = true; }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by entry distance (the order key of sphere_cast_wide_kernel)
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(t0 > best_t) ? ((__float_as_uint(fmaxf(t0, 0.0f)) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(t1 > best_t) ? ((__float_as_uint(fmaxf(t1, 0.0f)) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(t2 > best_t) ? ((__float_as_uint(fmaxf(t2, 0.0f)) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(t3 > best_t) ? ((__float_as_uint(fmaxf(t3, 0.0f)) & ~3u) | 3u) : none;
            {   // five compare-exchanges
                uint32_t a, c;
                a = min(k0, k1); c = max(k0, k1); k0 = a; k1 = c;
                a = min(k2, k3); c = max(k2, k3); k2 = a; k3 = c;
                a = min(k0, k2); c = max(k0, k2); k0 = a; k2 = c;
                a = min(k1, k3); c = max(k1, k3); k1 = a; k3 = c;
                a = min(k1, k2); c = max(k1, k2); k1 = a; k2 = c;
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
                if constexpr (ANY) out[i] = 0u;
                else reinterpret_cast<float4*>(out)[i] = make_float4(took ? best_t : LBVH_MAX_FLOAT, __uint_as_float(best_tri),
                                                                     __uint_as_float(best_feature), best_w);
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// ---- every triangle a moving triangle touches, as a CSR list (lbvh_triangle_cast_all, include/lbvh.h) -----------------------
// The frame of cast_gather_wide_kernel (count walk, scan, fill walk: the same kernel, the same decisions; persistent waves, lane
// refill with the write position reloaded, LDS + device-memory stack, leaf slots first, the first passing inner slot entered and
// the others pushed) around the arithmetic of triangle_cast_wide_kernel: load_triangle_cast's activity test and T, the grown box
// lo - u / hi - o against the FIXED bound T, `skip` before the stats count, the start flag from the slot's own box, and
// triangle_cast_time.  A candidate is what the cast kernel accepts while its best is still (T, 0): hit_counts(t, entry) && t < T.
// triangle_cast_time gives the whole record {t, tri, feature, w} in both walks; the count walk leaves feature and w unread.
// A kernel of its own, not a fourth shape of cast_gather_wide_kernel: the cast record's type is spelled in that kernel's symbols,
// and the walk as a device function under two entries changed the instructions of six of its twelve instantiations (DESIGN).
template <bool FILL, bool STATS>
__global__ __launch_bounds__(64) void triangle_cast_gather_wide_kernel(const lbvh_tri_ray* __restrict__ casts, uint32_t total,
                                                                       const lbvh_wide_node* __restrict__ wide,
                                                                       const lbvh_fast_node* __restrict__ lines,
                                                                       uint32_t* __restrict__ counts,            // !FILL: candidates of cast k
                                                                       const uint64_t* __restrict__ offsets,     // FILL: where segment k starts
                                                                       float4* __restrict__ hits, uint64_t capacity,     // lbvh_tri_cast_hit records
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
    uint32_t n_casts = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t ray = {};
    float4 qa = {}, qb = {}, qc = {};                    // the three vertices; qa.w = skip
    float ux = 0.0f, uy = 0.0f, uz = 0.0f, ox = 0.0f, oy = 0.0f, oz = 0.0f;      // what a box's lower / upper bounds lose
    float T = LBVH_MAX_FLOAT;
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
                    active = load_triangle_cast<false, false>(casts, k, qa, qb, qc, ray, T, nullptr);
                    const float h1x = qb.x - qa.x, h1y = qb.y - qa.y, h1z = qb.z - qa.z;
                    const float h2x = qc.x - qa.x, h2y = qc.y - qa.y, h2z = qc.z - qa.z;
                    ux = fmaxf(fmaxf(h1x, h2x), 0.0f); uy = fmaxf(fmaxf(h1y, h2y), 0.0f); uz = fmaxf(fmaxf(h1z, h2z), 0.0f);
                    ox = fminf(fminf(h1x, h2x), 0.0f); oy = fminf(fminf(h1y, h2y), 0.0f); oz = fminf(fminf(h1z, h2z), 0.0f);
                    sp = 0; node = 0;
                    if constexpr (FILL) { if (active) pos = offsets[k]; }      // (reloaded at every refill: a lane serves many casts)
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_casts++;
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
            const bool h0 = wide_box(lox.x - ux, loy.x - uy, loz.x - uz, hix.x - ox, hiy.x - oy, hiz.x - oz, ray, t0) && !(t0 > T) && ref.x != kWideEmpty;
            const bool h1 = wide_box(lox.y - ux, loy.y - uy, loz.y - uz, hix.y - ox, hiy.y - oy, hiz.y - oz, ray, t1) && !(t1 > T) && ref.y != kWideEmpty;
            const bool h2 = wide_box(lox.z - ux, loy.z - uy, loz.z - uz, hix.z - ox, hiy.z - oy, hiz.z - oz, ray, t2) && !(t2 > T) && ref.z != kWideEmpty;
            const bool h3 = wide_box(lox.w - ux, loy.w - uy, loz.w - uz, hix.w - ox, hiy.w - oy, hiz.w - oz, ray, t3) && !(t3 > T) && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                if (__float_as_uint(v0.w) == __float_as_uint(qa.w)) continue;      // `skip`
                if (STATS) n_tris++;
                // rule (2) of lbvh_triangle_intersections: the triangle's own box (the slot's, not grown) against the query's exact box
                const bool start = boxes_overlap(fminf(fminf(qa.x, qb.x), qc.x), fminf(fminf(qa.y, qb.y), qc.y), fminf(fminf(qa.z, qb.z), qc.z),
                                                 fmaxf(fmaxf(qa.x, qb.x), qc.x), fmaxf(fmaxf(qa.y, qb.y), qc.y), fmaxf(fmaxf(qa.z, qb.z), qc.z),
                                                 k == 0u ? lox.x : (k == 1u ? lox.y : (k == 2u ? lox.z : lox.w)),
                                                 k == 0u ? loy.x : (k == 1u ? loy.y : (k == 2u ? loy.z : loy.w)),
                                                 k == 0u ? loz.x : (k == 1u ? loz.y : (k == 2u ? loz.z : loz.w)),
                                                 k == 0u ? hix.x : (k == 1u ? hix.y : (k == 2u ? hix.z : hix.w)),
                                                 k == 0u ? hiy.x : (k == 1u ? hiy.y : (k == 2u ? hiy.z : hiy.w)),
                                                 k == 0u ? hiz.x : (k == 1u ? hiz.y : (k == 2u ? hiz.z : hiz.w)));
                uint32_t feature;
                float fw;
                const float t = triangle_cast_time(qa.x, qa.y, qa.z, qb.x, qb.y, qb.z, qc.x, qc.y, qc.z, ray.dx, ray.dy, ray.dz, v0, v1, v2,
                                                   start, __any(start) ? 0u : 6u, feature, fw);
                const float entry = k == 0u ? t0 : (k == 1u ? t1 : (k == 2u ? t2 : t3));
                if (hit_counts(t, entry) && t < T) {
                    if constexpr (FILL) {
                        if (pos < capacity) hits[pos] = make_float4(t, v0.w, __uint_as_float(feature), fw);      // never at or beyond the capacity
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
    if (STATS) add_ray_stats(stats, n_casts, n_steps, n_tris);
}

// ---- triangle intersection segments: WHERE a triangle cuts each scene triangle it intersects ------------------------------
// (lbvh_triangle_intersection_segments, include/lbvh.h).  The frame, the slot test and `skip` of triangle_query_wide_kernel; the
// count walk of the call IS that kernel's kTriCount form.  This is the fill walk: it writes a 32-byte lbvh_tri_segment where
// kTriFill writes an index.

// The header's record of a query (a, b, c) with the triangle line (t0, t1, t2); false: not a candidate.  The six tests are
// triangles_pierce's — the same operand selection, the same ray_triangle_edges call, so the same six t —, but no test ends the
// loop: a pair is a candidate iff some t passes, which is the decision of the count walk, and every passing t gives a point
// X_j = P_j + D_j * t_j (one multiplication and one addition per component).  The loop carries the pass mask, the running pair
// (six floats) and the two test numbers that gave it; nothing is indexed, so nothing goes to scratch.  Every lane takes six
// turns: a wave whose lanes disagree on which tests pass still merges at the loop's end.
// rec0 = {p0, tri (set by the caller)}, rec1 = {p1, edges}.
__device__ __forceinline__ bool triangle_segment_of(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                    const float4 t0, const float4 t1, const float4 t2, float4& rec0, float4& rec1)
{
    const float abx = bx - ax, aby = by - ay, abz = bz - az;
    const float acx = cx - ax, acy = cy - ay, acz = cz - az;
    uint32_t mask = 0u, j0 = 0u, j1 = 0u;
    float p0x = 0.0f, p0y = 0.0f, p0z = 0.0f, p1x = 0.0f, p1y = 0.0f, p1z = 0.0f;
#pragma nounroll
    for (uint32_t j = 0; j < 6u; j++) {
        const bool query_edge = j < 3u;
        ray_t r;
        if (j == 0u) { r.ox = ax; r.oy = ay; r.oz = az; r.dx = abx; r.dy = aby; r.dz = abz; }
        else if (j == 1u) { r.ox = bx; r.oy = by; r.oz = bz; r.dx = cx - bx; r.dy = cy - by; r.dz = cz - bz; }
        else if (j == 2u) { r.ox = cx; r.oy = cy; r.oz = cz; r.dx = ax - cx; r.dy = ay - cy; r.dz = az - cz; }
        else if (j == 3u) { r.ox = t0.x; r.oy = t0.y; r.oz = t0.z; r.dx = t1.x; r.dy = t1.y; r.dz = t1.z; }
        else if (j == 4u) { r.ox = t0.x; r.oy = t0.y; r.oz = t0.z; r.dx = t2.x; r.dy = t2.y; r.dz = t2.z; }
        else { r.ox = t0.x + t1.x; r.oy = t0.y + t1.y; r.oz = t0.z + t1.z; r.dx = t2.x - t1.x; r.dy = t2.y - t1.y; r.dz = t2.z - t1.z; }
        r.ix = 0.0f; r.iy = 0.0f; r.iz = 0.0f;           // (not read by the triangle test)
        const float4 v = query_edge ? t0 : make_float4(ax, ay, az, 0.0f);
        float bu = 0.0f, bv = 0.0f;
        const float t = ray_triangle_edges(r, v, query_edge ? t1.x : abx, query_edge ? t1.y : aby, query_edge ? t1.z : abz,
                                           query_edge ? t2.x : acx, query_edge ? t2.y : acy, query_edge ? t2.z : acz, bu, bv);
        if (0.0f <= t && t <= 1.0f) {                    // edge_pierces' decision (false for a NaN t and for the miss value)
            const float x = r.ox + r.dx * t, y = r.oy + r.dy * t, z = r.oz + r.dz * t;
            if (mask == 0u) { p0x = x; p0y = y; p0z = z; p1x = x; p1y = y; p1z = z; j0 = j; j1 = j; }
            else if ((mask & (mask - 1u)) == 0u) { p1x = x; p1y = y; p1z = z; j1 = j; }
            else {                                       // a third point or later: keep the two that lie farthest apart
                const float ex = p0x - p1x, ey = p0y - p1y, ez = p0z - p1z;
                const float fx = p0x - x, fy = p0y - y, fz = p0z - z;
                const float gx = p1x - x, gy = p1y - y, gz = p1z - z;
                const float d01 = dot3(ex, ey, ez, ex, ey, ez), d0 = dot3(fx, fy, fz, fx, fy, fz), d1 = dot3(gx, gy, gz, gx, gy, gz);
                if (d0 > d01 && d0 >= d1) { p1x = x; p1y = y; p1z = z; j1 = j; }
                else if (d1 > d01) { p0x = x; p0y = y; p0z = z; j0 = j; }
            }
            mask |= 1u << j;
        }
    }
    if (mask == 0u) return false;
    rec0.x = p0x; rec0.y = p0y; rec0.z = p0z;
    rec1 = make_float4(p1x, p1y, p1z, __uint_as_float(mask | (j0 << 8) | (j1 << 12)));
    return true;
}

template <bool STATS>
__global__ __launch_bounds__(64) void triangle_segment_wide_kernel(const float4* __restrict__ queries, uint32_t total,     // three float4 per query
                                                                   const lbvh_wide_node* __restrict__ wide,
                                                                   const lbvh_fast_node* __restrict__ lines,
                                                                   const uint64_t* __restrict__ offsets,     // where segment k starts
                                                                   lbvh_tri_segment* __restrict__ out, uint64_t capacity,
                                                                   uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                                   uint32_t lds_depth,              // <= kWideStackLds
                                                                   uint32_t deep_cap,               // <= kWideStackDeep
                                                                   uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    float4* records = reinterpret_cast<float4*>(out);
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t skip = kWideEmpty;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
    float lx = 0.0f, ly = 0.0f, lz = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;      // the query's box
    uint32_t sp = 0, node = 0;
    uint64_t pos = 0;                                    // where this lane's next record goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    const float inf = __builtin_inff();
                    const float4 qa = queries[3 * (size_t)k], qb = queries[3 * (size_t)k + 1], qc = queries[3 * (size_t)k + 2];
                    ax = qa.x; ay = qa.y; az = qa.z; skip = __float_as_uint(qa.w);
                    bx = qb.x; by = qb.y; bz = qb.z;
                    cx = qc.x; cy = qc.y; cz = qc.z;
                    lx = fminf(fminf(ax, bx), cx); ly = fminf(fminf(ay, by), cy); lz = fminf(fminf(az, bz), cz);
                    hx = fmaxf(fmaxf(ax, bx), cx); hy = fmaxf(fmaxf(ay, by), cy); hz = fmaxf(fmaxf(az, bz), cz);
                    active = fabsf(ax) < inf && fabsf(ay) < inf && fabsf(az) < inf && fabsf(bx) < inf && fabsf(by) < inf && fabsf(bz) < inf &&
                             fabsf(cx) < inf && fabsf(cy) < inf && fabsf(cz) < inf;         // all nine finite (false for NaN)
                    sp = 0; node = 0;
                    if (active) pos = offsets[k];
                    if (STATS && active) n_queries++;
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
            const bool h0 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x) && ref.x != kWideEmpty;
            const bool h1 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y) && ref.y != kWideEmpty;
            const bool h2 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z) && ref.z != kWideEmpty;
            const bool h3 = boxes_overlap(lx, ly, lz, hx, hy, hz, lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w) && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 t0, t1, t2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
                if (__float_as_uint(t0.w) == skip) continue;
                if (STATS) n_tris++;
                float4 rec0, rec1;
                rec0.w = t0.w;                                   // the ORIGINAL triangle index
                if (!triangle_segment_of(ax, ay, az, bx, by, bz, cx, cy, cz, t0, t1, t2, rec0, rec1)) continue;
                if (pos < capacity) { records[2 * pos] = rec0; records[2 * pos + 1] = rec1; }     // never a record at or beyond the capacity
                pos++;
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
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- shape overlaps: which triangles a capsule or an oriented box touches where it stands (lbvh_capsule_overlaps, -------
// lbvh_obb_overlaps, include/lbvh.h).  The frame of triangle_query_wide_kernel with the casts' grown bounds for the slot test: a
// slot is entered iff the shape's origin (centre) lies in the slot's box grown as capsule_cast_wide_kernel / box_cast_wide_kernel
// grow it, formed per slot (two operations per bound for the capsule, one for the box, each monotone in lo / hi, so every ancestor
// of a candidate's leaf passes), in closed comparisons.  At a leaf slot that passes — its box is the triangle's own — the triangle
// line is read once and the casts' start-overlap arithmetic decides: shape_touches below.  kTriCount and kTriFill are the two
// walks of the CSR protocol; kTriAny stops a lane at its first candidate.
enum overlap_shape : int { kShapeCapsule = 0, kShapeObb = 1 };

// a capsule (origin o, axis h, R2 = r*r) against the triangle line (a, e1, e2): some derived triangle j = 0 .. 7 of lbvh_capsule_cast
// has point_triangle2(o) <= R2 — the start overlap of sphere_triangle_time, the first one ends the loop —, or the axis pierces the
// face.  One copy of the point test in a loop that is not unrolled, as in capsule_triangle_time; the loop leaves through its
// condition: with a `return` in its body the compiler unrolled it all the same (240 VGPRs, 2 waves per SIMD, against 85 / 5).
__device__ __forceinline__ bool capsule_touches(const ray_t& o, float R2, float hx, float hy, float hz, const float4 a, const float4 e1,
                                                const float4 e2)
{
    bool within = false;
#pragma nounroll
    for (uint32_t j = 0; j < 8u && !within; j++) {
        float4 p, q1, q2;
        capsule_triangle(j, a, e1, e2, hx, hy, hz, p, q1, q2);
        float u, v;
        within = point_triangle2(o.ox, o.oy, o.oz, p, q1, q2, u, v) <= R2;
    }
    if (within) return true;
    ray_t ax;
    ax.ox = o.ox; ax.oy = o.oy; ax.oz = o.oz;
    ax.dx = hx; ax.dy = hy; ax.dz = hz;
    ax.ix = 0.0f; ax.iy = 0.0f; ax.iz = 0.0f;            // (not read by the triangle test)
    float u = 0.0f, v = 0.0f;
    const float tp = ray_triangle_edges(ax, a, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, u, v);
    return 0.0f <= tp && tp <= 1.0f;
}

// a box (centre c, half-axis vectors b) against the triangle line: no one of the thirteen axes of lbvh_box_cast separates them,
// lo <= rb && -rb <= hi on every axis (box_triangle_time's v = 0 branch); the first separating axis ends the loop.  A NaN in lo,
// hi or rb fails the comparison: no candidate.
__device__ __forceinline__ bool box_touches(const ray_t& c, const box_axes& b, const float4 a, const float4 e1, const float4 e2)
{
    const float mx = a.x - c.ox, my = a.y - c.oy, mz = a.z - c.oz;
    const float e3x = e2.x - e1.x, e3y = e2.y - e1.y, e3z = e2.z - e1.z;
#pragma nounroll
    for (uint32_t j = 0; j < 13u; j++) {
        float lx, ly, lz, lo, hi, rb;
        box_axis_spans(j, mx, my, mz, b, e1, e2, e3x, e3y, e3z, lx, ly, lz, lo, hi, rb);
        if (!(lo <= rb && -rb <= hi)) return false;
    }
    return true;
}

// the origin (centre) o against one slot box [lo, hi] grown below by `under` and above by `over`, then by r on both sides
// (capsule: under = max(h, 0), over = min(h, 0), the cast's (lo - max(h, 0)) - r and (hi - min(h, 0)) + r; box: lo - g and hi + g)
template <int SHAPE>
__device__ __forceinline__ bool shape_in_grown(float lo, float hi, float o, float under, float over, float r)
{
    if constexpr (SHAPE == kShapeCapsule) return (lo - under) - r <= o && o <= (hi - over) + r;
    else return lo - under <= o && o <= hi + under;
}

template <int SHAPE, int MODE, bool STATS>
__global__ __launch_bounds__(64) void shape_overlap_wide_kernel(const float4* __restrict__ shapes, uint32_t total,   // two (capsule) or four (box) float4 per shape
                                                                const lbvh_wide_node* __restrict__ wide,
                                                                const lbvh_fast_node* __restrict__ lines,
                                                                uint32_t* __restrict__ counts,            // kTriCount: candidates of shape k; kTriAny: the flags
                                                                const uint64_t* __restrict__ offsets,     // kTriFill: where segment k starts
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
    uint32_t n_shapes = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t o = {};                                        // the origin / centre (the direction is not read)
    box_axes b = {};                                     // box: the half-axis vectors
    float r = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;     // capsule: the radius and the axis; box: h = g, the half extent per world axis
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // kTriFill: where this lane's next candidate goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float inf = __builtin_inff();
                    if constexpr (SHAPE == kShapeCapsule) {
                        const float4 q0 = shapes[2 * (size_t)k], q1 = shapes[2 * (size_t)k + 1];
                        o.ox = q0.x; o.oy = q0.y; o.oz = q0.z; r = q0.w;
                        hx = q1.x; hy = q1.y; hz = q1.z;
                        active = r > 0.0f && r < inf && (q0.x == q0.x && q0.y == q0.y && q0.z == q0.z) &&
                                 fabsf(hx) < inf && fabsf(hy) < inf && fabsf(hz) < inf;
                    } else {
                        const float4 q0 = shapes[4 * (size_t)k], x = shapes[4 * (size_t)k + 1], y = shapes[4 * (size_t)k + 2], z = shapes[4 * (size_t)k + 3];
                        o.ox = q0.x; o.oy = q0.y; o.oz = q0.z;
                        b.xx = x.x; b.xy = x.y; b.xz = x.z;
                        b.yx = y.x; b.yy = y.y; b.yz = y.z;
                        b.zx = z.x; b.zy = z.y; b.zz = z.z;
                        hx = (fabsf(b.xx) + fabsf(b.yx)) + fabsf(b.zx);
                        hy = (fabsf(b.xy) + fabsf(b.yy)) + fabsf(b.zy);
                        hz = (fabsf(b.xz) + fabsf(b.yz)) + fabsf(b.zz);
                        const float det = dot3(x.x, x.y, x.z, y.y * z.z - y.z * z.y, y.z * z.x - y.x * z.z, y.x * z.y - y.y * z.x);
                        active = (q0.x == q0.x && q0.y == q0.y && q0.z == q0.z) &&
                                 fabsf(x.x) < inf && fabsf(x.y) < inf && fabsf(x.z) < inf && fabsf(y.x) < inf && fabsf(y.y) < inf && fabsf(y.z) < inf &&
                                 fabsf(z.x) < inf && fabsf(z.y) < inf && fabsf(z.z) < inf && fabsf(det) < inf && det != 0.0f;
                    }
                    sp = 0; node = 0;
                    if constexpr (MODE == kTriFill) { if (active) pos = offsets[k]; }
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_shapes++;
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
            // capsule: max(h, 0) and min(h, 0) are formed here from h, as in capsule_cast_wide_kernel; box: g both ways
            const bool cap = SHAPE == kShapeCapsule;
            const float ux = cap ? fmaxf(hx, 0.0f) : hx, uy = cap ? fmaxf(hy, 0.0f) : hy, uz = cap ? fmaxf(hz, 0.0f) : hz;
            const float vx = cap ? fminf(hx, 0.0f) : hx, vy = cap ? fminf(hy, 0.0f) : hy, vz = cap ? fminf(hz, 0.0f) : hz;
#define SHAPE_SLOT(c)                                                                                                          \
    (shape_in_grown<SHAPE>(lox.c, hix.c, o.ox, ux, vx, r) && shape_in_grown<SHAPE>(loy.c, hiy.c, o.oy, uy, vy, r) &&          \
     shape_in_grown<SHAPE>(loz.c, hiz.c, o.oz, uz, vz, r) && ref.c != kWideEmpty)
            const bool h0 = SHAPE_SLOT(x), h1 = SHAPE_SLOT(y), h2 = SHAPE_SLOT(z), h3 = SHAPE_SLOT(w);
#undef SHAPE_SLOT
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 t0, t1, t2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
                const uint32_t tri = __float_as_uint(t0.w);
                if (STATS) n_tris++;
                bool touches;
                if constexpr (SHAPE == kShapeCapsule) touches = capsule_touches(o, r * r, hx, hy, hz, t0, t1, t2);
                else touches = box_touches(o, b, t0, t1, t2);
                if (!touches) continue;
                if constexpr (MODE == kTriFill) {
                    if (pos < capacity) tris[pos] = tri;         // never a word at or beyond the capacity
                    pos++;
                } else {
                    n_found++;
                    if constexpr (MODE == kTriAny) { leaves = 0u; inner = 0u; sp = 0; }       // the first candidate ends the walk
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
                if constexpr (MODE != kTriFill) counts[i] = n_found;
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_shapes, n_steps, n_tris);
}

// ---- capsule contacts: how deep a capsule is in each triangle it touches, and which way out (lbvh_capsule_contacts, --------
// lbvh_capsule_deepest, include/lbvh.h).  The frame and the slot test of shape_overlap_wide_kernel<kShapeCapsule>; the count walk
// of lbvh_capsule_contacts IS that kernel's kTriCount form.  kContactFill writes a 32-byte record where the overlap's fill walk
// writes an index; kContactDeepest keeps the deepest record of the lane's shape in registers and writes it when the walk ends.
enum contact_mode : int { kContactFill = 0, kContactDeepest = 1 };

// The header's contact of a capsule (origin o, axis h, radius r) with the triangle line (a, e1, e2); false: not a candidate.
// The decision is capsule_touches' on the same values — `within` is some d_j <= R2 over the same eight dist2, the pierce is the
// same call —, but no derived triangle ends the loop: the least d_j picks s.  One copy of the point test in one rolled loop that
// leaves through its condition (as capsule_touches): j = 0 .. 7 the derived triangles at o, j = 8 the scene triangle at
// x = o + h*s, entered by candidates only.  rec0 = {depth, tri (set by the caller), u, v}, rec1 = {normal, s}.
__device__ __forceinline__ bool capsule_contact_of(const ray_t& o, float r, float hx, float hy, float hz, const float4 a, const float4 e1,
                                                   const float4 e2, float4& rec0, float4& rec1)
{
    ray_t ax;
    ax.ox = o.ox; ax.oy = o.oy; ax.oz = o.oz;
    ax.dx = hx; ax.dy = hy; ax.dz = hz;
    ax.ix = 0.0f; ax.iy = 0.0f; ax.iz = 0.0f;            // (not read by the triangle test)
    float pu = 0.0f, pv = 0.0f;
    const float tp = ray_triangle_edges(ax, a, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, pu, pv);
    const bool pierced = 0.0f <= tp && tp <= 1.0f;
    const float R2 = r * r;
    bool within = false;
    float least = __builtin_inff(), least_v = 0.0f;
    uint32_t which = 0u;
    float s = 0.0f, dist2 = 0.0f, u = 0.0f, v = 0.0f;
#pragma nounroll
    for (uint32_t j = 0; j < 9u && (j < 8u || within || pierced); j++) {
        const bool last = j == 8u;
        // s as lbvh_capsule_cast derives it from the winning j: 0, 1, v' or 1 - v'; t_p for the pierce (read at j = 8 only)
        s = pierced ? tp : (which == 0u ? 0.0f : (which == 1u ? 1.0f : ((which & 1u) ? 1.0f - least_v : least_v)));
        float4 p, q1, q2;
        capsule_triangle(last ? 0u : j, a, e1, e2, hx, hy, hz, p, q1, q2);
        const float px = last ? o.ox + hx * s : o.ox, py = last ? o.oy + hy * s : o.oy, pz = last ? o.oz + hz * s : o.oz;
        float uj, vj;
        const float d = point_triangle2(px, py, pz, p, q1, q2, uj, vj);
        if (last) { dist2 = d; u = uj; v = vj; }
        else {
            within = within || d <= R2;
            if (d < least) { least = d; which = j; least_v = vj; }     // strictly less; false for a NaN
        }
    }
    if (!(within || pierced)) return false;
    float depth, nx, ny, nz;
    if (!pierced && dist2 > 0.0f) {                      // the residual of point_triangle2 at x, divided by its length
        const float apx = (o.ox + hx * s) - a.x, apy = (o.oy + hy * s) - a.y, apz = (o.oz + hz * s) - a.z;
        const float rx = apx - (e1.x * u + e2.x * v), ry = apy - (e1.y * u + e2.y * v), rz = apz - (e1.z * u + e2.z * v);
        const float dist = sqrtf(dist2);
        nx = rx / dist; ny = ry / dist; nz = rz / dist;
        depth = r - dist;
    } else {                                             // face contact: the axis pierces the face, or x lies on the triangle
        const float Nx = e1.y * e2.z - e1.z * e2.y, Ny = e1.z * e2.x - e1.x * e2.z, Nz = e1.x * e2.y - e1.y * e2.x;
        const float len = sqrtf(dot3(Nx, Ny, Nz, Nx, Ny, Nz));
        if (len == 0.0f || len != len) { nx = 0.0f; ny = 0.0f; nz = 0.0f; depth = r; }
        else {
            const float g0 = dot3(Nx, Ny, Nz, o.ox - a.x, o.oy - a.y, o.oz - a.z);
            const float g1 = dot3(Nx, Ny, Nz, (o.ox + hx) - a.x, (o.oy + hy) - a.y, (o.oz + hz) - a.z);
            const float sign = g0 + g1 >= 0.0f ? 1.0f : -1.0f;
            nx = (sign * Nx) / len; ny = (sign * Ny) / len; nz = (sign * Nz) / len;
            depth = r + fmaxf(fmaxf(-sign * g0, -sign * g1), 0.0f) / len;
        }
    }
    rec0.x = depth; rec0.z = u; rec0.w = v;
    rec1 = make_float4(nx, ny, nz, s);
    return true;
}

template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void capsule_contact_wide_kernel(const lbvh_capsule* __restrict__ capsules, uint32_t total,
                                                                  const lbvh_wide_node* __restrict__ wide,
                                                                  const lbvh_fast_node* __restrict__ lines,
                                                                  const uint64_t* __restrict__ offsets,     // kContactFill: where segment k starts
                                                                  lbvh_contact* __restrict__ out,           // kContactFill: the records; kContactDeepest: one per shape
                                                                  uint64_t capacity,                        // kContactFill: records in `out`
                                                                  uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                                  uint32_t lds_depth,              // <= kWideStackLds
                                                                  uint32_t deep_cap,               // <= kWideStackDeep
                                                                  uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const float4* shapes = reinterpret_cast<const float4*>(capsules);
    float4* records = reinterpret_cast<float4*>(out);
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_shapes = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t o = {};                                        // the origin (the direction is not read)
    float r = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;
    uint32_t sp = 0, node = 0;
    uint64_t pos = 0;                                    // kContactFill: where this lane's next record goes
    float4 best0 = {}, best1 = {};                       // kContactDeepest: the deepest record so far
    const float4 none0 = make_float4(0.0f, __uint_as_float(LBVH_NULL), 0.0f, 0.0f), none1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float inf = __builtin_inff();
                    const float4 q0 = shapes[2 * (size_t)k], q1 = shapes[2 * (size_t)k + 1];
                    o.ox = q0.x; o.oy = q0.y; o.oz = q0.z; r = q0.w;
                    hx = q1.x; hy = q1.y; hz = q1.z;
                    active = r > 0.0f && r < inf && (q0.x == q0.x && q0.y == q0.y && q0.z == q0.z) &&
                             fabsf(hx) < inf && fabsf(hy) < inf && fabsf(hz) < inf;
                    sp = 0; node = 0;
                    if constexpr (MODE == kContactFill) { if (active) pos = offsets[k]; }
                    else {
                        best0 = none0; best1 = none1;
                        if (!active) { records[2 * (size_t)k] = none0; records[2 * (size_t)k + 1] = none1; }
                    }
                    if (STATS && active) n_shapes++;
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
            const float ux = fmaxf(hx, 0.0f), uy = fmaxf(hy, 0.0f), uz = fmaxf(hz, 0.0f);
            const float vx = fminf(hx, 0.0f), vy = fminf(hy, 0.0f), vz = fminf(hz, 0.0f);
#define SHAPE_SLOT(c)                                                                                                                  \
    (shape_in_grown<kShapeCapsule>(lox.c, hix.c, o.ox, ux, vx, r) && shape_in_grown<kShapeCapsule>(loy.c, hiy.c, o.oy, uy, vy, r) &&  \
     shape_in_grown<kShapeCapsule>(loz.c, hiz.c, o.oz, uz, vz, r) && ref.c != kWideEmpty)
            const bool h0 = SHAPE_SLOT(x), h1 = SHAPE_SLOT(y), h2 = SHAPE_SLOT(z), h3 = SHAPE_SLOT(w);
#undef SHAPE_SLOT
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 t0, t1, t2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
                if (STATS) n_tris++;
                float4 rec0, rec1;
                rec0.y = t0.w;                                   // the ORIGINAL triangle index
                if (!capsule_contact_of(o, r, hx, hy, hz, t0, t1, t2, rec0, rec1)) continue;
                if constexpr (MODE == kContactFill) {
                    if (pos < capacity) { records[2 * pos] = rec0; records[2 * pos + 1] = rec1; }     // never a record at or beyond the capacity
                    pos++;
                } else {
                    // the greatest depth; on equal depth the lower original index (the none-record's index is above every one)
                    const uint32_t tri = __float_as_uint(rec0.y), best_tri = __float_as_uint(best0.y);
                    if (best_tri == LBVH_NULL || rec0.x > best0.x || (!(rec0.x < best0.x) && tri < best_tri)) { best0 = rec0; best1 = rec1; }
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
                if constexpr (MODE == kContactDeepest) { records[2 * (size_t)i] = best0; records[2 * (size_t)i + 1] = best1; }
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_shapes, n_steps, n_tris);
}

// ---- segment queries: the nearest triangle of a segment / anything within a distance (lbvh_segment_closest_point, -----------
// lbvh_segment_within_distance, include/lbvh.h).  The frame and the nearest-first order of point_query_wide_kernel, with the box
// distance taken on bounds grown by the segment's axis; the narrow phase is steps 1 - 3 of capsule_contact_of.

// The header's distance of the segment [o, o + h] (`seg`: the origin, h in the direction; the inverse is not read) from the
// triangle line (a, e1, e2), with s, (u, v) and whether the pierce gave it (dist2 = +0 then, and the caller's delta is 0).  The
// rolled loop of capsule_contact_of without `within`, R2 and step 4: j = 0 .. 7 the derived triangles at o, j = 8 the scene
// triangle at x = o + h*s.  A pierced pair enters at j = 8 — the eight distances decide nothing for it —, and the ninth test is
// left out when no d_j was below +inf: which = 0 and s = 0 then, x is o, and its dist2 is d_0, which was not: NaN is returned.
__device__ __forceinline__ float segment_triangle2(const ray_t& seg, const float4 a, const float4 e1, const float4 e2, float& u_out,
                                                   float& v_out, float& s_out, bool& pierced_out)
{
    float pu = 0.0f, pv = 0.0f;
    const float tp = ray_triangle_edges(seg, a, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, pu, pv);
    const bool pierced = 0.0f <= tp && tp <= 1.0f;
    float least = __builtin_inff(), least_v = 0.0f;
    uint32_t which = 0u;
    float s = 0.0f, dist2 = __builtin_nanf(""), u = 0.0f, v = 0.0f;
#pragma nounroll
    for (uint32_t j = pierced ? 8u : 0u; j < 9u && (j < 8u || pierced || least < __builtin_inff()); j++) {
        const bool last = j == 8u;
        // s as lbvh_capsule_cast derives it from the winning j: 0, 1, v' or 1 - v'; t_p for the pierce (read at j = 8 only)
        s = pierced ? tp : (which == 0u ? 0.0f : (which == 1u ? 1.0f : ((which & 1u) ? 1.0f - least_v : least_v)));
        float4 p, q1, q2;
        capsule_triangle(last ? 0u : j, a, e1, e2, seg.dx, seg.dy, seg.dz, p, q1, q2);
        const float px = last ? seg.ox + seg.dx * s : seg.ox, py = last ? seg.oy + seg.dy * s : seg.oy, pz = last ? seg.oz + seg.dz * s : seg.oz;
        float uj, vj;
        const float d = point_triangle2(px, py, pz, p, q1, q2, uj, vj);
        if (last) { dist2 = d; u = uj; v = vj; }
        else if (d < least) { least = d; which = j; least_v = vj; }        // strictly less; false for a NaN
    }
    u_out = u; v_out = v; s_out = s;
    pierced_out = pierced;
    return pierced ? 0.0f : dist2;
}

// query k into the lane (best = R; the axis into seg's direction): false (none-record / 0 written, lane stays idle) for an inactive query
template <bool ANY>
__device__ __forceinline__ bool load_segment_query(const lbvh_segment_query* __restrict__ queries, uint32_t k, ray_t& seg, float& best,
                                                   std::conditional_t<ANY, uint32_t, lbvh_segment_closest>* __restrict__ out)
{
    const float inf = __builtin_inff();
    const float4 q0 = reinterpret_cast<const float4*>(queries)[2 * (size_t)k], q1 = reinterpret_cast<const float4*>(queries)[2 * (size_t)k + 1];
    seg.ox = q0.x; seg.oy = q0.y; seg.oz = q0.z;
    seg.dx = q1.x; seg.dy = q1.y; seg.dz = q1.z;
    best = fminf(q0.w, LBVH_MAX_FLOAT);
    if (q0.w > 0.0f && (q0.x == q0.x && q0.y == q0.y && q0.z == q0.z) && fabsf(q1.x) < inf && fabsf(q1.y) < inf && fabsf(q1.z) < inf)
        return true;                                                              // false for a NaN radius too
    if constexpr (ANY) out[k] = 0u;
    else {
        reinterpret_cast<float4*>(out)[2 * (size_t)k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), 0.0f, 0.0f);
        reinterpret_cast<float4*>(out)[2 * (size_t)k + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return false;
}

// One segment per lane over the four-wide nodes: point_query_wide_kernel with every box grown by the lane's axis before its
// distance from the origin is taken — lo - max(h, 0), hi - min(h, 0), one operation per bound, the max and min once per query —
// and segment_triangle2 at a leaf slot.  The grown bounds are monotone in lo and hi, so box2g grows from a box to any box inside
// it as box2 does, a subtree skipped because box2g > best holds no candidate at or below best, and the record does not depend on
// the order of the walk.  The closest form keeps {best, tri, u, v, delta, s} in registers and writes two 16-byte stores when the
// lane's walk ends.  ANY: a flag, the walk cut off at its first candidate (best stays R).
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void segment_query_wide_kernel(const lbvh_segment_query* __restrict__ queries, uint32_t total,
                                                                const lbvh_wide_node* __restrict__ wide,
                                                                const lbvh_fast_node* __restrict__ lines,
                                                                std::conditional_t<ANY, uint32_t, lbvh_segment_closest>* __restrict__ out,
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

    bool active = false, took = false;
    uint32_t i = 0;
    ray_t seg = {};                                      // the origin and, as the direction, the axis (the inverse is not read)
    float ux = 0.0f, uy = 0.0f, uz = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;      // max(h, 0) and min(h, 0) per axis
    float best = LBVH_MAX_FLOAT, best_u = 0.0f, best_v = 0.0f, best_s = 0.0f, best_dx = 0.0f, best_dy = 0.0f, best_dz = 0.0f;
    uint32_t best_tri = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    active = load_segment_query<ANY>(queries, k, seg, best, out);
                    ux = fmaxf(seg.dx, 0.0f); uy = fmaxf(seg.dy, 0.0f); uz = fmaxf(seg.dz, 0.0f);
                    vx = fminf(seg.dx, 0.0f); vy = fminf(seg.dy, 0.0f); vz = fminf(seg.dz, 0.0f);
                    best_tri = 0; best_u = 0.0f; best_v = 0.0f; best_s = 0.0f; best_dx = 0.0f; best_dy = 0.0f; best_dz = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_queries++;
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
#define GROWN_BOX2(c) point_box2(lox.c - ux, loy.c - uy, loz.c - uz, hix.c - vx, hiy.c - vy, hiz.c - vz, seg.ox, seg.oy, seg.oz)
            const float b0 = GROWN_BOX2(x), b1 = GROWN_BOX2(y), b2 = GROWN_BOX2(z), b3 = GROWN_BOX2(w);
#undef GROWN_BOX2
            const bool h0 = !(b0 > best) && ref.x != kWideEmpty, h1 = !(b1 > best) && ref.y != kWideEmpty;
            const bool h2 = !(b2 > best) && ref.z != kWideEmpty, h3 = !(b3 > best) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                if (STATS) n_tris++;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                float u = 0.0f, v = 0.0f, s = 0.0f;
                bool pierced = false;
                const float dist2 = segment_triangle2(seg, v0, v1, v2, u, v, s, pierced);
                const uint32_t tri = __float_as_uint(v0.w);
                const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                // best starts at R and best_tri at 0: dist2 == R is never taken.  Ties go to the lower triangle index.
                if (!(dist2 < own) && (dist2 < best || (dist2 == best && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else {
                        best = dist2; best_tri = tri; best_u = u; best_v = v; best_s = s; took = true;
                        // delta: the residual of point_triangle2 at x, from the nearest point of the triangle to x; 0 where pierced
                        const float apx = (seg.ox + seg.dx * s) - v0.x, apy = (seg.oy + seg.dy * s) - v0.y, apz = (seg.oz + seg.dz * s) - v0.z;
                        best_dx = pierced ? 0.0f : apx - (v1.x * u + v2.x * v);
                        best_dy = pierced ? 0.0f : apy - (v1.y * u + v2.y * v);
                        best_dz = pierced ? 0.0f : apz - (v1.z * u + v2.z * v);
                    }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by box distance as in point_query_wide_kernel: the distance's bit pattern with the slot number
            // in its two lowest bits; compared with `best` once more, which may have shrunk in the leaf loop
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(b0 > best) ? ((__float_as_uint(b0) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(b1 > best) ? ((__float_as_uint(b1) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(b2 > best) ? ((__float_as_uint(b2) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(b3 > best) ? ((__float_as_uint(b3) & ~3u) | 3u) : none;
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
                if constexpr (ANY) out[i] = 0u;
                else {
                    float4* rec = reinterpret_cast<float4*>(out) + 2 * (size_t)i;
                    rec[0] = make_float4(took ? best : LBVH_MAX_FLOAT, __uint_as_float(best_tri), best_u, best_v);
                    rec[1] = make_float4(best_dx, best_dy, best_dz, best_s);
                }
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- triangle distance queries: the nearest triangle of a triangle / anything within a distance (lbvh_triangle_closest_point, --
// lbvh_triangle_within_distance, include/lbvh.h).  The frame and the nearest-first order of segment_query_wide_kernel with the
// box-against-box distance for the slot test; the narrow phase is six calls of segment_triangle2 with the operands of
// triangles_pierce.

// Edge test m of the header for the query (a, b, c) and the scene line (t0, t1, t2): the segment (P, D) into `seg` and the other
// triangle's line into (v, f1, f2) — triangles_pierce's operands, every difference and sum the one fp32 operation of the header.
__device__ __forceinline__ void triangle_edge_test(uint32_t m, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy,
                                                   float cz, const float4 t0, const float4 t1, const float4 t2, ray_t& seg, float4& v,
                                                   float4& f1, float4& f2)
{
    float px, py, pz, dx, dy, dz;
    if (m == 0u) { px = ax; py = ay; pz = az; dx = bx - ax; dy = by - ay; dz = bz - az; }
    else if (m == 1u) { px = bx; py = by; pz = bz; dx = cx - bx; dy = cy - by; dz = cz - bz; }
    else if (m == 2u) { px = cx; py = cy; pz = cz; dx = ax - cx; dy = ay - cy; dz = az - cz; }
    else if (m == 3u) { px = t0.x; py = t0.y; pz = t0.z; dx = t1.x; dy = t1.y; dz = t1.z; }
    else if (m == 4u) { px = t0.x; py = t0.y; pz = t0.z; dx = t2.x; dy = t2.y; dz = t2.z; }
    else { px = t0.x + t1.x; py = t0.y + t1.y; pz = t0.z + t1.z; dx = t2.x - t1.x; dy = t2.y - t1.y; dz = t2.z - t1.z; }
    seg.ox = px; seg.oy = py; seg.oz = pz;
    seg.dx = dx; seg.dy = dy; seg.dz = dz;
    seg.ix = 0.0f; seg.iy = 0.0f; seg.iz = 0.0f;         // (not read)
    const bool query_edge = m < 3u;
    v = query_edge ? t0 : make_float4(ax, ay, az, 0.0f);
    f1 = query_edge ? t1 : make_float4(bx - ax, by - ay, bz - az, 0.0f);
    f2 = query_edge ? t2 : make_float4(cx - ax, cy - ay, cz - az, 0.0f);
}

// The header's distance of the query triangle from the scene line: the least dist2_m in the order m = 0 .. 5, strictly less, with
// edge = m | (pierced ? 8 : 0), s and the (u, v) of that test's step 3 (what delta is formed from when the pair is taken).  ONE
// copy of segment_triangle2 in a loop that is not unrolled (six inlined copies of its nine-test loop would be six times the code
// and the registers of the widest); the loop ends at the first dist2_m == +0: nothing after it is strictly less.  +inf when no
// test gave a number.
__device__ __forceinline__ float triangle_triangle2(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                    const float4 t0, const float4 t1, const float4 t2, uint32_t& edge_out, float& s_out,
                                                    float& u_out, float& v_out)
{
    float least = __builtin_inff(), s = 0.0f, u = 0.0f, v = 0.0f;
    uint32_t edge = 0u;
#pragma nounroll
    for (uint32_t m = 0; m < 6u && !(least == 0.0f); m++) {
        ray_t seg;
        float4 p, f1, f2;
        triangle_edge_test(m, ax, ay, az, bx, by, bz, cx, cy, cz, t0, t1, t2, seg, p, f1, f2);
        float um = 0.0f, vm = 0.0f, sm = 0.0f;
        bool pierced = false;
        const float d = segment_triangle2(seg, p, f1, f2, um, vm, sm, pierced);
        if (d < least) { least = d; edge = m | (pierced ? 8u : 0u); s = sm; u = um; v = vm; }     // strictly less; false for a NaN
    }
    edge_out = edge; s_out = s; u_out = u; v_out = v;
    return least;
}

// query k into the lane (best = R): false (none-record / 0 written, lane stays idle) for an inactive query
template <bool ANY>
__device__ __forceinline__ bool load_tri_distance_query(const lbvh_tri_distance_query* __restrict__ queries, uint32_t k, float4& qa, float4& qb,
                                                        float4& qc, float& best,
                                                        std::conditional_t<ANY, uint32_t, lbvh_tri_closest>* __restrict__ out)
{
    const float inf = __builtin_inff();
    qa = reinterpret_cast<const float4*>(queries)[3 * (size_t)k];
    qb = reinterpret_cast<const float4*>(queries)[3 * (size_t)k + 1];
    qc = reinterpret_cast<const float4*>(queries)[3 * (size_t)k + 2];
    best = fminf(qb.w, LBVH_MAX_FLOAT);
    if (qb.w > 0.0f && fabsf(qa.x) < inf && fabsf(qa.y) < inf && fabsf(qa.z) < inf && fabsf(qb.x) < inf && fabsf(qb.y) < inf &&
        fabsf(qb.z) < inf && fabsf(qc.x) < inf && fabsf(qc.y) < inf && fabsf(qc.z) < inf)
        return true;                                                              // false for a NaN radius or coordinate
    if constexpr (ANY) out[k] = 0u;
    else {
        reinterpret_cast<float4*>(out)[2 * (size_t)k] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0u), __uint_as_float(0u), 0.0f);
        reinterpret_cast<float4*>(out)[2 * (size_t)k + 1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
    }
    return false;
}

// box2q of the header: the squared distance of the box (lx .. hz) from the query's box (qlx .. qhz), point_box2 with an interval
// in the point's place
__device__ __forceinline__ float box_box2(float lx, float ly, float lz, float hx, float hy, float hz, float qlx, float qly, float qlz,
                                          float qhx, float qhy, float qhz)
{
    const float gx = fmaxf(fmaxf(lx - qhx, qlx - hx), 0.0f);
    const float gy = fmaxf(fmaxf(ly - qhy, qly - hy), 0.0f);
    const float gz = fmaxf(fmaxf(lz - qhz, qlz - hz), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// One query triangle per lane over the four-wide nodes: segment_query_wide_kernel with box2q in the place of the grown box's
// distance — the query's box is taken once per query — and triangle_triangle2 at a leaf slot, after `skip`.  box2q is monotone in
// the node box, so a subtree skipped because box2q > best holds no candidate at or below best, and the record does not depend on
// the order of the walk.  The closest form keeps {best, tri, edge, s, delta} in registers, forms delta only for a pair it takes
// (the operands of the winning m once more), and writes two 16-byte stores when the lane's walk ends.  ANY: a flag, the walk cut
// off at its first candidate (best stays R); no delta.
template <bool ANY, bool STATS>
__global__ __launch_bounds__(64) void triangle_distance_wide_kernel(const lbvh_tri_distance_query* __restrict__ queries, uint32_t total,
                                                                    const lbvh_wide_node* __restrict__ wide,
                                                                    const lbvh_fast_node* __restrict__ lines,
                                                                    std::conditional_t<ANY, uint32_t, lbvh_tri_closest>* __restrict__ out,
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

    bool active = false, took = false;
    uint32_t i = 0, skip = kWideEmpty;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
    float lx = 0.0f, ly = 0.0f, lz = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;      // the query's box
    float best = LBVH_MAX_FLOAT, best_s = 0.0f, best_dx = 0.0f, best_dy = 0.0f, best_dz = 0.0f;
    uint32_t best_tri = 0, best_edge = 0, sp = 0, node = 0;
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently wrong record: report it, as the ray walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    float4 qa, qb, qc;
                    active = load_tri_distance_query<ANY>(queries, k, qa, qb, qc, best, out);
                    ax = qa.x; ay = qa.y; az = qa.z; skip = __float_as_uint(qa.w);
                    bx = qb.x; by = qb.y; bz = qb.z;
                    cx = qc.x; cy = qc.y; cz = qc.z;
                    lx = fminf(fminf(ax, bx), cx); ly = fminf(fminf(ay, by), cy); lz = fminf(fminf(az, bz), cz);
                    hx = fmaxf(fmaxf(ax, bx), cx); hy = fmaxf(fmaxf(ay, by), cy); hz = fmaxf(fmaxf(az, bz), cz);
                    best_tri = 0; best_edge = 0; best_s = 0.0f; best_dx = 0.0f; best_dy = 0.0f; best_dz = 0.0f; took = false;
                    sp = 0; node = 0;
                    if (STATS && active) n_queries++;
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
#define BOX2Q(c) box_box2(lox.c, loy.c, loz.c, hix.c, hiy.c, hiz.c, lx, ly, lz, hx, hy, hz)
            const float b0 = BOX2Q(x), b1 = BOX2Q(y), b2 = BOX2Q(z), b3 = BOX2Q(w);
#undef BOX2Q
            const bool h0 = !(b0 > best) && ref.x != kWideEmpty, h1 = !(b1 > best) && ref.y != kWideEmpty;
            const bool h2 = !(b2 > best) && ref.z != kWideEmpty, h3 = !(b3 > best) && ref.w != kWideEmpty;
            // leaf slots first: a lane's leaves one after the other, every lane's k-th at the same time
            uint32_t leaves = (h0 && (ref.x >> 31) ? 1u : 0u) | (h1 && (ref.y >> 31) ? 2u : 0u) | (h2 && (ref.z >> 31) ? 4u : 0u) |
                              (h3 && (ref.w >> 31) ? 8u : 0u);
            bool found = false;                          // ANY: a candidate was accepted
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                const uint32_t tri = __float_as_uint(v0.w);
                if (tri == skip) continue;
                if (STATS) n_tris++;
                uint32_t edge = 0u;
                float s = 0.0f, u = 0.0f, v = 0.0f;
                const float dist2 = triangle_triangle2(ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, edge, s, u, v);
                const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                // best starts at R and best_tri at 0: dist2 == R is never taken.  Ties go to the lower triangle index.
                if (!(dist2 < own) && (dist2 < best || (dist2 == best && tri < best_tri))) {
                    if constexpr (ANY) { found = true; break; }
                    else {
                        best = dist2; best_tri = tri; best_edge = edge; best_s = s; took = true;
                        // delta: the residual of point_triangle2 at x = P + D*s of the winning test, turned round for a scene edge
                        // (m >= 3) so that it points from the scene triangle to the query; 0 where pierced.  The three lines below must
                        // stay operation for operation what segment_query_wide_kernel forms its delta with — x = o + h*s, ap = x - a,
                        // rv = ap - (e1*u + e2*v), step 3 of the header, on the (u, v) segment_triangle2 returned —: relation (c)
                        // promises the same words
                        ray_t seg;
                        float4 p, f1, f2;
                        triangle_edge_test(edge & 7u, ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, seg, p, f1, f2);
                        const float apx = (seg.ox + seg.dx * s) - p.x, apy = (seg.oy + seg.dy * s) - p.y, apz = (seg.oz + seg.dz * s) - p.z;
                        const float rx = apx - (f1.x * u + f2.x * v), ry = apy - (f1.y * u + f2.y * v), rz = apz - (f1.z * u + f2.z * v);
                        const bool pierced = (edge & 8u) != 0u, turn = (edge & 7u) >= 3u;
                        best_dx = pierced ? 0.0f : (turn ? -rx : rx);
                        best_dy = pierced ? 0.0f : (turn ? -ry : ry);
                        best_dz = pierced ? 0.0f : (turn ? -rz : rz);
                    }
                }
            }
            if (ANY && found) {
                if constexpr (ANY) out[i] = 1u;
                active = false;
                continue;
            }
            // nodes to enter, ordered by box distance as in point_query_wide_kernel: the distance's bit pattern with the slot number
            // in its two lowest bits; compared with `best` once more, which may have shrunk in the leaf loop
            constexpr uint32_t none = 0xFFFFFFFFu;
            uint32_t k0 = h0 && !(ref.x >> 31) && !(b0 > best) ? ((__float_as_uint(b0) & ~3u) | 0u) : none;
            uint32_t k1 = h1 && !(ref.y >> 31) && !(b1 > best) ? ((__float_as_uint(b1) & ~3u) | 1u) : none;
            uint32_t k2 = h2 && !(ref.z >> 31) && !(b2 > best) ? ((__float_as_uint(b2) & ~3u) | 2u) : none;
            uint32_t k3 = h3 && !(ref.w >> 31) && !(b3 > best) ? ((__float_as_uint(b3) & ~3u) | 3u) : none;
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
                if constexpr (ANY) out[i] = 0u;
                else {
                    float4* rec = reinterpret_cast<float4*>(out) + 2 * (size_t)i;
                    rec[0] = make_float4(took ? best : LBVH_MAX_FLOAT, __uint_as_float(best_tri), __uint_as_float(best_edge), best_s);
                    rec[1] = make_float4(best_dx, best_dy, best_dz, __uint_as_float(0u));
                }
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- triangle proximity: every triangle within a distance of a triangle (lbvh_triangle_gather_within_distance, include/lbvh.h). --
// The frame of shape_overlap_wide_kernel / capsule_contact_wide_kernel — nothing shrinks, so there is no nearest-first order: every
// passing inner slot is pushed — with triangle_distance_wide_kernel's query, box2q against the fixed bound R for the four slots and
// triangle_triangle2 at a leaf slot, after `skip`.

// delta of a listed pair: a COPY of the lines triangle_distance_wide_kernel forms its record's delta with — sharing one function
// between the two kernels changed that kernel's instructions, which this file's existing kernels must keep —: the residual of
// point_triangle2 at x = P + D*s of the winning test, turned round for a scene edge (m >= 3) so that it points from the scene triangle
// to the query; 0 where pierced.  The three lines must stay operation for operation those: relation (b) of
// lbvh_triangle_gather_within_distance promises the closest call's words.
__device__ __forceinline__ void triangle_pair_delta(uint32_t edge, float s, float u, float v, float ax, float ay, float az, float bx, float by,
                                                    float bz, float cx, float cy, float cz, const float4 v0, const float4 v1, const float4 v2,
                                                    float& dx, float& dy, float& dz)
{
    ray_t seg;
    float4 p, f1, f2;
    triangle_edge_test(edge & 7u, ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, seg, p, f1, f2);
    const float apx = (seg.ox + seg.dx * s) - p.x, apy = (seg.oy + seg.dy * s) - p.y, apz = (seg.oz + seg.dz * s) - p.z;
    const float rx = apx - (f1.x * u + f2.x * v), ry = apy - (f1.y * u + f2.y * v), rz = apz - (f1.z * u + f2.z * v);
    const bool pierced = (edge & 8u) != 0u, turn = (edge & 7u) >= 3u;
    dx = pierced ? 0.0f : (turn ? -rx : rx);
    dy = pierced ? 0.0f : (turn ? -ry : ry);
    dz = pierced ? 0.0f : (turn ? -rz : rz);
}

// the header's active rule of a triangle distance query {a, skip | b, max_dist2 | c, _pad}, false for a NaN radius or coordinate: a
// copy of load_tri_distance_query's condition (that function also writes the closest call's none-record, and taking the condition
// out of it changed triangle_distance_wide_kernel's instructions)
__device__ __forceinline__ bool tri_distance_query_active(const float4 qa, const float4 qb, const float4 qc)
{
    const float inf = __builtin_inff();
    return qb.w > 0.0f && fabsf(qa.x) < inf && fabsf(qa.y) < inf && fabsf(qa.z) < inf && fabsf(qb.x) < inf && fabsf(qb.y) < inf &&
           fabsf(qb.z) < inf && fabsf(qc.x) < inf && fabsf(qc.y) < inf && fabsf(qc.z) < inf;
}

// The one decision of both walks: the pair's record values, and whether the triangle is a candidate (the closest call's predicate
// against the fixed R; `own` is box2q of the leaf slot's box).  Count and fill call it on the same values.
__device__ __forceinline__ bool triangle_proximity_of(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                                      const float4 v0, const float4 v1, const float4 v2, float own, float R, float& dist2,
                                                      uint32_t& edge, float& s, float& u, float& v)
{
    dist2 = triangle_triangle2(ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, edge, s, u, v);
    return dist2 < R && !(dist2 < own);                  // both false for a NaN
}

// FILL false: the candidates of query k are counted into counts[k] (0 for an inactive query).  FILL true: the lane starts at
// offsets[k] and writes {dist2, tri, edge, s | delta, 0} as two 16-byte stores per candidate, never at or beyond the capacity.
template <bool FILL, bool STATS>
__global__ __launch_bounds__(64) void triangle_proximity_wide_kernel(const lbvh_tri_distance_query* __restrict__ queries, uint32_t total,
                                                                     const lbvh_wide_node* __restrict__ wide,
                                                                     const lbvh_fast_node* __restrict__ lines,
                                                                     uint32_t* __restrict__ counts,            // !FILL: candidates of query k
                                                                     const uint64_t* __restrict__ offsets,     // FILL: where segment k starts
                                                                     lbvh_tri_closest* __restrict__ out,       // FILL: the records
                                                                     uint64_t capacity,                        // FILL: records in `out`
                                                                     uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                                     uint32_t lds_depth,              // <= kWideStackLds
                                                                     uint32_t deep_cap,               // <= kWideStackDeep
                                                                     uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    float4* records = reinterpret_cast<float4*>(out);
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_queries = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0, skip = kWideEmpty;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
    float lx = 0.0f, ly = 0.0f, lz = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f;      // the query's box
    float R = 0.0f;
    uint32_t n_found = 0, sp = 0, node = 0;
    uint64_t pos = 0;                                    // FILL: where this lane's next record goes
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float4 qa = reinterpret_cast<const float4*>(queries)[3 * (size_t)k];
                    const float4 qb = reinterpret_cast<const float4*>(queries)[3 * (size_t)k + 1];
                    const float4 qc = reinterpret_cast<const float4*>(queries)[3 * (size_t)k + 2];
                    active = tri_distance_query_active(qa, qb, qc);
                    R = fminf(qb.w, LBVH_MAX_FLOAT);
                    ax = qa.x; ay = qa.y; az = qa.z; skip = __float_as_uint(qa.w);
                    bx = qb.x; by = qb.y; bz = qb.z;
                    cx = qc.x; cy = qc.y; cz = qc.z;
                    lx = fminf(fminf(ax, bx), cx); ly = fminf(fminf(ay, by), cy); lz = fminf(fminf(az, bz), cz);
                    hx = fmaxf(fmaxf(ax, bx), cx); hy = fmaxf(fmaxf(ay, by), cy); hz = fmaxf(fmaxf(az, bz), cz);
                    sp = 0; node = 0;
                    if constexpr (FILL) { if (active) pos = offsets[k]; }
                    else { n_found = 0; if (!active) counts[k] = 0u; }
                    if (STATS && active) n_queries++;
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
#define BOX2Q(c) box_box2(lox.c, loy.c, loz.c, hix.c, hiy.c, hiz.c, lx, ly, lz, hx, hy, hz)
            const float b0 = BOX2Q(x), b1 = BOX2Q(y), b2 = BOX2Q(z), b3 = BOX2Q(w);
#undef BOX2Q
            // entered iff box2q < R: false for a NaN
            const bool h0 = b0 < R && ref.x != kWideEmpty, h1 = b1 < R && ref.y != kWideEmpty;
            const bool h2 = b2 < R && ref.z != kWideEmpty, h3 = b3 < R && ref.w != kWideEmpty;
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                float4 v0, v1, v2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[pick4(ref, k) & 0x7FFFFFFFu]), v0, v1, v2);
                const uint32_t tri = __float_as_uint(v0.w);
                if (tri == skip) continue;
                if (STATS) n_tris++;
                const float own = k == 0u ? b0 : (k == 1u ? b1 : (k == 2u ? b2 : b3));
                uint32_t edge = 0u;
                float dist2 = 0.0f, s = 0.0f, u = 0.0f, v = 0.0f;
                if (!triangle_proximity_of(ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, own, R, dist2, edge, s, u, v)) continue;
                if constexpr (FILL) {
                    if (pos < capacity) {                        // never a record at or beyond the capacity
                        float dx, dy, dz;
                        triangle_pair_delta(edge, s, u, v, ax, ay, az, bx, by, bz, cx, cy, cz, v0, v1, v2, dx, dy, dz);
                        records[2 * pos] = make_float4(dist2, __uint_as_float(tri), __uint_as_float(edge), s);
                        records[2 * pos + 1] = make_float4(dx, dy, dz, __uint_as_float(0u));
                    }
                    pos++;
                } else n_found++;
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
    if (STATS) add_ray_stats(stats, n_queries, n_steps, n_tris);
}

// ---- box contacts: how deep an oriented box is in each triangle it touches, and which way out (lbvh_obb_contacts, ------------
// lbvh_obb_deepest, include/lbvh.h).  The frame and the slot test of shape_overlap_wide_kernel<kShapeObb>; the count walk of
// lbvh_obb_contacts IS that kernel's kTriCount form.  The two forms are capsule_contact_wide_kernel's.

// The header's contact of a box (centre c, half-axis vectors b) with the triangle line (a, e1, e2); false: not a candidate.  The
// decision is box_touches' on the same values — lo <= rb && -rb <= hi on every axis from the same box_axis_spans, the first
// separating axis ends the loop (through its condition, as capsule_contact_of) —, and the same pass keeps the least d_j = pen / len
// over the axes that count.  Per counting axis one square root and one division; the winner's sign * L, len and far are kept
// and its four other quotients are formed once, after the loop.  rec0 = {depth, tri (set by the caller), axis, back},
// rec1 = {normal, 0}.
__device__ __forceinline__ bool box_contact_of(const ray_t& c, const box_axes& b, const float4 a, const float4 e1, const float4 e2,
                                               float4& rec0, float4& rec1)
{
    const float inf = __builtin_inff();
    const float mx = a.x - c.ox, my = a.y - c.oy, mz = a.z - c.oz;
    const float e3x = e2.x - e1.x, e3y = e2.y - e1.y, e3z = e2.z - e1.z;
    float least = inf, win_len = 1.0f, win_far = 0.0f, wx = 0.0f, wy = 0.0f, wz = 0.0f;
    uint32_t axis = LBVH_BOX_AXIS_START;
    bool apart = false;
#pragma nounroll
    for (uint32_t j = 0; j < 13u && !apart; j++) {
        float lx, ly, lz, lo, hi, rb;
        box_axis_spans(j, mx, my, mz, b, e1, e2, e3x, e3y, e3z, lx, ly, lz, lo, hi, rb);
        apart = !(lo <= rb && -rb <= hi);
        const float len2 = dot3(lx, ly, lz, lx, ly, lz);
        if (len2 >= 1.17549435e-38f && len2 < inf) {         // a normal finite number: a zero or denormal axis does not count
            const float pos = hi + rb, neg = rb - lo;        // the push along +L and along -L
            const float len = sqrtf(len2);
            const float d = fminf(pos, neg) / len;
            if (d < least) {                                 // strictly less; false for a NaN
                least = d; axis = j; win_len = len; win_far = fmaxf(pos, neg);
                const bool up = pos <= neg;
                wx = up ? lx : -lx; wy = up ? ly : -ly; wz = up ? lz : -lz;
            }
        }
    }
    if (apart) return false;
    const bool none = axis == LBVH_BOX_AXIS_START;
    rec0.x = none ? 0.0f : least;
    rec0.z = __uint_as_float(axis);
    rec0.w = none ? 0.0f : win_far / win_len;
    rec1 = make_float4(wx / win_len, wy / win_len, wz / win_len, 0.0f);     // (none: 0 / 1)
    return true;
}

template <int MODE, bool STATS>
__global__ __launch_bounds__(64) void box_contact_wide_kernel(const lbvh_obb* __restrict__ boxes, uint32_t total,
                                                              const lbvh_wide_node* __restrict__ wide,
                                                              const lbvh_fast_node* __restrict__ lines,
                                                              const uint64_t* __restrict__ offsets,     // kContactFill: where segment k starts
                                                              lbvh_box_contact* __restrict__ out,       // kContactFill: the records; kContactDeepest: one per shape
                                                              uint64_t capacity,                        // kContactFill: records in `out`
                                                              uint32_t* __restrict__ deep,     // [gridDim.x][kWideStackDeep][64]
                                                              uint32_t lds_depth,              // <= kWideStackLds
                                                              uint32_t deep_cap,               // <= kWideStackDeep
                                                              uint32_t* __restrict__ fault, lbvh_ray_stats* stats)
{
    __shared__ uint32_t s_stack[kWideStackLds][LBVH_WAVE];
    uint32_t* my_deep = deep + (size_t)blockIdx.x * (kWideStackDeep * LBVH_WAVE) + threadIdx.x;
    const float4* shapes = reinterpret_cast<const float4*>(boxes);
    float4* records = reinterpret_cast<float4*>(out);
    const uint32_t lane = threadIdx.x;
    const uint32_t run = max((total + gridDim.x - 1) / gridDim.x, 32u);
    uint32_t next = blockIdx.x * run;
    if (next >= total) return;
    const uint32_t end = min(next + run, total);
    uint32_t n_shapes = 0, n_steps = 0, n_tris = 0;

    bool active = false;
    uint32_t i = 0;
    ray_t o = {};                                        // the centre (the direction is not read)
    box_axes b = {};                                     // the half-axis vectors
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;               // g, the half extent per world axis
    uint32_t sp = 0, node = 0;
    uint64_t pos = 0;                                    // kContactFill: where this lane's next record goes
    float4 best0 = {}, best1 = {};                       // kContactDeepest: the deepest record so far
    const float4 none0 = make_float4(0.0f, __uint_as_float(LBVH_NULL), 0.0f, 0.0f), none1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto push = [&](uint32_t ref) {
        if (sp < lds_depth) { s_stack[sp][lane] = ref; sp++; }
        else if (sp < lds_depth + deep_cap) { my_deep[(sp - lds_depth) * LBVH_WAVE] = ref; sp++; }
        // a dropped entry would be a silently short list: report it, as the other walkers do (lbvh_debug_ray_stack_limit provokes it)
        else __hip_atomic_store(fault, LBVH_FAULT_RAY_STACK, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    for (;;) {
        const uint64_t idle = __ballot(!active);
        if (idle != 0 && next < end) {
            if (!active) {
                const uint32_t k = next + mbcnt64(idle);
                if (k < end) {
                    i = k;
                    const float inf = __builtin_inff();
                    const float4 q0 = shapes[4 * (size_t)k], x = shapes[4 * (size_t)k + 1], y = shapes[4 * (size_t)k + 2], z = shapes[4 * (size_t)k + 3];
                    o.ox = q0.x; o.oy = q0.y; o.oz = q0.z;
                    b.xx = x.x; b.xy = x.y; b.xz = x.z;
                    b.yx = y.x; b.yy = y.y; b.yz = y.z;
                    b.zx = z.x; b.zy = z.y; b.zz = z.z;
                    hx = (fabsf(b.xx) + fabsf(b.yx)) + fabsf(b.zx);
                    hy = (fabsf(b.xy) + fabsf(b.yy)) + fabsf(b.zy);
                    hz = (fabsf(b.xz) + fabsf(b.yz)) + fabsf(b.zz);
                    const float det = dot3(x.x, x.y, x.z, y.y * z.z - y.z * z.y, y.z * z.x - y.x * z.z, y.x * z.y - y.y * z.x);
                    active = (q0.x == q0.x && q0.y == q0.y && q0.z == q0.z) &&
                             fabsf(x.x) < inf && fabsf(x.y) < inf && fabsf(x.z) < inf && fabsf(y.x) < inf && fabsf(y.y) < inf && fabsf(y.z) < inf &&
                             fabsf(z.x) < inf && fabsf(z.y) < inf && fabsf(z.z) < inf && fabsf(det) < inf && det != 0.0f;
                    sp = 0; node = 0;
                    if constexpr (MODE == kContactFill) { if (active) pos = offsets[k]; }
                    else {
                        best0 = none0; best1 = none1;
                        if (!active) { records[2 * (size_t)k] = none0; records[2 * (size_t)k + 1] = none1; }
                    }
                    if (STATS && active) n_shapes++;
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
#define SHAPE_SLOT(c)                                                                                                                  \
    (shape_in_grown<kShapeObb>(lox.c, hix.c, o.ox, hx, hx, 0.0f) && shape_in_grown<kShapeObb>(loy.c, hiy.c, o.oy, hy, hy, 0.0f) &&    \
     shape_in_grown<kShapeObb>(loz.c, hiz.c, o.oz, hz, hz, 0.0f) && ref.c != kWideEmpty)
            const bool h0 = SHAPE_SLOT(x), h1 = SHAPE_SLOT(y), h2 = SHAPE_SLOT(z), h3 = SHAPE_SLOT(w);
#undef SHAPE_SLOT
            const uint32_t hit = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
            const uint32_t leaf = (ref.x >> 31) | ((ref.y >> 31) << 1) | ((ref.z >> 31) << 2) | ((ref.w >> 31) << 3);
            uint32_t leaves = hit & leaf, inner = hit & ~leaf;
            while (leaves != 0u) {
                const uint32_t k = (uint32_t)__builtin_ctz(leaves);
                leaves &= leaves - 1u;
                const uint32_t line = pick4(ref, k) & 0x7FFFFFFFu;
                float4 t0, t1, t2;
                unpack_fast_triangle(reinterpret_cast<const float4*>(&lines[line]), t0, t1, t2);
                if (STATS) n_tris++;
                float4 rec0, rec1;
                rec0.y = t0.w;                                   // the ORIGINAL triangle index
                if (!box_contact_of(o, b, t0, t1, t2, rec0, rec1)) continue;
                if constexpr (MODE == kContactFill) {
                    if (pos < capacity) { records[2 * pos] = rec0; records[2 * pos + 1] = rec1; }     // never a record at or beyond the capacity
                    pos++;
                } else {
                    // the greatest depth; on equal depth the lower original index (the none-record's index is above every one)
                    const uint32_t tri = __float_as_uint(rec0.y), best_tri = __float_as_uint(best0.y);
                    if (best_tri == LBVH_NULL || rec0.x > best0.x || (!(rec0.x < best0.x) && tri < best_tri)) { best0 = rec0; best1 = rec1; }
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
                if constexpr (MODE == kContactDeepest) { records[2 * (size_t)i] = best0; records[2 * (size_t)i + 1] = best1; }
                active = false;
            }
        }
    }
    if (STATS) add_ray_stats(stats, n_shapes, n_steps, n_tris);
}

// ---- bounce ----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t pcg_hash(uint32_t v)
{
    const uint32_t state = v * 747796405u + 2891336453u;
    const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
    return (word >> 22u) ^ word;
}

__device__ __forceinline__ float path_rnd(uint32_t seed, uint32_t index, uint32_t bounce, uint32_t draw)
{
    const uint32_t h = pcg_hash(pcg_hash(pcg_hash(seed + 0x9E3779B9u * index) + bounce) + draw);
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// one path's bounce; returns true when the path goes on
// MARK (lbvh_path_bounce, which owns the hit records between its calls): a path that ends leaves a DEAD record in
// hits[i] (t = MAX_FLOAT, triangle 0xFFFFFFFF), and a later bounce that finds it skips the path without touching its
// 64-byte state — after the first bounce most of a frame's paths are dead.
// FIRST (lbvh_path_first_bounce): the path state is not read but MADE here from the camera, as path_begin_kernel would
// have written it: the 132 MB of initial states of a 1080p frame are neither stored by one kernel nor loaded by the next.
template <bool MARK, bool FIRST>
__device__ __forceinline__ bool scatter_path(const lbvh_triangle* __restrict__ triangles, const lbvh_hit* hits, size_t i,
                                             uint32_t bounce, uint32_t seed, float albedo, lbvh_path_state* __restrict__ states,
                                             const lbvh_camera& cam);

// LIST: also append the indices of the paths that go on, so that the next segment is traced without a separate pass over
// all path states.  A workgroup handles kScatterItems x 256 paths and reserves its run of the list with ONE global atomic:
// with one path per thread the 8 100 workgroups of a 1080p frame queued on that one counter for most of the kernel's
// 67 - 91 us (the bounces' own work shrinks with the live paths, the kernel's time did not).
constexpr int kScatterItems = 8;
constexpr int kScatterItemsList = 2;       // ... when the paths come from a live list (see path_scatter_kernel)
// DOMAIN (round 5): the paths to look at are the `*n_domain` entries of `domain` — the list of live paths the previous bounce
// left behind — instead of all `count` pixels (domain == nullptr): from the second bounce on a scatter then costs what its live
// paths cost, not a pass over 2 M hit records of which most are dead (1080p: 35 / 33 / 33 us for bounces 2, 3 and the frame's last
// scatter -> 27 / 18 / 14 us).
// ITEMS paths per thread, one after the other (each item's ballot closes its chain of dependent loads): 8 for a pass over every
// pixel — few workgroups, one list reservation each —, 2 when the domain is a list of live paths: there the kernel is the latency
// of a thread's items in sequence (8 items: 32 us however few paths are live), not the reservation
template <bool LIST, bool FIRST = false, int ITEMS = kScatterItems>
__global__ __launch_bounds__(256) void path_scatter_kernel(const lbvh_triangle* __restrict__ triangles,
                                                           const lbvh_hit* hits, size_t count, uint32_t bounce,
                                                           uint32_t seed, float albedo, lbvh_path_state* __restrict__ states,
                                                           uint32_t* __restrict__ n_alive, uint32_t* __restrict__ list, lbvh_camera cam,
                                                           const uint32_t* __restrict__ domain, const uint32_t* __restrict__ n_domain)
{
    __shared__ uint32_t s_n, s_base;
    const size_t i0 = (size_t)blockIdx.x * (256 * ITEMS) + threadIdx.x;
    const size_t total = domain ? (size_t)*n_domain : count;
    if ((size_t)blockIdx.x * (256 * ITEMS) >= total) return;          // (uniform) nothing of the domain falls to this workgroup
    if (LIST) {
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
    }
    uint32_t ofs[ITEMS];                      // position inside this wave's run, or ~0u: the path ended
    uint32_t idx[ITEMS];                      // the path (pixel) index of item k
    uint32_t wave_n = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; k++) {
        const size_t at = i0 + (size_t)k * 256;
        const size_t i = at < total ? (domain ? (size_t)domain[at] : at) : 0;
        idx[k] = (uint32_t)i;
        const bool on = at < total && scatter_path<LIST, FIRST>(triangles, hits, i, bounce, seed, albedo, states, cam);
        if (LIST) {
            const uint64_t m = __ballot(on);
            ofs[k] = on ? wave_n + mbcnt64(m) : 0xFFFFFFFFu;
            wave_n += (uint32_t)__popcll(m);
        }
    }
    if (LIST) {
        uint32_t wave_base = 0;
        if (lane_id() == 0 && wave_n) wave_base = atomicAdd(&s_n, wave_n);
        wave_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_base);
        __syncthreads();
        if (threadIdx.x == 0 && s_n) s_base = __hip_atomic_fetch_add(n_alive, s_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ITEMS; k++)
            if (ofs[k] != 0xFFFFFFFFu) list[s_base + wave_base + ofs[k]] = idx[k];
    }
}

template <bool MARK, bool FIRST>
__device__ __forceinline__ bool scatter_path(const lbvh_triangle* __restrict__ triangles, const lbvh_hit* hits, size_t i,
                                             uint32_t bounce, uint32_t seed, float albedo, lbvh_path_state* __restrict__ states,
                                             const lbvh_camera& cam)
{
    const float4 h = reinterpret_cast<const float4*>(hits)[i];
    const bool missed = !(h.x < LBVH_MAX_FLOAT);
    // ended in an earlier bounce: only lbvh_path_bounce writes DEAD records, so at bounce 0 a {MAX_FLOAT, 0xFFFFFFFF} record is
    // the caller's own fill value (an untraced pixel) and is an ordinary miss, as in lbvh_path_scatter
    if (MARK && bounce > 0u && missed && __float_as_uint(h.y) == 0xFFFFFFFFu) return false;
    float4* st = reinterpret_cast<float4*>(&states[i]);
    float4 o, d, thr, rad;
    if (FIRST) {                     // path_begin_kernel's state for pixel i, not read but made
        const uint32_t py = (uint32_t)(i / (size_t)cam.screen_width), px = (uint32_t)(i - (size_t)py * cam.screen_width);
        const ray_t r = make_ray(cam, px, py);
        o = make_float4(r.ox, r.oy, r.oz, __uint_as_float(1u));
        d = make_float4(r.dx, r.dy, r.dz, 0.0f);
        thr = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
        rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        o = st[0];
        if (__float_as_uint(o.w) == 0u) return false;
        d = st[1]; thr = st[2]; rad = st[3];
    }
    if (missed) {
        const float sk = 0.5f * (d.y + 1.0f);
        rad.x = rad.x + thr.x * ((1.0f - sk) * 1.0f + sk * 0.5f);
        rad.y = rad.y + thr.y * ((1.0f - sk) * 1.0f + sk * 0.7f);
        rad.z = rad.z + thr.z * ((1.0f - sk) * 1.0f + sk * 1.0f);
        o.w = __uint_as_float(0u);
        st[0] = o;
        st[3] = rad;
        if (FIRST) { st[1] = d; st[2] = thr; }
        if (MARK) reinterpret_cast<float4*>(const_cast<lbvh_hit*>(hits))[i] = make_float4(LBVH_MAX_FLOAT, __uint_as_float(0xFFFFFFFFu), 0.0f, 0.0f);
        return false;
    }
    if (bounce == 0) rad.w = 1.0f;
    const float4* tp = reinterpret_cast<const float4*>(&triangles[__float_as_uint(h.y)]);
    const float4 a = tp[0], b = tp[1], c = tp[2];
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
    const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float nl = sqrtf(dot3(nx, ny, nz, nx, ny, nz));
    if (nl > 0.0f) { nx = nx / nl; ny = ny / nl; nz = nz / nl; } else { nx = 0.0f; ny = 1.0f; nz = 0.0f; }
    if (dot3(nx, ny, nz, d.x, d.y, d.z) > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    o.x = o.x + d.x * h.x; o.y = o.y + d.y * h.x; o.z = o.z + d.z * h.x;
    thr.x = thr.x * albedo; thr.y = thr.y * albedo; thr.z = thr.z * albedo;
    // uniform point on the unit sphere, Marsaglia 1972, at most 8 tries
    float px = 0.0f, py = 0.0f, pz = 1.0f;
    for (uint32_t k = 0; k < 16; k += 2) {
        const float x1 = 2.0f * path_rnd(seed, (uint32_t)i, bounce, k) - 1.0f;
        const float x2 = 2.0f * path_rnd(seed, (uint32_t)i, bounce, k + 1) - 1.0f;
        const float ss = x1 * x1 + x2 * x2;
        if (ss < 1.0f) {
            const float r = sqrtf(1.0f - ss);
            px = 2.0f * x1 * r; py = 2.0f * x2 * r; pz = 1.0f - 2.0f * ss;
            break;
        }
    }
    float vx = nx + px, vy = ny + py, vz = nz + pz;
    const float dl = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
    if (dl > 1e-6f) { vx = vx / dl; vy = vy / dl; vz = vz / dl; } else { vx = nx; vy = ny; vz = nz; }
    d.x = vx; d.y = vy; d.z = vz;
    st[0] = o; st[1] = d; st[2] = thr; st[3] = rad;
    return true;
}

__global__ __launch_bounds__(256) void path_resolve_kernel(const lbvh_path_state* __restrict__ states, size_t count,
                                                           uint16_t* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float4 rad = reinterpret_cast<const float4*>(&states[i])[3];
    ushort4 o;
    o.x = __half_as_ushort(__float2half_rn(rad.x));
    o.y = __half_as_ushort(__float2half_rn(rad.y));
    o.z = __half_as_ushort(__float2half_rn(rad.z));
    o.w = __half_as_ushort(__float2half_rn(rad.w));
    reinterpret_cast<ushort4*>(out)[i] = o;
}

}  // namespace

static_assert(sizeof(lbvh_path_state) == 64, "path state must be 64 bytes");

// the walk over the live rays of `list` (or over plain rays, PLAIN: `total` is their count): four-wide nodes (made on first use
// after a rebuild) — few_rays: with the kernel that keeps two fetches of a step in flight (the later bounces of a frame) —, or the
// binary nodes the packet walk uses (lbvh_debug_ray_walker(ctx, 0): the cross-check of the tests; 2: the few-rays kernel for every launch)
template <bool PLAIN, int Q>
static lbvh_status launch_ray_walk(lbvh_context* ctx, const walk_src<PLAIN>* d_states, walk_total<PLAIN> n_alive, const uint32_t* list,
                                   float t_min, walk_out<Q>* d_hits, walk_launch w, bool few_rays = false)
{
    if (ctx->ray_walker != 0u) {
        const lbvh_status wrc = use_wide_nodes(ctx, &w);
        if (wrc != LBVH_OK) return wrc;
        lbvh_ray_stats* st = ctx->ray_stats;
        if (few_rays || ctx->ray_walker == 2u)
            LBVH_LAUNCH_STATS(ctx, st, (trace_rays_wide_chain_kernel<PLAIN, Q, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_states, n_alive, list, t_min,
                              w.wn, ctx->fast_nodes, d_hits, w.deep, w.lds, w.deep_cap, ctx->fault_dev, st);
        else
            LBVH_LAUNCH_STATS(ctx, st, (trace_rays_wide_kernel<PLAIN, Q, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_states, n_alive, list, t_min,
                              w.wn, ctx->fast_nodes, d_hits, w.deep, w.lds, w.deep_cap, ctx->fault_dev, st);
    } else {
        LBVH_LAUNCH(ctx, (trace_rays_kernel<PLAIN, Q>), dim3(w.waves), dim3(LBVH_WAVE), d_states, n_alive, list, t_min, ctx->fast_nodes,
                    ctx->fast_tris, d_hits, w.deep, ctx->ray_stack_lds, std::min<uint32_t>(ctx->ray_stack_deep, kRayStackDeep), ctx->fault_dev);
    }
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

// lbvh_trace_closest / lbvh_trace_occluded / lbvh_count_hits: plain rays by direct index, no live-ray list
template <int Q>
static lbvh_status trace_plain_rays(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene,
                                    walk_out<Q>* d_out, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_rays != nullptr && h_scene != nullptr && d_out != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_rays & 15) == 0 && ((uintptr_t)d_out & (Q != kClosest ? 3 : 15)) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, false, &w);
    if (rc != LBVH_OK) return rc;
    return launch_ray_walk<true, Q>(ctx, d_rays, (uint32_t)count, nullptr, 0.0f, d_out, w);
}

// lbvh_closest_point_query / lbvh_within_distance
template <bool ANY>
static lbvh_status point_queries(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                 std::conditional_t<ANY, uint32_t, lbvh_closest_point>* d_out, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_queries != nullptr && h_scene != nullptr && d_out != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_out & (ANY ? 3 : 15)) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    PER_QUERY_WALK(point_query_wide_kernel, d_queries, d_out);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

// lbvh_segment_closest_point / lbvh_segment_within_distance and lbvh_triangle_closest_point / lbvh_triangle_within_distance: the
// point queries' checks on 32- or 48-byte queries and 32-byte records
template <bool ANY, class QUERY, class OUT>
static lbvh_status distance_queries(lbvh_context* ctx, const QUERY* d_queries, size_t count, const lbvh_scene* h_scene, OUT* d_out,
                                    const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_queries != nullptr && h_scene != nullptr && d_out != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_out & (ANY ? 3 : 15)) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    if constexpr (std::is_same_v<QUERY, lbvh_segment_query>) PER_QUERY_WALK(segment_query_wide_kernel, d_queries, d_out);
    else PER_QUERY_WALK(triangle_distance_wide_kernel, d_queries, d_out);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

// lbvh_sphere_cast / lbvh_sphere_cast_any (CAST = lbvh_sphere_ray), lbvh_capsule_cast / lbvh_capsule_cast_any (lbvh_capsule_ray),
// lbvh_box_cast / lbvh_box_cast_any (lbvh_box_ray, HIT = lbvh_box_hit), lbvh_triangle_cast / lbvh_triangle_cast_any (lbvh_tri_ray,
// lbvh_tri_cast_hit).  The box and triangle casts' rejections name the entry point; the sphere and capsule casts keep the text
// they have had.
template <bool ANY, class CAST, class HIT = lbvh_hit>
static lbvh_status shape_casts(lbvh_context* ctx, const CAST* d_casts, size_t count, const lbvh_scene* h_scene,
                               std::conditional_t<ANY, uint32_t, HIT>* d_out, const char* who)
{
#define CAST_REQUIRE(cond)                                                                                        \
    do {                                                                                                          \
        if constexpr (std::is_same_v<CAST, lbvh_box_ray> || std::is_same_v<CAST, lbvh_tri_ray>) NAMED_REQUIRE(cond); \
        else LBVH_REQUIRE(ctx, cond);                                                                             \
    } while (0)
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    CAST_REQUIRE(d_casts != nullptr && h_scene != nullptr && d_out != nullptr);
    CAST_REQUIRE(((uintptr_t)d_casts & 15) == 0 && ((uintptr_t)d_out & (ANY ? 3 : 15)) == 0);
    CAST_REQUIRE(count <= 0xFFFFFFFFull);
#undef CAST_REQUIRE
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    if constexpr (std::is_same_v<CAST, lbvh_sphere_ray>) PER_QUERY_WALK(sphere_cast_wide_kernel, d_casts, d_out);
    else if constexpr (std::is_same_v<CAST, lbvh_capsule_ray>) PER_QUERY_WALK(capsule_cast_wide_kernel, d_casts, d_out);
    else if constexpr (std::is_same_v<CAST, lbvh_box_ray>) PER_QUERY_WALK(box_cast_wide_kernel, d_casts, d_out);
    else PER_QUERY_WALK(triangle_cast_wide_kernel, d_casts, d_out);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

// lbvh_box_overlaps / lbvh_gather_within_distance.  Four-wide walk only.
template <bool BOX>
static lbvh_status overlap_queries(lbvh_context* ctx, const void* d_queries, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                   uint32_t* d_tris, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_queries != nullptr && h_scene != nullptr && d_offsets != nullptr);
    LBVH_REQUIRE(ctx, d_tris != nullptr || capacity == 0);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const float4* q = (const float4*)d_queries;
    const uint32_t total = (uint32_t)count, leaf_base = ctx->fast_capacity;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (overlap_wide_kernel<BOX, false, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes, leaf_base,
                              counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (overlap_wide_kernel<BOX, true, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes, leaf_base,
                              (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_tris, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        });
}

// lbvh_triangle_intersections: a CSR answer; lbvh_triangle_intersects_any: one launch, the flags are the walk's own output.
// Four-wide walk only.
template <bool ANY>
static lbvh_status triangle_queries(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                    uint32_t* d_tris, uint64_t capacity, uint32_t* d_flags, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_queries != nullptr && h_scene != nullptr && (ANY ? d_flags != nullptr : d_offsets != nullptr));
    LBVH_REQUIRE(ctx, d_tris != nullptr || capacity == 0);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0 && ((uintptr_t)d_flags & 3) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const float4* q = (const float4*)d_queries;
    const uint32_t total = (uint32_t)count;
    if constexpr (ANY) {
        LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_query_wide_kernel<kTriAny, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                          d_flags, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        LBVH_HIP_TRY(ctx, hipGetLastError());
        return LBVH_OK;
    } else {
        return csr_query(
            ctx, count, d_offsets, capacity,
            [&](uint32_t* counts) {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_query_wide_kernel<kTriCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                                  counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
            },
            [&] {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_query_wide_kernel<kTriFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                                  (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_tris, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
            });
    }
}

// lbvh_triangle_intersection_segments: triangle_queries<false> with a record in place of an index — the count walk is that
// function's, the fill walk forms the segments.  Four-wide walk only.  (a rejection names the entry point)
static lbvh_status triangle_segments(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                     lbvh_tri_segment* d_segments, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_queries != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_segments != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_segments & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const float4* q = (const float4*)d_queries;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_query_wide_kernel<kTriCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                              counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_segment_wide_kernel<STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                              (const uint64_t*)d_offsets, d_segments, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        });
}

// lbvh_capsule_overlaps / lbvh_obb_overlaps: a CSR answer; lbvh_capsule_overlaps_any / lbvh_obb_overlaps_any: one launch, the
// flags are the walk's own output — triangle_queries with the shape's walk.  Four-wide walk only.  (a rejection names the entry point)
template <int SHAPE, bool ANY>
static lbvh_status shape_overlaps(lbvh_context* ctx, const void* d_shapes, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                  uint32_t* d_tris, uint64_t capacity, uint32_t* d_flags, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_shapes != nullptr && h_scene != nullptr && (ANY ? d_flags != nullptr : d_offsets != nullptr));
    NAMED_REQUIRE(d_tris != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_shapes & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_tris & 3) == 0 && ((uintptr_t)d_flags & 3) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const float4* q = (const float4*)d_shapes;
    const uint32_t total = (uint32_t)count;
    if constexpr (ANY) {
        LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (shape_overlap_wide_kernel<SHAPE, kTriAny, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn, ctx->fast_nodes,
                          d_flags, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        LBVH_HIP_TRY(ctx, hipGetLastError());
        return LBVH_OK;
    } else {
        return csr_query(
            ctx, count, d_offsets, capacity,
            [&](uint32_t* counts) {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (shape_overlap_wide_kernel<SHAPE, kTriCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn,
                                  ctx->fast_nodes, counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                                  ctx->ray_stats);
            },
            [&] {
                LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (shape_overlap_wide_kernel<SHAPE, kTriFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), q, total, w.wn,
                                  ctx->fast_nodes, (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_tris, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                                  ctx->ray_stats);
            });
    }
}

// lbvh_sphere_cast_all / lbvh_capsule_cast_all / lbvh_box_cast_all: a CSR answer of hit records (lbvh_box_hit for the box) —
// lbvh_gather_hits with the shape's walk.  Four-wide walk only.  (a rejection names the entry point)
template <int SHAPE, class HIT>
static lbvh_status cast_gathers(lbvh_context* ctx, const cast_ray<SHAPE>* d_casts, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                HIT* d_hits, uint64_t capacity, const char* who)
{
    static_assert(sizeof(HIT) == sizeof(float4), "a cast-all record is one float4");
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_casts != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_hits != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_casts & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_hits & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (cast_gather_wide_kernel<SHAPE, false, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_casts, total, w.wn,
                              ctx->fast_nodes, counts, (const uint64_t*)nullptr, (float4*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                              ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (cast_gather_wide_kernel<SHAPE, true, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_casts, total, w.wn,
                              ctx->fast_nodes, (uint32_t*)nullptr, (const uint64_t*)d_offsets, (float4*)d_hits, capacity, w.deep, w.lds, w.deep_cap,
                              ctx->fault_dev, ctx->ray_stats);
        });
}

// lbvh_triangle_cast_all: cast_gathers with the triangle's own kernel (triangle_cast_gather_wide_kernel says why it has one)
static lbvh_status triangle_cast_gathers(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                         lbvh_tri_cast_hit* d_hits, uint64_t capacity, const char* who)
{
    static_assert(sizeof(lbvh_tri_cast_hit) == sizeof(float4), "a cast-all record is one float4");
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_casts != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_hits != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_casts & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_hits & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_cast_gather_wide_kernel<false, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_casts, total, w.wn,
                              ctx->fast_nodes, counts, (const uint64_t*)nullptr, (float4*)nullptr, (uint64_t)0, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                              ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_cast_gather_wide_kernel<true, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_casts, total, w.wn,
                              ctx->fast_nodes, (uint32_t*)nullptr, (const uint64_t*)d_offsets, (float4*)d_hits, capacity, w.deep, w.lds, w.deep_cap,
                              ctx->fault_dev, ctx->ray_stats);
        });
}

// lbvh_capsule_contacts: shape_overlaps<kShapeCapsule, false> with a record in place of an index — the count walk is that
// function's, the fill walk forms the contacts.  lbvh_capsule_deepest: the contact walk's one-record form, one launch.
static lbvh_status capsule_contacts(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                    lbvh_contact* d_contacts, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_shapes != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_contacts != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_shapes & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_contacts & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (shape_overlap_wide_kernel<kShapeCapsule, kTriCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE),
                              (const float4*)d_shapes, total, w.wn, ctx->fast_nodes, counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0,
                              w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (capsule_contact_wide_kernel<kContactFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_shapes, total,
                              w.wn, ctx->fast_nodes, (const uint64_t*)d_offsets, d_contacts, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                              ctx->ray_stats);
        });
}

// lbvh_triangle_gather_within_distance: capsule_contacts with the triangle distance query — both walks are
// triangle_proximity_wide_kernel's.  Four-wide walk only.  (a rejection names the entry point)
static lbvh_status triangle_proximity(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                      uint64_t* d_offsets, lbvh_tri_closest* d_records, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_queries != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_records != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_records & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_proximity_wide_kernel<false, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_queries, total,
                              w.wn, ctx->fast_nodes, counts, (const uint64_t*)nullptr, (lbvh_tri_closest*)nullptr, (uint64_t)0, w.deep, w.lds,
                              w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (triangle_proximity_wide_kernel<true, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_queries, total,
                              w.wn, ctx->fast_nodes, (uint32_t*)nullptr, (const uint64_t*)d_offsets, d_records, capacity, w.deep, w.lds, w.deep_cap,
                              ctx->fault_dev, ctx->ray_stats);
        });
}

static lbvh_status capsule_deepest(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene, lbvh_contact* d_out,
                                   const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_shapes != nullptr && h_scene != nullptr && d_out != nullptr);
    NAMED_REQUIRE(((uintptr_t)d_shapes & 15) == 0 && ((uintptr_t)d_out & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (capsule_contact_wide_kernel<kContactDeepest, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_shapes,
                      (uint32_t)count, w.wn, ctx->fast_nodes, (const uint64_t*)nullptr, d_out, (uint64_t)0, w.deep, w.lds, w.deep_cap,
                      ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

// lbvh_obb_contacts / lbvh_obb_deepest: capsule_contacts / capsule_deepest for the box — the count walk is
// shape_overlaps<kShapeObb, false>'s, the fill walk forms the contacts; one record per shape from the contact walk's one-record form.
static lbvh_status obb_contacts(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene, uint64_t* d_offsets,
                                lbvh_box_contact* d_contacts, uint64_t capacity, const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_shapes != nullptr && h_scene != nullptr && d_offsets != nullptr);
    NAMED_REQUIRE(d_contacts != nullptr || capacity == 0);
    NAMED_REQUIRE(((uintptr_t)d_shapes & 15) == 0 && ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_contacts & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    const uint32_t total = (uint32_t)count;
    return csr_query(
        ctx, count, d_offsets, capacity,
        [&](uint32_t* counts) {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (shape_overlap_wide_kernel<kShapeObb, kTriCount, STATS>), dim3(w.waves), dim3(LBVH_WAVE),
                              (const float4*)d_shapes, total, w.wn, ctx->fast_nodes, counts, (const uint64_t*)nullptr, (uint32_t*)nullptr, (uint64_t)0,
                              w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
        },
        [&] {
            LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (box_contact_wide_kernel<kContactFill, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_shapes, total,
                              w.wn, ctx->fast_nodes, (const uint64_t*)d_offsets, d_contacts, capacity, w.deep, w.lds, w.deep_cap, ctx->fault_dev,
                              ctx->ray_stats);
        });
}

static lbvh_status obb_deepest(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene, lbvh_box_contact* d_out,
                               const char* who)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    NAMED_REQUIRE(d_shapes != nullptr && h_scene != nullptr && d_out != nullptr);
    NAMED_REQUIRE(((uintptr_t)d_shapes & 15) == 0 && ((uintptr_t)d_out & 15) == 0);
    NAMED_REQUIRE(count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, who, true, &w);
    if (rc != LBVH_OK) return rc;
    LBVH_LAUNCH_STATS(ctx, ctx->ray_stats, (box_contact_wide_kernel<kContactDeepest, STATS>), dim3(w.waves), dim3(LBVH_WAVE), d_shapes,
                      (uint32_t)count, w.wn, ctx->fast_nodes, (const uint64_t*)nullptr, d_out, (uint64_t)0, w.deep, w.lds, w.deep_cap,
                      ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

extern "C" {

lbvh_status lbvh_triangle_intersections(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                        uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return triangle_queries<false>(ctx, d_queries, count, h_scene, d_offsets, d_tris, capacity, nullptr, "lbvh_triangle_intersections");
}

lbvh_status lbvh_triangle_intersects_any(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                         uint32_t* d_flags)
{
    return triangle_queries<true>(ctx, d_queries, count, h_scene, nullptr, nullptr, 0, d_flags, "lbvh_triangle_intersects_any");
}

lbvh_status lbvh_triangle_intersection_segments(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                                uint64_t* d_offsets, lbvh_tri_segment* d_segments, uint64_t capacity)
{
    return triangle_segments(ctx, d_queries, count, h_scene, d_offsets, d_segments, capacity, "lbvh_triangle_intersection_segments");
}

lbvh_status lbvh_capsule_overlaps(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return shape_overlaps<kShapeCapsule, false>(ctx, d_shapes, count, h_scene, d_offsets, d_tris, capacity, nullptr, "lbvh_capsule_overlaps");
}

lbvh_status lbvh_capsule_overlaps_any(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                      uint32_t* d_flags)
{
    return shape_overlaps<kShapeCapsule, true>(ctx, d_shapes, count, h_scene, nullptr, nullptr, 0, d_flags, "lbvh_capsule_overlaps_any");
}

lbvh_status lbvh_capsule_contacts(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, lbvh_contact* d_contacts, uint64_t capacity)
{
    return capsule_contacts(ctx, d_shapes, count, h_scene, d_offsets, d_contacts, capacity, "lbvh_capsule_contacts");
}

lbvh_status lbvh_capsule_deepest(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                 lbvh_contact* d_out)
{
    return capsule_deepest(ctx, d_shapes, count, h_scene, d_out, "lbvh_capsule_deepest");
}

lbvh_status lbvh_obb_contacts(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, lbvh_box_contact* d_contacts, uint64_t capacity)
{
    return obb_contacts(ctx, d_shapes, count, h_scene, d_offsets, d_contacts, capacity, "lbvh_obb_contacts");
}

lbvh_status lbvh_obb_deepest(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                             lbvh_box_contact* d_out)
{
    return obb_deepest(ctx, d_shapes, count, h_scene, d_out, "lbvh_obb_deepest");
}

lbvh_status lbvh_obb_overlaps(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return shape_overlaps<kShapeObb, false>(ctx, d_shapes, count, h_scene, d_offsets, d_tris, capacity, nullptr, "lbvh_obb_overlaps");
}

lbvh_status lbvh_obb_overlaps_any(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint32_t* d_flags)
{
    return shape_overlaps<kShapeObb, true>(ctx, d_shapes, count, h_scene, nullptr, nullptr, 0, d_flags, "lbvh_obb_overlaps_any");
}

lbvh_status lbvh_sphere_cast(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene, lbvh_hit* d_hits)
{
    return shape_casts<false>(ctx, d_casts, count, h_scene, d_hits, "lbvh_sphere_cast");
}

lbvh_status lbvh_sphere_cast_any(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene, uint32_t* d_flags)
{
    return shape_casts<true>(ctx, d_casts, count, h_scene, d_flags, "lbvh_sphere_cast_any");
}

lbvh_status lbvh_capsule_cast(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene, lbvh_hit* d_hits)
{
    return shape_casts<false>(ctx, d_casts, count, h_scene, d_hits, "lbvh_capsule_cast");
}

lbvh_status lbvh_capsule_cast_any(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene, uint32_t* d_flags)
{
    return shape_casts<true>(ctx, d_casts, count, h_scene, d_flags, "lbvh_capsule_cast_any");
}

lbvh_status lbvh_box_cast(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene, lbvh_box_hit* d_hits)
{
    return shape_casts<false, lbvh_box_ray, lbvh_box_hit>(ctx, d_casts, count, h_scene, d_hits, "lbvh_box_cast");
}

lbvh_status lbvh_box_cast_any(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene, uint32_t* d_flags)
{
    return shape_casts<true, lbvh_box_ray, lbvh_box_hit>(ctx, d_casts, count, h_scene, d_flags, "lbvh_box_cast_any");
}

lbvh_status lbvh_triangle_cast(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene, lbvh_tri_cast_hit* d_hits)
{
    return shape_casts<false, lbvh_tri_ray, lbvh_tri_cast_hit>(ctx, d_casts, count, h_scene, d_hits, "lbvh_triangle_cast");
}

lbvh_status lbvh_triangle_cast_any(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene, uint32_t* d_flags)
{
    return shape_casts<true, lbvh_tri_ray, lbvh_tri_cast_hit>(ctx, d_casts, count, h_scene, d_flags, "lbvh_triangle_cast_any");
}

lbvh_status lbvh_closest_point_query(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                     lbvh_closest_point* d_out)
{
    return point_queries<false>(ctx, d_queries, count, h_scene, d_out, "lbvh_closest_point_query");
}

lbvh_status lbvh_within_distance(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                 uint32_t* d_flags)
{
    return point_queries<true>(ctx, d_queries, count, h_scene, d_flags, "lbvh_within_distance");
}

lbvh_status lbvh_segment_closest_point(lbvh_context* ctx, const lbvh_segment_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                       lbvh_segment_closest* d_out)
{
    return distance_queries<false>(ctx, d_queries, count, h_scene, d_out, "lbvh_segment_closest_point");
}

lbvh_status lbvh_segment_within_distance(lbvh_context* ctx, const lbvh_segment_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                         uint32_t* d_flags)
{
    return distance_queries<true>(ctx, d_queries, count, h_scene, d_flags, "lbvh_segment_within_distance");
}

lbvh_status lbvh_triangle_closest_point(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                        lbvh_tri_closest* d_out)
{
    return distance_queries<false>(ctx, d_queries, count, h_scene, d_out, "lbvh_triangle_closest_point");
}

lbvh_status lbvh_triangle_within_distance(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count,
                                          const lbvh_scene* h_scene, uint32_t* d_flags)
{
    return distance_queries<true>(ctx, d_queries, count, h_scene, d_flags, "lbvh_triangle_within_distance");
}

lbvh_status lbvh_triangle_gather_within_distance(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count,
                                                 const lbvh_scene* h_scene, uint64_t* d_offsets, lbvh_tri_closest* d_records,
                                                 uint64_t capacity)
{
    return triangle_proximity(ctx, d_queries, count, h_scene, d_offsets, d_records, capacity, "lbvh_triangle_gather_within_distance");
}

// the four-wide walk only, one launch; the per-lane lists are dynamic LDS sized from k
lbvh_status lbvh_k_closest_points(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, uint32_t k,
                                  const lbvh_scene* h_scene, lbvh_closest_point* d_out, uint32_t* d_found)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_queries != nullptr && h_scene != nullptr && d_out != nullptr);
    LBVH_REQUIRE(ctx, k >= 1u && k <= (uint32_t)LBVH_K_CLOSEST_MAX);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_found & 3) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_k_closest_points", true, &w);
    if (rc != LBVH_OK) return rc;
    const size_t list_lds = (size_t)3 * k * LBVH_WAVE * sizeof(uint32_t);       // 768 bytes per slot: 24 KiB at k = 32
    LBVH_LAUNCH_STATS_SHMEM(ctx, ctx->ray_stats, k_closest_wide_kernel<STATS>, dim3(w.waves), dim3(LBVH_WAVE), list_lds, d_queries, (uint32_t)count, k,
                            w.wn, ctx->fast_nodes, d_out, d_found, w.deep, w.lds, w.deep_cap, ctx->fault_dev, ctx->ray_stats);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

lbvh_status lbvh_box_overlaps(lbvh_context* ctx, const lbvh_aabb* d_boxes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return overlap_queries<true>(ctx, d_boxes, count, h_scene, d_offsets, d_tris, capacity, "lbvh_box_overlaps");
}

lbvh_status lbvh_gather_within_distance(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                        uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity)
{
    return overlap_queries<false>(ctx, d_queries, count, h_scene, d_offsets, d_tris, capacity, "lbvh_gather_within_distance");
}

lbvh_status lbvh_sphere_cast_all(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                 uint64_t* d_offsets, lbvh_hit* d_hits, uint64_t capacity)
{
    return cast_gathers<kCastSphere>(ctx, d_casts, count, h_scene, d_offsets, d_hits, capacity, "lbvh_sphere_cast_all");
}

lbvh_status lbvh_capsule_cast_all(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, lbvh_hit* d_hits, uint64_t capacity)
{
    return cast_gathers<kCastCapsule>(ctx, d_casts, count, h_scene, d_offsets, d_hits, capacity, "lbvh_capsule_cast_all");
}

lbvh_status lbvh_box_cast_all(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, lbvh_box_hit* d_hits, uint64_t capacity)
{
    return cast_gathers<kCastBox>(ctx, d_casts, count, h_scene, d_offsets, d_hits, capacity, "lbvh_box_cast_all");
}

lbvh_status lbvh_triangle_cast_all(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                   uint64_t* d_offsets, lbvh_tri_cast_hit* d_hits, uint64_t capacity)
{
    return triangle_cast_gathers(ctx, d_casts, count, h_scene, d_offsets, d_hits, capacity, "lbvh_triangle_cast_all");
}

lbvh_status lbvh_animate(lbvh_context* ctx, const lbvh_triangle* d_rest, uint32_t n, const uint32_t* d_body,
                         const float* d_centres, float cos_angle, float sin_angle, lbvh_triangle* d_out)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (n == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_rest != nullptr && d_body != nullptr && d_centres != nullptr && d_out != nullptr);
    LBVH_REQUIRE(ctx, d_rest != d_out);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_rest & 15) == 0 && ((uintptr_t)d_out & 15) == 0 && ((uintptr_t)d_centres & 15) == 0);
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    lbvh_note_write(ctx, d_out, (size_t)n * sizeof(lbvh_triangle));
    LBVH_LAUNCH(ctx, animate_kernel, dim3((unsigned)(((size_t)n * 8 + 255) / 256)), dim3(256), d_rest, n, d_body, (const float4*)d_centres, cos_angle,
                sin_angle, d_out);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

lbvh_status lbvh_path_begin(lbvh_context* ctx, const lbvh_camera* h_camera, lbvh_path_state* d_states)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, h_camera != nullptr && d_states != nullptr && ((uintptr_t)d_states & 15) == 0);
    const lbvh_camera cam = *h_camera;
    LBVH_REQUIRE(ctx, cam.screen_width > 0 && cam.screen_height > 0);
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->ray_list.valid = false;                      // new states: no bounce has listed their live paths yet
    LBVH_LAUNCH(ctx, path_begin_kernel, dim3((cam.screen_width + 15) / 16, (cam.screen_height + 15) / 16), dim3(256), cam,
                d_states);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

lbvh_status lbvh_trace_rays(lbvh_context* ctx, const lbvh_path_state* d_states, size_t count, float t_min,
                            const lbvh_scene* h_scene, lbvh_hit* d_hits)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_states != nullptr && h_scene != nullptr && d_hits != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_states & 15) == 0 && ((uintptr_t)d_hits & 15) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_trace_rays", false, &w);     // (the list is dropped: this call takes list 0 for its own rays)
    if (rc != LBVH_OK) return rc;
    uint32_t* n_alive = ray_counter(ctx, 0);
    uint32_t* list = ray_list(ctx, count, 0);
    LBVH_HIP_TRY(ctx, hipMemsetAsync(n_alive, 0, 4, ctx->cur_stream));
    LBVH_LAUNCH(ctx, alive_rays_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), d_states, count, n_alive, list, d_hits);
    return launch_ray_walk<false, kClosest>(ctx, d_states, n_alive, list, t_min, d_hits, w);
}

lbvh_status lbvh_trace_closest(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene, lbvh_hit* d_hits)
{
    return trace_plain_rays<kClosest>(ctx, d_rays, count, h_scene, d_hits, "lbvh_trace_closest");
}

lbvh_status lbvh_trace_occluded(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene, uint32_t* d_occluded)
{
    return trace_plain_rays<kAny>(ctx, d_rays, count, h_scene, d_occluded, "lbvh_trace_occluded");
}

lbvh_status lbvh_count_hits(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene, uint32_t* d_counts)
{
    return trace_plain_rays<kCount>(ctx, d_rays, count, h_scene, d_counts, "lbvh_count_hits");
}

lbvh_status lbvh_path_scatter(lbvh_context* ctx, const lbvh_scene* h_scene, const lbvh_hit* d_hits, size_t count,
                              uint32_t bounce, uint32_t seed, float albedo, lbvh_path_state* d_states)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, h_scene != nullptr && h_scene->triangles != nullptr && d_hits != nullptr && d_states != nullptr);
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the live paths of the bounce before, if this call continues that very frame (same buffers, next bounce): only they can
    // have anything to scatter
    const bool from_list = bounce >= 2u && ctx->ray_list.valid && ctx->ray_list.states == (const void*)d_states && ctx->ray_list.hits == (const void*)d_hits &&
                           ctx->ray_list.count == count && ctx->ray_list.bounce + 1u == bounce && ctx->ray_scratch != nullptr;
    ctx->ray_list.valid = false;                      // the states change without a new list being made
    if (from_list)
        LBVH_LAUNCH(ctx, (path_scatter_kernel<false, false, kScatterItemsList>), dim3((unsigned)((count + 256 * kScatterItemsList - 1) / (256 * kScatterItemsList))),
                    dim3(256), h_scene->triangles, d_hits, count, bounce, seed, albedo, d_states, nullptr, nullptr, lbvh_camera{},
                    ray_list(ctx, count, ctx->ray_list.turn), ray_counter(ctx, ctx->ray_list.turn));
    else
        LBVH_LAUNCH(ctx, path_scatter_kernel<false>, dim3((unsigned)((count + 256 * kScatterItems - 1) / (256 * kScatterItems))), dim3(256), h_scene->triangles,
                    d_hits, count, bounce, seed, albedo, d_states, nullptr, nullptr, lbvh_camera{}, nullptr, nullptr);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

}  // extern "C"

static lbvh_status path_bounce_impl(lbvh_context* ctx, const lbvh_scene* h_scene, lbvh_path_state* d_states, lbvh_hit* d_hits,
                                    size_t count, uint32_t bounce, uint32_t seed, float albedo, float t_min,
                                    const lbvh_camera* h_first_camera)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, h_scene != nullptr && h_scene->triangles != nullptr && d_hits != nullptr && d_states != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_states & 15) == 0 && ((uintptr_t)d_hits & 15) == 0 && count <= 0xFFFFFFFFull);
    walk_launch w;
    const lbvh_status rc = begin_walk(ctx, h_scene, count, "lbvh_path_bounce", false, &w, /* keep_list */ true);
    if (rc != LBVH_OK) return rc;
    // the paths to look at: the list the bounce before left behind, if this call continues that very frame (same buffers, next
    // bounce, nothing written into them since: lbvh_note_write); otherwise every pixel.  The new list goes into the other buffer.
    // (from the second bounce on: at bounce 1 two fifths of a frame's paths are still alive and the two forms cost the same, 53 - 56 us
    // at 1080p; bounces 2, 3 and the last scatter 35 / 33 / 33 -> 27 - 31 / 18 - 20 / 14 - 16 us; 4 paths per thread instead of 2: 33 / 21 / 20)
    const bool from_list = !h_first_camera && bounce >= 2u && ctx->ray_list.valid && ctx->ray_list.states == (const void*)d_states &&
                           ctx->ray_list.hits == (const void*)d_hits && ctx->ray_list.count == count && ctx->ray_list.bounce + 1u == bounce;
    const uint32_t prev = ctx->ray_list.turn, turn = from_list ? prev ^ 1u : 0u;
    uint32_t* n_alive = ray_counter(ctx, turn);
    uint32_t* list = ray_list(ctx, count, turn);
    LBVH_HIP_TRY(ctx, hipMemsetAsync(n_alive, 0, 4, ctx->cur_stream));
    const dim3 scatter_grid((unsigned)((count + 256 * kScatterItems - 1) / (256 * kScatterItems)));
    if (h_first_camera)
        LBVH_LAUNCH(ctx, (path_scatter_kernel<true, true>), scatter_grid, dim3(256), h_scene->triangles, d_hits, count, 0u, seed, albedo, d_states,
                    n_alive, list, *h_first_camera, nullptr, nullptr);
    else if (from_list)
        LBVH_LAUNCH(ctx, (path_scatter_kernel<true, false, kScatterItemsList>), dim3((unsigned)((count + 256 * kScatterItemsList - 1) / (256 * kScatterItemsList))),
                    dim3(256), h_scene->triangles, d_hits, count, bounce, seed, albedo, d_states, n_alive, list, lbvh_camera{}, ray_list(ctx, count, prev),
                    ray_counter(ctx, prev));
    else
        LBVH_LAUNCH(ctx, (path_scatter_kernel<true, false>), scatter_grid, dim3(256), h_scene->triangles, d_hits, count, bounce, seed, albedo,
                    d_states, n_alive, list, lbvh_camera{}, nullptr, nullptr);
    ctx->ray_list.valid = true;
    ctx->ray_list.states = d_states; ctx->ray_list.hits = d_hits; ctx->ray_list.count = count;
    ctx->ray_list.bounce = h_first_camera ? 0u : bounce;
    ctx->ray_list.turn = turn;
    return launch_ray_walk<false, kClosest>(ctx, d_states, n_alive, list, t_min, d_hits, w, bounce >= 1u);
}

extern "C" {

lbvh_status lbvh_path_bounce(lbvh_context* ctx, const lbvh_scene* h_scene, lbvh_path_state* d_states, lbvh_hit* d_hits,
                             size_t count, uint32_t bounce, uint32_t seed, float albedo, float t_min)
{
    return path_bounce_impl(ctx, h_scene, d_states, d_hits, count, bounce, seed, albedo, t_min, nullptr);
}

lbvh_status lbvh_path_first_bounce(lbvh_context* ctx, const lbvh_camera* h_camera, const lbvh_scene* h_scene, lbvh_path_state* d_states,
                                   lbvh_hit* d_hits, uint32_t seed, float albedo, float t_min)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, h_camera != nullptr && h_camera->screen_width > 0 && h_camera->screen_height > 0);
    return path_bounce_impl(ctx, h_scene, d_states, d_hits, (size_t)h_camera->screen_width * (size_t)h_camera->screen_height, 0u, seed, albedo,
                            t_min, h_camera);
}

lbvh_status lbvh_path_resolve(lbvh_context* ctx, const lbvh_path_state* d_states, size_t count, uint16_t* d_rgba16f)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_states != nullptr && d_rgba16f != nullptr && ((uintptr_t)d_rgba16f & 7) == 0);
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    LBVH_LAUNCH(ctx, path_resolve_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), d_states, count, d_rgba16f);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

}  // extern "C"
