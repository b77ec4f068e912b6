// lbvh_segsort.hip — lbvh_sort_hit_segments / lbvh_sort_index_segments (include/lbvh.h): every segment of a CSR list put into
// ascending key order in place, on the device, with no scratch: the pass that follows lbvh_gather_hits, lbvh_box_overlaps and
// lbvh_gather_within_distance when a consumer needs the segments ordered.
//
// One implementation for both record types (seg_key<T>): a 16-byte hit record carries the 64-bit key (K(t), tri), a 32-bit index
// is its own key.  The sort is the all-ascending bitonic network: the first step of a merge of 2h records pairs i with
// i ^ (2h - 1), the later ones pair i with i + j for j = h/2 .. 1.  Every exchange puts the smaller record at the lower index, so
// records "at +infinity" behind the end of a range would never move: a range of any length is sorted without padding by skipping
// every exchange whose partner lies at or behind its end.
//
// Two launches over the same offsets, on disjoint segments:
//   wave tier   segments of 2 .. kWaveRecords records (0 and 1 need nothing).  A 64-lane workgroup takes 64 consecutive queries,
//               one per lane, and cuts them into sub-runs of consecutive lanes with at most kWaveRecords records in all; a sub-run
//               is loaded into LDS, every record tagged with its lane's rank in the sub-run, sorted ONCE by (rank, key) — which
//               sorts every segment inside its own slot, with no loop per segment — and stored back to where it came from.
//   block tier  longer segments, one at a time by a workgroup of kBlockThreads: up to kBlockRecords records in LDS; beyond that
//               the chunks of kBlockRecords are sorted in LDS, and of every later merge the steps of stride >= kBlockRecords are
//               exchanges on device memory by the same workgroup (a workgroup lives on one CU: after the barrier it sees its own
//               stores) and the steps below that run in LDS again.  O(n log^2 n) on one CU.
// Neither kernel uses atomics, per-thread scratch or anything of the context but its stream.
#include "lbvh_common.h"

#include <algorithm>

namespace {

constexpr uint32_t kWaveRecords = 256;         // W: records of a wave-tier sub-run (4 per lane)
constexpr uint32_t kBlockRecords = 4096;       // B: records of a block-tier chunk (64 KiB of hits)
constexpr uint32_t kBlockThreads = 1024;
constexpr uint32_t kBlockWaves = kBlockThreads / LBVH_WAVE;
constexpr uint32_t kSortWaves = 8192;          // the per-lane walkers' grid (lbvh_path.hip kRayWaves): 32 waves on each of 256 CUs
constexpr uint32_t kSortBlocks = 512;          // block tier: two workgroups of 1 024 threads per CU
static_assert((kWaveRecords & (kWaveRecords - 1)) == 0 && kWaveRecords <= (1u << 14) && kWaveRecords % LBVH_WAVE == 0, "tier border");
static_assert((kBlockRecords & (kBlockRecords - 1)) == 0 && kBlockRecords <= (1u << 14) && kBlockRecords >= kWaveRecords, "tier border");

// K of include/lbvh.h: the fp32 word as an unsigned word that orders as the values do, -0 with +0, every NaN after +inf
__device__ __forceinline__ uint32_t order_word(uint32_t w)
{
    if ((w & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
    if (w == 0x80000000u) w = 0u;
    return (w & 0x80000000u) ? ~w : (w | 0x80000000u);
}

template <typename T> struct seg_key;
template <> struct seg_key<uint4> {            // lbvh_hit as four words: {t, tri, u, v}
    static __device__ __forceinline__ uint64_t of(const uint4& r) { return ((uint64_t)order_word(r.x) << 32) | r.y; }
};
template <> struct seg_key<uint32_t> {
    static __device__ __forceinline__ uint64_t of(uint32_t r) { return r; }
};

// one exchange in LDS; TAGGED: ordered by (tag, key), the tag travels with its record
template <typename T, bool TAGGED>
__device__ __forceinline__ void exchange_lds(T* rec, uint32_t* tag, uint32_t i, uint32_t p)
{
    const T a = rec[i], b = rec[p];
    bool swap = seg_key<T>::of(b) < seg_key<T>::of(a);
    if (TAGGED) {
        const uint32_t ta = tag[i], tb = tag[p];
        swap = tb < ta || (tb == ta && swap);
        if (swap) { tag[i] = tb; tag[p] = ta; }
    }
    if (swap) { rec[i] = b; rec[p] = a; }
}

// one step of the network over rec[0 .. m) by NT threads.  FLIP: i with i ^ (2h - 1); else i with i + h.  Pair t has its lower
// index at i = (t / h) * 2h + t % h, which grows with t.
template <typename T, bool TAGGED, bool FLIP, uint32_t NT>
__device__ __forceinline__ void step_lds(T* rec, uint32_t* tag, uint32_t m, uint32_t h, uint32_t tid)
{
    __syncthreads();
    for (uint32_t t = tid;; t += NT) {
        const uint32_t i = ((t & ~(h - 1u)) << 1) | (t & (h - 1u));
        if (i >= m) break;
        const uint32_t p = FLIP ? (i ^ (2u * h - 1u)) : (i + h);
        if (p < m) exchange_lds<T, TAGGED>(rec, tag, i, p);
    }
}

// the steps of a merge that follow its first one, from stride h down to 1
template <typename T, bool TAGGED, uint32_t NT>
__device__ __forceinline__ void tail_lds(T* rec, uint32_t* tag, uint32_t m, uint32_t h, uint32_t tid)
{
    for (uint32_t j = h; j != 0u; j >>= 1) step_lds<T, TAGGED, false, NT>(rec, tag, m, j, tid);
}

template <typename T, bool TAGGED, uint32_t NT>
__device__ __forceinline__ void sort_lds(T* rec, uint32_t* tag, uint32_t m, uint32_t tid)
{
    for (uint32_t h = 1; h < m; h <<= 1) {
        step_lds<T, TAGGED, true, NT>(rec, tag, m, h, tid);
        tail_lds<T, TAGGED, NT>(rec, tag, m, h >> 1, tid);
    }
    __syncthreads();
}

// ---- wave tier ----------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(LBVH_WAVE) void segsort_wave_kernel(const uint64_t* offsets, uint32_t count, T* data, uint64_t capacity)
{
    __shared__ T s_rec[kWaveRecords];
    __shared__ uint32_t s_tag[kWaveRecords];
    __shared__ uint64_t s_delta[LBVH_WAVE];        // per rank: the segment's first record minus its first LDS slot
    constexpr uint32_t kPerLane = kWaveRecords / LBVH_WAVE;
    const uint32_t lane = threadIdx.x;
    const uint32_t groups = count / LBVH_WAVE + (count % LBVH_WAVE != 0u ? 1u : 0u);
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t q = (uint64_t)g * LBVH_WAVE + lane;
        uint64_t lo = 0, hi = 0;
        if (q < count) { lo = offsets[q]; hi = offsets[q + 1]; }
        const bool fits = lo <= hi && hi <= capacity;
        const uint64_t m = hi - lo;
        const uint32_t len = (fits && m >= 2u && m <= kWaveRecords) ? (uint32_t)m : 0u;
        const uint32_t incl = wave_inclusive_sum(len);
        if (wave_total_from_inclusive(incl) == 0u) continue;
        uint32_t a = 0;                            // the sub-run is lanes [a, b): uniform
        while (a < LBVH_WAVE) {
            const uint32_t base = a != 0u ? (uint32_t)__shfl((int)incl, (int)(a - 1u)) : 0u;
            const uint64_t over = __ballot(lane >= a && incl - base > kWaveRecords);
            const uint32_t b = over != 0ull ? (uint32_t)__builtin_ctzll(over) : (uint32_t)LBVH_WAVE;     // > a: no len exceeds W
            const uint32_t n = (uint32_t)__shfl((int)incl, (int)(b - 1u)) - base;
            if (n != 0u) {
                const bool mine = lane >= a && lane < b && len != 0u;
                const uint32_t start = incl - len - base;
                // the owner rank of every slot: the heads of the segments, then a running maximum over the slots
                for (uint32_t s = lane; s < n; s += LBVH_WAVE) s_tag[s] = 0u;
                __syncthreads();
                if (mine) {
                    s_tag[start] = lane - a;
                    s_delta[lane - a] = lo - start;
                }
                __syncthreads();
                uint32_t run = 0, upto[kPerLane];
#pragma unroll
                for (uint32_t k = 0; k < kPerLane; k++) {
                    const uint32_t s = lane * kPerLane + k;
                    run = max(run, s < n ? s_tag[s] : 0u);
                    upto[k] = run;
                }
                uint32_t below = run;
#pragma unroll
                for (uint32_t d = 1; d < LBVH_WAVE; d <<= 1) {
                    const uint32_t other = (uint32_t)__shfl_up((int)below, d);
                    if (lane >= d) below = max(below, other);
                }
                below = (uint32_t)__shfl_up((int)below, 1u);
                if (lane == 0u) below = 0u;
                __syncthreads();
#pragma unroll
                for (uint32_t k = 0; k < kPerLane; k++) {
                    const uint32_t s = lane * kPerLane + k;
                    if (s < n) s_tag[s] = max(below, upto[k]);
                }
                __syncthreads();
                // slot s holds record s_delta[owner] + s: inside [lo, hi) of its owner, and hi <= capacity
                for (uint32_t s = lane; s < n; s += LBVH_WAVE) s_rec[s] = data[s_delta[s_tag[s]] + s];
                sort_lds<T, true, LBVH_WAVE>(s_rec, s_tag, n, lane);
                // (rank, key) order leaves every slot with its owner's tag
                for (uint32_t s = lane; s < n; s += LBVH_WAVE) data[s_delta[s_tag[s]] + s] = s_rec[s];
                __syncthreads();
            }
            a = b;
        }
    }
}

// ---- block tier ---------------------------------------------------------------------------------------------------------------

template <typename T>
__device__ __forceinline__ void exchange_global(T* g, uint64_t i, uint64_t p)
{
    const T a = g[i], b = g[p];
    if (seg_key<T>::of(b) < seg_key<T>::of(a)) { g[i] = b; g[p] = a; }
}

// one step of the network on device memory over g[0 .. n), as step_lds
template <typename T, bool FLIP>
__device__ __forceinline__ void step_global(T* g, uint64_t n, uint64_t h, uint32_t tid)
{
    __syncthreads();
    for (uint64_t t = tid;; t += kBlockThreads) {
        const uint64_t i = ((t & ~(h - 1ull)) << 1) | (t & (h - 1ull));
        if (i >= n) break;
        const uint64_t p = FLIP ? (i ^ (2ull * h - 1ull)) : (i + h);
        if (p < n) exchange_global<T>(g, i, p);
    }
}

// g[0 .. n): one fitting segment, n > kWaveRecords
template <typename T>
__device__ void sort_long(T* g, uint64_t n, T* s_rec, uint32_t tid)
{
    // FIRST: every chunk sorted in LDS; later: the steps of a merge below the chunk size
    auto chunks = [&](bool first) {
        for (uint64_t c = 0; c < n; c += kBlockRecords) {
            const uint32_t m = (uint32_t)min((uint64_t)kBlockRecords, n - c);
            __syncthreads();
            for (uint32_t i = tid; i < m; i += kBlockThreads) s_rec[i] = g[c + i];
            if (first) sort_lds<T, false, kBlockThreads>(s_rec, nullptr, m, tid);
            else { tail_lds<T, false, kBlockThreads>(s_rec, nullptr, m, kBlockRecords / 2u, tid); __syncthreads(); }
            for (uint32_t i = tid; i < m; i += kBlockThreads) g[c + i] = s_rec[i];
        }
    };
    chunks(true);
    for (uint64_t h = kBlockRecords; h < n; h <<= 1) {         // the merge of sorted runs of h records into runs of 2h
        step_global<T, true>(g, n, h, tid);
        for (uint64_t j = h >> 1; j >= kBlockRecords; j >>= 1) step_global<T, false>(g, n, j, tid);
        chunks(false);
    }
}

template <typename T>
__global__ __launch_bounds__(kBlockThreads) void segsort_block_kernel(const uint64_t* offsets, uint32_t count, T* data, uint64_t capacity)
{
    __shared__ T s_rec[kBlockRecords];
    __shared__ uint64_t s_long[kBlockWaves];       // per wave of the workgroup: its lanes with a long segment
    __shared__ uint64_t s_seg[2];                  // the segment in hand: first record, length
    const uint32_t tid = threadIdx.x, lane = tid % LBVH_WAVE, wave = tid / LBVH_WAVE;
    const uint32_t groups = count / kBlockThreads + (count % kBlockThreads != 0u ? 1u : 0u);
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t q = (uint64_t)g * kBlockThreads + tid;
        uint64_t lo = 0, hi = 0;
        if (q < count) { lo = offsets[q]; hi = offsets[q + 1]; }
        const bool is_long = lo <= hi && hi <= capacity && hi - lo > kWaveRecords;
        const uint64_t mask = __ballot(is_long);
        __syncthreads();                           // the previous group's masks have been read
        if (lane == 0u) s_long[wave] = mask;
        __syncthreads();
        for (uint32_t w = 0; w < kBlockWaves; w++) {
            uint64_t left = s_long[w];             // uniform over the workgroup
            while (left != 0ull) {
                const uint32_t l = (uint32_t)__builtin_ctzll(left);
                left &= left - 1ull;
                __syncthreads();                   // the previous segment's s_seg has been read
                if (tid == w * LBVH_WAVE + l) { s_seg[0] = lo; s_seg[1] = hi - lo; }
                __syncthreads();
                sort_long<T>(data + s_seg[0], s_seg[1], s_rec, tid);
            }
        }
    }
}

template <typename T>
lbvh_status sort_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, T* d_data, uint64_t capacity)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_offsets != nullptr && d_data != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_data & (sizeof(T) - 1)) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    if (capacity == 0) return LBVH_OK;
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // records move inside the caller's buffer: if that is a path tracer's hit buffer or a scene array, what was made from it is stale
    lbvh_note_write(ctx, d_data, (size_t)std::min<uint64_t>(capacity, SIZE_MAX / sizeof(T)) * sizeof(T));
    const uint32_t total = (uint32_t)count;
    const uint32_t waves = (uint32_t)std::min<size_t>(kSortWaves, (count + LBVH_WAVE - 1) / LBVH_WAVE);
    const uint32_t blocks = (uint32_t)std::min<size_t>(kSortBlocks, (count + kBlockThreads - 1) / kBlockThreads);
    LBVH_LAUNCH(ctx, segsort_wave_kernel<T>, dim3(waves), dim3(LBVH_WAVE), d_offsets, total, d_data, capacity);
    LBVH_LAUNCH(ctx, segsort_block_kernel<T>, dim3(blocks), dim3(kBlockThreads), d_offsets, total, d_data, capacity);
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
}

}  // namespace

extern "C" {

lbvh_status lbvh_sort_hit_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, lbvh_hit* d_hits, uint64_t capacity)
{
    return sort_segments<uint4>(ctx, d_offsets, count, (uint4*)d_hits, capacity);
}

lbvh_status lbvh_sort_index_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, uint32_t* d_tris, uint64_t capacity)
{
    return sort_segments<uint32_t>(ctx, d_offsets, count, d_tris, capacity);
}

}  // extern "C"
