// lbvh_segsort.hip — lbvh_sort_hit_segments / lbvh_sort_index_segments / lbvh_sort_record_segments (include/lbvh.h): every segment of a CSR list put into
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
//
// lbvh_sort_record_segments — the 32-byte records of the contact, proximity, intersection-segment and plane-section lists — keeps
// the two tiers and the network but does not push 32-byte records through it: a compare-exchange would move 64 bytes through LDS.
// It sorts 16-byte ENTRIES {key high, key low, source slot, rank} instead — the key is formed once per record, from its first
// 16 bytes and the order mode, a template parameter of the two kernels that the LDS network never sees — and then moves every record once, from the
// LDS slot its entry names:
//   wave tier   a sub-run's records are staged in LDS (kWaveRecords * 32 bytes) next to the entries; the entries are sorted by
//               (rank, key) and slot s of the segment receives the record of entry s as two 16-byte stores.
//   block tier  chunks of kRecordChunk records, staged the same way (32 + 16 bytes a record: 48 KiB a workgroup at 1 024 records,
//               so two workgroups of 1 024 threads share a CU's 160 KiB); the exchanges at strides >= kRecordChunk move whole
//               records on device memory and read the second half of a pair only when it swaps.
#include "lbvh_common.h"

#include <algorithm>

namespace {

constexpr uint32_t kWaveRecords = 256;         // W: records of a wave-tier sub-run (4 per lane)
constexpr uint32_t kBlockRecords = 4096;       // B: records of a block-tier chunk (64 KiB of hits)
constexpr uint32_t kBlockThreads = 1024;
constexpr uint32_t kBlockWaves = kBlockThreads / LBVH_WAVE;
constexpr uint32_t kRecordChunk = 1024;        // records of a block-tier chunk of 32-byte records: 32 KiB of records + 16 KiB of entries
constexpr uint32_t kSortWaves = 8192;          // the per-lane walkers' grid (lbvh_walk.h kRayWaves): 32 waves on each of 256 CUs
constexpr uint32_t kSortBlocks = 512;          // block tier: two workgroups of 1 024 threads per CU
static_assert((kWaveRecords & (kWaveRecords - 1)) == 0 && kWaveRecords <= (1u << 14) && kWaveRecords % LBVH_WAVE == 0, "tier border");
static_assert((kBlockRecords & (kBlockRecords - 1)) == 0 && kBlockRecords <= (1u << 14) && kBlockRecords >= kWaveRecords, "tier border");
static_assert((kRecordChunk & (kRecordChunk - 1)) == 0 && kRecordChunk <= (1u << 14) && kRecordChunk >= kWaveRecords, "tier border");
static_assert(2u * (kRecordChunk * 48u + 1024u) <= 160u * 1024u, "two workgroups of the record block tier per CU");

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
// the stand-in of a 32-byte record in the network: {key high, key low, the LDS slot of its record, its segment's rank in a sub-run}
struct sort_entry { uint4 w; };
template <> struct seg_key<sort_entry> {
    static __device__ __forceinline__ uint64_t of(const sort_entry& e) { return ((uint64_t)e.w.x << 32) | e.w.y; }
};

// the key of a 32-byte record under `order` (include/lbvh.h), from its first 16 bytes: words 0, 1 and 3
__device__ __forceinline__ uint64_t record_key(const uint4& head, uint32_t order)
{
    if (order == LBVH_SORT_RECORDS_BY_TRI) return head.w;
    uint32_t k = order_word(head.x);
    if (order == LBVH_SORT_RECORDS_DESCENDING && k != 0xFFFFFFFFu) k = ~k;     // D: a NaN stays last
    return ((uint64_t)k << 32) | head.y;
}

#ifdef LBVH_RECORD_SORT_DIRECT
// A/B variant only (tools/build_variant.sh record_direct -DLBVH_RECORD_SORT_DIRECT, tools/record_sort_bench.py): the straightforward
// instantiation of the two kernels below with a 32-byte T — every compare-exchange moves 64 bytes through LDS, a block-tier chunk is
// 128 KiB (one workgroup per CU) — so that the entries-then-permute kernels can be measured against it.  Needs 32-byte alignment.
template <uint32_t ORDER> struct rec32 { uint4 lo, hi; };
template <uint32_t ORDER> struct seg_key<rec32<ORDER>> {
    static __device__ __forceinline__ uint64_t of(const rec32<ORDER>& r) { return record_key(r.lo, ORDER); }
};
#endif

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

// an entry carries its tag in its own fourth word: one 16-byte exchange, `tag` is not used
template <>
__device__ __forceinline__ void exchange_lds<sort_entry, true>(sort_entry* rec, uint32_t*, uint32_t i, uint32_t p)
{
    const sort_entry a = rec[i], b = rec[p];
    if (b.w.w < a.w.w || (b.w.w == a.w.w && seg_key<sort_entry>::of(b) < seg_key<sort_entry>::of(a))) { rec[i] = b; rec[p] = a; }
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

// ---- 32-byte records: entries through the network, every record moved once ------------------------------------------------------

// A record is two uint4: record r of `data` is data[2r], data[2r + 1].  The frame of segsort_wave_kernel; the owner rank of a slot
// is built in the fourth word of its entry.
template <uint32_t ORDER>
__global__ __launch_bounds__(LBVH_WAVE) void recsort_wave_kernel(const uint64_t* offsets, uint32_t count, uint4* data, uint64_t capacity)
{
    constexpr uint32_t order = ORDER;           // a template parameter: fewer instructions than a uniform argument (profiles/record_sort)
    __shared__ uint4 s_rec[2 * kWaveRecords];
    __shared__ sort_entry s_ent[kWaveRecords];
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
                for (uint32_t s = lane; s < n; s += LBVH_WAVE) s_ent[s].w.w = 0u;
                __syncthreads();
                if (mine) {
                    s_ent[start].w.w = lane - a;
                    s_delta[lane - a] = lo - start;
                }
                __syncthreads();
                uint32_t run = 0, upto[kPerLane];
#pragma unroll
                for (uint32_t k = 0; k < kPerLane; k++) {
                    const uint32_t s = lane * kPerLane + k;
                    run = max(run, s < n ? s_ent[s].w.w : 0u);
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
                    if (s < n) s_ent[s].w.w = max(below, upto[k]);
                }
                __syncthreads();
                // slot s holds record s_delta[owner] + s: inside [lo, hi) of its owner, and hi <= capacity.  Half x of the record
                // is word x of the pair; the first half has the key words.
                // (The odd lane of a slot reads s_ent[s].w.w while the even lane rewrites s_ent[s].w: the rewrite stores the same
                // rank in that word, and the one wave of the workgroup reads before it writes, so the read sees the rank either way.)
                for (uint32_t x = lane; x < 2u * n; x += LBVH_WAVE) {
                    const uint32_t s = x >> 1, rank = s_ent[s].w.w;
                    const uint4 v = data[2u * (s_delta[rank] + s) + (x & 1u)];
                    s_rec[x] = v;
                    if ((x & 1u) == 0u) {
                        const uint64_t key = record_key(v, order);
                        s_ent[s].w = make_uint4((uint32_t)(key >> 32), (uint32_t)key, s, rank);
                    }
                }
                sort_lds<sort_entry, true, LBVH_WAVE>(s_ent, nullptr, n, lane);
                // (rank, key) order leaves every slot with an entry of its owner's rank: slot s receives the record of entry s
                for (uint32_t x = lane; x < 2u * n; x += LBVH_WAVE) {
                    const uint32_t s = x >> 1;
                    const uint4 e = s_ent[s].w;
                    data[2u * (s_delta[e.w] + s) + (x & 1u)] = s_rec[2u * e.z + (x & 1u)];
                }
                __syncthreads();
            }
            a = b;
        }
    }
}

// one step of the network on device memory over the records g[0 .. 2n), as step_global: the first halves decide, the second halves
// are read only by a pair that swaps
template <bool FLIP>
__device__ __forceinline__ void step_global_records(uint4* g, uint64_t n, uint64_t h, uint32_t tid, uint32_t order)
{
    __syncthreads();
    for (uint64_t t = tid;; t += kBlockThreads) {
        const uint64_t i = ((t & ~(h - 1ull)) << 1) | (t & (h - 1ull));
        if (i >= n) break;
        const uint64_t p = FLIP ? (i ^ (2ull * h - 1ull)) : (i + h);
        if (p < n) {
            const uint4 a0 = g[2ull * i], b0 = g[2ull * p];
            if (record_key(b0, order) < record_key(a0, order)) {
                const uint4 a1 = g[2ull * i + 1ull], b1 = g[2ull * p + 1ull];
                g[2ull * i] = b0; g[2ull * i + 1ull] = b1;
                g[2ull * p] = a0; g[2ull * p + 1ull] = a1;
            }
        }
    }
}

// g[0 .. 2n): the records of one fitting segment, n > kWaveRecords; sort_long with chunks of kRecordChunk
__device__ void sort_long_records(uint4* g, uint64_t n, uint4* s_rec, sort_entry* s_ent, uint32_t tid, uint32_t order)
{
    // FIRST: every chunk sorted in LDS; later: the steps of a merge below the chunk size
    auto chunks = [&](bool first) {
        for (uint64_t c = 0; c < n; c += kRecordChunk) {
            const uint32_t m = (uint32_t)min((uint64_t)kRecordChunk, n - c);
            __syncthreads();
            for (uint32_t x = tid; x < 2u * m; x += kBlockThreads) {
                const uint4 v = g[2ull * c + x];
                s_rec[x] = v;
                if ((x & 1u) == 0u) {
                    const uint64_t key = record_key(v, order);
                    s_ent[x >> 1].w = make_uint4((uint32_t)(key >> 32), (uint32_t)key, x >> 1, 0u);
                }
            }
            if (first) sort_lds<sort_entry, false, kBlockThreads>(s_ent, nullptr, m, tid);
            else { tail_lds<sort_entry, false, kBlockThreads>(s_ent, nullptr, m, kRecordChunk / 2u, tid); __syncthreads(); }
            for (uint32_t x = tid; x < 2u * m; x += kBlockThreads) g[2ull * c + x] = s_rec[2u * s_ent[x >> 1].w.z + (x & 1u)];
        }
    };
    chunks(true);
    for (uint64_t h = kRecordChunk; h < n; h <<= 1) {          // the merge of sorted runs of h records into runs of 2h
        step_global_records<true>(g, n, h, tid, order);
        for (uint64_t j = h >> 1; j >= kRecordChunk; j >>= 1) step_global_records<false>(g, n, j, tid, order);
        chunks(false);
    }
}

// the frame of segsort_block_kernel
template <uint32_t ORDER>
__global__ __launch_bounds__(kBlockThreads) void recsort_block_kernel(const uint64_t* offsets, uint32_t count, uint4* data, uint64_t capacity)
{
    constexpr uint32_t order = ORDER;           // a template parameter: fewer instructions than a uniform argument (profiles/record_sort)
    __shared__ uint4 s_rec[2 * kRecordChunk];
    __shared__ sort_entry s_ent[kRecordChunk];
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
                sort_long_records(data + 2ull * s_seg[0], s_seg[1], s_rec, s_ent, tid, order);
            }
        }
    }
}

lbvh_status sort_records(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, uint4* d_records, uint64_t capacity, uint32_t order)
{
    if (!ctx) return LBVH_ERR_INVALID_ARG;
    LBVH_REQUIRE(ctx, order <= LBVH_SORT_RECORDS_BY_TRI);
    if (count == 0) return LBVH_OK;
    LBVH_REQUIRE(ctx, d_offsets != nullptr && d_records != nullptr);
    LBVH_REQUIRE(ctx, ((uintptr_t)d_offsets & 7) == 0 && ((uintptr_t)d_records & 15) == 0);
    LBVH_REQUIRE(ctx, count <= 0xFFFFFFFFull);
    if (capacity == 0) return LBVH_OK;
#ifdef LBVH_RECORD_SORT_DIRECT
    if (order == LBVH_SORT_RECORDS_ASCENDING) return sort_segments<rec32<0>>(ctx, d_offsets, count, (rec32<0>*)d_records, capacity);
    if (order == LBVH_SORT_RECORDS_DESCENDING) return sort_segments<rec32<1>>(ctx, d_offsets, count, (rec32<1>*)d_records, capacity);
    return sort_segments<rec32<2>>(ctx, d_offsets, count, (rec32<2>*)d_records, capacity);
#else
    LBVH_HIP_TRY(ctx, hipSetDevice(ctx->device));
    lbvh_note_write(ctx, d_records, (size_t)std::min<uint64_t>(capacity, SIZE_MAX / 32u) * 32u);
    const uint32_t total = (uint32_t)count;
    const uint32_t waves = (uint32_t)std::min<size_t>(kSortWaves, (count + LBVH_WAVE - 1) / LBVH_WAVE);
    const uint32_t blocks = (uint32_t)std::min<size_t>(kSortBlocks, (count + kBlockThreads - 1) / kBlockThreads);
#define LBVH_RECSORT_LAUNCH(ORDER)                                                                                              \
    LBVH_LAUNCH(ctx, recsort_wave_kernel<ORDER>, dim3(waves), dim3(LBVH_WAVE), d_offsets, total, d_records, capacity);          \
    LBVH_LAUNCH(ctx, recsort_block_kernel<ORDER>, dim3(blocks), dim3(kBlockThreads), d_offsets, total, d_records, capacity)
    if (order == LBVH_SORT_RECORDS_ASCENDING) { LBVH_RECSORT_LAUNCH(LBVH_SORT_RECORDS_ASCENDING); }
    else if (order == LBVH_SORT_RECORDS_DESCENDING) { LBVH_RECSORT_LAUNCH(LBVH_SORT_RECORDS_DESCENDING); }
    else { LBVH_RECSORT_LAUNCH(LBVH_SORT_RECORDS_BY_TRI); }
#undef LBVH_RECSORT_LAUNCH
    LBVH_HIP_TRY(ctx, hipGetLastError());
    return LBVH_OK;
#endif
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

lbvh_status lbvh_sort_record_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, void* d_records, uint64_t capacity,
                                      uint32_t order)
{
    return sort_records(ctx, d_offsets, count, (uint4*)d_records, capacity, order);
}

}  // extern "C"
