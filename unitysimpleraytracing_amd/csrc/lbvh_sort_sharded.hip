// lbvh_sort_sharded.hip — lbvh_sort_pairs_sharded: the key-range sharded sort of cfg4 (BASELINE configs[3]) as ONE call over N
// contexts of this process.  The algorithm of sharded_sort.py (one process per GPU) with its torch operations and RCCL
// collectives replaced by the HIP kernels of lbvh_sort.hip, peer-mapped memory and sync events:
//
//   1. local sort         every context sorts its block in place                      lbvh_launch_sort (four passes, no hint)
//   2. splitters          four MSD rounds: digit histogram of the own sorted block     key_histogram_kernel (round r's table)
//                         restricted to the prefixes found so far; record; wait for    sync events (device side)
//                         every other context; sum all W tables and pick the digits    splitter_digit_kernel (redundant on all)
//   3. send counts        the W - 1 splitters' positions in the own block -> pinned    lower_bound_kernel + one copy
//                         host row; the host blocks ONCE (every stream), checks the
//                         capacities and computes the receive offsets
//   4. exchange           one launch per source: every (source range -> destination)   shard_range_copy_kernel
//                         run of keys and of values, stored straight into the
//                         destination contexts' output buffers
//   5. receive sort       each destination waits for every source's event, sorts its   lbvh_launch_sort (four passes, no hint)
//                         slice in place
//   6. broadcast          REPLICATE: every sorted slice into every other context's     shard_range_copy_kernel
//                         output at its global offset; every stream waits for the
//                         broadcasts into its buffer
//
// One ordering event per context, re-recorded at every phase: every wait for phase k is enqueued (host order) before any
// record of phase k + 1, so each wait binds to the record it was meant for.  Stores into another context's buffers (exchange,
// broadcast) come after the round-0 waits, i.e. after everything every context had enqueued before the call.
#include <algorithm>
#include "lbvh_common.h"

namespace {

constexpr uint32_t kMaxW = LBVH_SORT_SHARDED_MAX_CONTEXTS;
constexpr uint32_t kRounds = 4;
constexpr uint32_t kMaxCount = (1u << 30) - 1u;        // lbvh_sort_pairs' per-call limit (the sort's 30-bit status counts)
// device scratch (words): kRounds tables of 16 x 256 | prefixes[16] | positions[16] | remaining[16] (u64)
constexpr size_t kTableWords = 16 * 256;
constexpr size_t kPrefixOff = kRounds * kTableWords, kPosOff = kPrefixOff + 16, kRemOff = kPosOff + 16;
constexpr size_t kScratchBytes = (kRemOff + 2 * 16) * 4;
static_assert(kRemOff % 2 == 0, "the u64 ranks must be 8-byte aligned");

uint32_t* table_of(lbvh_context* c, uint32_t round) { return c->shard_scratch + round * kTableWords; }
uint32_t* prefixes_of(lbvh_context* c) { return c->shard_scratch + kPrefixOff; }
uint32_t* positions_of(lbvh_context* c) { return c->shard_scratch + kPosOff; }
uint64_t* remaining_of(lbvh_context* c) { return reinterpret_cast<uint64_t*>(c->shard_scratch + kRemOff); }

bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

bool misaligned(const void* p) { return ((uintptr_t)p & 3u) != 0; }

int prepare(lbvh_context* c)
{
    LBVH_HIP_TRY(c, hipSetDevice(c->device));
    if (!c->shard_scratch) {
        void* p = nullptr;
        LBVH_HIP_TRY(c, hipMalloc(&p, kScratchBytes));
        c->shard_scratch = (uint32_t*)p;
    }
    if (!c->shard_event) {
        hipEvent_t e = nullptr;
        LBVH_HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToSystem));
        c->shard_event = e;
    }
    if (!c->shard_host) {
        void* p = nullptr;
        LBVH_HIP_TRY(c, hipHostMalloc(&p, kMaxW * 4, hipHostMallocDefault));
        c->shard_host = (uint32_t*)p;
    }
    return LBVH_OK;
}

int use(lbvh_context* c)
{
    LBVH_HIP_TRY(c, hipSetDevice(c->device));
    return LBVH_OK;
}

int record(lbvh_context* c)
{
    LBVH_HIP_TRY(c, hipEventRecord(c->shard_event, c->stream));
    return LBVH_OK;
}

// c's stream waits (on the device) for the last record of every other context's ordering event
int wait_others(lbvh_context* const* ctxs, uint32_t n, uint32_t self)
{
    lbvh_context* c = ctxs[self];
    for (uint32_t j = 0; j < n; ++j)
        if (j != self) LBVH_HIP_TRY(c, hipStreamWaitEvent(c->stream, ctxs[j]->shard_event, 0));
    return LBVH_OK;
}

// stage spans for lbvh_profile_begin / _end (include/lbvh_debug.h): nothing is recorded unless the context profiles
hipEvent_t stage_begin(lbvh_context* c)
{
    if (!c->prof_enabled) return nullptr;
    hipEvent_t a = lbvh_prof_event(c);
    (void)hipEventRecord(a, c->stream);
    return a;
}

void stage_end(lbvh_context* c, hipEvent_t a, const char* name)
{
    if (!a) return;
    hipEvent_t b = lbvh_prof_event(c);
    (void)hipEventRecord(b, c->stream);
    c->prof_spans.push_back({name, a, b});
}

#define SHARD_TRY(i, expr)                         \
    do {                                           \
        const int _rc = (expr);                    \
        if (_rc != LBVH_OK) { *who = (int)(i); return _rc; } \
    } while (0)

int sharded_impl(lbvh_context* const* ctxs, uint32_t W, uint32_t* const* d_keys, uint32_t* const* d_values,
                 const uint32_t* h_counts, uint32_t* const* d_out_keys, uint32_t* const* d_out_values,
                 const uint32_t* h_out_capacity, uint32_t* h_out_counts, uint32_t flags, int* who, std::string* why)
{
    // ---- arguments: nothing is enqueued before they all pass
    auto bad = [&](const std::string& s) { *why = s; return LBVH_ERR_INVALID_ARG; };
    if (!d_keys || !d_values || !h_counts || !d_out_keys || !d_out_values || !h_out_capacity || !h_out_counts)
        return bad("a pointer-array argument is NULL");
    if (flags & ~LBVH_SORT_SHARDED_REPLICATE) return bad("unknown flags");
    const bool replicate = (flags & LBVH_SORT_SHARDED_REPLICATE) != 0;
    uint64_t total = 0;
    for (uint32_t i = 0; i < W; ++i) {
        const uint32_t n = h_counts[i], cap = h_out_capacity[i];
        total += n;
        if (n && (!d_keys[i] || !d_values[i])) return bad("block " + std::to_string(i) + " has pairs but a NULL pointer");
        if (cap && (!d_out_keys[i] || !d_out_values[i])) return bad("output " + std::to_string(i) + " has a capacity but a NULL pointer");
        if (misaligned(d_keys[i]) || misaligned(d_values[i]) || misaligned(d_out_keys[i]) || misaligned(d_out_values[i]))
            return bad("context " + std::to_string(i) + ": a pointer is not 4-byte aligned");
        const size_t nb = (size_t)n * 4, cb = (size_t)cap * 4;
        if (overlap(d_out_keys[i], cb, d_keys[i], nb) || overlap(d_out_keys[i], cb, d_values[i], nb) ||
            overlap(d_out_values[i], cb, d_keys[i], nb) || overlap(d_out_values[i], cb, d_values[i], nb) ||
            overlap(d_out_keys[i], cb, d_out_values[i], cb))
            return bad("context " + std::to_string(i) + ": an output overlaps an input or the other output");
    }
    if (total > kMaxCount) return bad("more than 2^30 - 1 pairs in total");
    for (uint32_t q = 0; q < W; ++q) h_out_counts[q] = 0;
    if (total == 0) return LBVH_OK;

    // ---- peers (both directions: histogram tables are read, outputs written), scratch
    for (uint32_t i = 0; i < W; ++i)
        for (uint32_t j = 0; j < W; ++j)
            if (ctxs[j]->device != ctxs[i]->device) SHARD_TRY(i, lbvh_peer_enable(ctxs[i], ctxs[j]->device));
    for (uint32_t i = 0; i < W; ++i) SHARD_TRY(i, prepare(ctxs[i]));

    // ---- 1. local sort
    for (uint32_t i = 0; i < W; ++i) {
        lbvh_context* c = ctxs[i];
        SHARD_TRY(i, use(c));
        lbvh_note_write(c, d_keys[i], (size_t)h_counts[i] * 4);
        lbvh_note_write(c, d_values[i], (size_t)h_counts[i] * 4);
        hipEvent_t a = stage_begin(c);
        SHARD_TRY(i, lbvh_launch_sort(c, d_keys[i], d_values[i], h_counts[i], false, 32u, false));
        stage_end(c, a, "sharded:local_sort");
    }

    // send[i][q]: pairs of block i that go to slice q (= a run of its sorted block starting at edge[i][q])
    uint32_t edge[kMaxW][kMaxW + 1], send[kMaxW][kMaxW];
    if (W == 1) {
        edge[0][0] = 0;
        edge[0][1] = h_counts[0];
        send[0][0] = h_counts[0];
    } else {
        // ---- 2. splitters: four MSD rounds
        hipEvent_t span[kMaxW];
        for (uint32_t r = 0; r < kRounds; ++r) {
            const uint32_t shift = 24u - 8u * r;
            for (uint32_t i = 0; i < W; ++i) {
                lbvh_context* c = ctxs[i];
                SHARD_TRY(i, use(c));
                if (r == 0) span[i] = stage_begin(c);
                SHARD_TRY(i, r == 0 ? lbvh_launch_key_histogram(c, d_keys[i], h_counts[i], nullptr, 1u, 32u, shift, table_of(c, 0))
                                    : lbvh_launch_key_histogram(c, d_keys[i], h_counts[i], prefixes_of(c), W - 1u, shift + 8u, shift,
                                                                table_of(c, r)));
                SHARD_TRY(i, record(c));
            }
            for (uint32_t i = 0; i < W; ++i) {
                lbvh_context* c = ctxs[i];
                SHARD_TRY(i, use(c));
                SHARD_TRY(i, wait_others(ctxs, W, i));
                const uint32_t* tables[kMaxW];
                for (uint32_t j = 0; j < W; ++j) tables[j] = table_of(ctxs[j], r);
                SHARD_TRY(i, lbvh_launch_splitter_digit(c, tables, W, W - 1u, r, total, prefixes_of(c), remaining_of(c)));
                if (r == kRounds - 1) stage_end(c, span[i], "sharded:splitters");
            }
        }
        // ---- 3. send counts: the one host synchronisation
        for (uint32_t i = 0; i < W; ++i) {
            lbvh_context* c = ctxs[i];
            SHARD_TRY(i, use(c));
            SHARD_TRY(i, lbvh_launch_lower_bound(c, d_keys[i], h_counts[i], prefixes_of(c), W - 1u, positions_of(c)));
            const hipError_t e = hipMemcpyAsync(c->shard_host, positions_of(c), (W - 1u) * 4u, hipMemcpyDeviceToHost, c->stream);
            if (e != hipSuccess) { *who = (int)i; return lbvh_set_error(c, LBVH_ERR_HIP, "hipMemcpyAsync(send offsets)", hipGetErrorString(e)); }
        }
        for (uint32_t i = 0; i < W; ++i) {
            lbvh_context* c = ctxs[i];
            const hipError_t e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { *who = (int)i; return lbvh_set_error(c, LBVH_ERR_HIP, "hipStreamSynchronize", hipGetErrorString(e)); }
            SHARD_TRY(i, lbvh_check_fault(c));
        }
        for (uint32_t i = 0; i < W; ++i) {
            edge[i][0] = 0;
            for (uint32_t q = 1; q < W; ++q) edge[i][q] = ctxs[i]->shard_host[q - 1];
            edge[i][W] = h_counts[i];
            for (uint32_t q = 0; q < W; ++q) {
                if (edge[i][q + 1] < edge[i][q]) {          // splitters are non-decreasing: cannot happen
                    *who = (int)i;
                    return lbvh_set_error(ctxs[i], LBVH_ERR_HIP, "lbvh_sort_pairs_sharded", "internal: decreasing send offsets");
                }
                send[i][q] = edge[i][q + 1] - edge[i][q];
            }
        }
    }
    // slice lengths, capacities, offsets
    uint32_t base[kMaxW + 1];
    base[0] = 0;
    for (uint32_t q = 0; q < W; ++q) {
        uint32_t n = 0;
        for (uint32_t i = 0; i < W; ++i) n += send[i][q];
        h_out_counts[q] = n;
        base[q + 1] = base[q] + n;
    }
    for (uint32_t q = 0; q < W; ++q) {
        const uint32_t need = replicate ? (uint32_t)total : h_out_counts[q];
        if (need > h_out_capacity[q]) {
            char msg[160];
            snprintf(msg, sizeof msg, "%s %u needs %u pairs, its capacity is %u (h_out_counts is filled; nothing was written to any output)",
                     replicate ? "output (REPLICATE) of context" : "slice", q, need, h_out_capacity[q]);
            return bad(msg);
        }
    }
    for (uint32_t q = 0; q < W; ++q) {
        const size_t words = replicate ? (size_t)total : h_out_counts[q];
        lbvh_note_write(ctxs[q], d_out_keys[q], words * 4);
        lbvh_note_write(ctxs[q], d_out_values[q], words * 4);
    }

    // ---- 4. exchange: one range-copy launch per source
    for (uint32_t i = 0; i < W; ++i) {
        lbvh_context* c = ctxs[i];
        SHARD_TRY(i, use(c));
        lbvh_copy_run runs[2 * kMaxW];
        uint32_t n_runs = 0;
        for (uint32_t q = 0; q < W; ++q) {
            if (!send[i][q]) continue;
            uint32_t off = replicate ? base[q] : 0u;          // earlier sources' runs come first: arrival in source order
            for (uint32_t s = 0; s < i; ++s) off += send[s][q];
            runs[n_runs++] = {d_keys[i] + edge[i][q], d_out_keys[q] + off, send[i][q]};
            runs[n_runs++] = {d_values[i] + edge[i][q], d_out_values[q] + off, send[i][q]};
        }
        hipEvent_t a = stage_begin(c);
        SHARD_TRY(i, lbvh_launch_range_copy(c, runs, n_runs));
        stage_end(c, a, "sharded:exchange");
        SHARD_TRY(i, record(c));
    }
    if (W == 1) return LBVH_OK;          // one block: its sorted copy is the result

    // ---- 5. receive sort
    for (uint32_t q = 0; q < W; ++q) {
        lbvh_context* c = ctxs[q];
        SHARD_TRY(q, use(c));
        SHARD_TRY(q, wait_others(ctxs, W, q));
        const uint32_t at = replicate ? base[q] : 0u;
        hipEvent_t a = stage_begin(c);
        SHARD_TRY(q, lbvh_launch_sort(c, d_out_keys[q] + at, d_out_values[q] + at, h_out_counts[q], false, 32u, false));
        stage_end(c, a, "sharded:receive_sort");
    }
    if (!replicate) return LBVH_OK;

    // ---- 6. broadcast: slice q into every other output at its global offset
    for (uint32_t q = 0; q < W; ++q) {
        lbvh_context* c = ctxs[q];
        SHARD_TRY(q, use(c));
        lbvh_copy_run runs[2 * kMaxW];
        uint32_t n_runs = 0;
        for (uint32_t p = 0; p < W && h_out_counts[q]; ++p) {
            if (p == q) continue;
            runs[n_runs++] = {d_out_keys[q] + base[q], d_out_keys[p] + base[q], h_out_counts[q]};
            runs[n_runs++] = {d_out_values[q] + base[q], d_out_values[p] + base[q], h_out_counts[q]};
        }
        hipEvent_t a = stage_begin(c);
        SHARD_TRY(q, lbvh_launch_range_copy(c, runs, n_runs));
        stage_end(c, a, "sharded:broadcast");
        SHARD_TRY(q, record(c));
    }
    for (uint32_t p = 0; p < W; ++p) {
        lbvh_context* c = ctxs[p];
        SHARD_TRY(p, use(c));
        SHARD_TRY(p, wait_others(ctxs, W, p));
    }
    return LBVH_OK;
}

}  // namespace

extern "C" lbvh_status lbvh_sort_pairs_sharded(lbvh_context* const* ctxs, uint32_t n_ctx, uint32_t* const* d_keys,
                                               uint32_t* const* d_values, const uint32_t* h_counts, uint32_t* const* d_out_keys,
                                               uint32_t* const* d_out_values, const uint32_t* h_out_capacity, uint32_t* h_out_counts,
                                               uint32_t flags)
{
    if (!ctxs || n_ctx == 0 || n_ctx > kMaxW) {
        const char* msg = "n_ctx must be 1 .. LBVH_SORT_SHARDED_MAX_CONTEXTS (16) with a non-NULL context array";
        if (ctxs && n_ctx > kMaxW)
            for (uint32_t i = 0; i < kMaxW; ++i)
                if (ctxs[i]) lbvh_set_error(ctxs[i], LBVH_ERR_INVALID_ARG, "lbvh_sort_pairs_sharded", msg);
        return lbvh_set_error(nullptr, LBVH_ERR_INVALID_ARG, "lbvh_sort_pairs_sharded", msg);
    }
    std::string why;
    for (uint32_t i = 0; i < n_ctx && why.empty(); ++i) {
        if (!ctxs[i]) why = "context " + std::to_string(i) + " is NULL";
        for (uint32_t j = 0; j < i && why.empty(); ++j)
            if (ctxs[i] == ctxs[j]) why = "contexts " + std::to_string(j) + " and " + std::to_string(i) + " are the same context";
    }
    int who = -1;
    const int rc = why.empty() ? sharded_impl(ctxs, n_ctx, d_keys, d_values, h_counts, d_out_keys, d_out_values, h_out_capacity,
                                              h_out_counts, flags, &who, &why)
                               : LBVH_ERR_INVALID_ARG;
    if (rc == LBVH_OK) return LBVH_OK;
    // the text goes to every context of the call (and to lbvh_last_error(NULL) when none is usable)
    const std::string msg = who >= 0 ? ctxs[who]->err : "lbvh_sort_pairs_sharded: " + why;
    for (uint32_t i = 0; i < n_ctx; ++i)
        if (ctxs[i]) ctxs[i]->err = msg;
    lbvh_set_error(nullptr, rc, msg.c_str(), nullptr);
    return rc;
}
