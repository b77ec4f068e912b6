/*
 * lbvh.h — C ABI of liblbvh.so, the MI355X (gfx950) native LBVH ray-tracing hot path.
 *
 * This is the drop-in boundary for the hot path of drzhn/UnitySimpleRaytracing:
 *   Morton/AABB -> radix sort -> DistributeKeys -> Karras tree -> AABB refit -> primary-ray traversal.
 * In the reference that path sits behind UnityEngine.ComputeBuffer / ComputeShader.Dispatch; here
 * every Dispatch (and the two CPU loops the reference runs on the host) is one `extern "C"` call
 * that a C# [DllImport] shim, the C++ host classes under unitysimpleraytracing_amd/host/ and the
 * Python ctypes tests all bind the same way.  Citations are file:line in the reference tree
 * (Sc/ = Assets/_Scripts/, Sh/ = Assets/_Shaders/).
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary; every call returns lbvh_status
 *     (0 = LBVH_OK, negative = error; lbvh_last_error(ctx) gives the text).
 *   - pointers named d_* are DEVICE pointers (hipMalloc'ed memory on the context's GPU: from
 *     lbvh_buffer_alloc, or any other allocator, e.g. a torch tensor's data_ptr()).
 *     Pointers named h_* are host pointers borrowed for the duration of the call.
 *   - all stage calls are asynchronous and ordered on the context's HIP stream;
 *     lbvh_buffer_download and lbvh_sync block (= ComputeBuffer.GetData, Sc/DataBuffer.cs:50-54).
 *   - a context is bound to one GPU and is not thread-safe; multi-GPU = one context per device
 *     (one process per GPU in bench.py; one process driving N contexts in host/lbvh_host.hpp MultiGpuDrawer).
 *   - buffer layouts are the reference's, bit for bit (Sh/Constants.cginc:9-54,
 *     Sc/SceneDataTypes.cs:4-89).
 */
#ifndef LBVH_H
#define LBVH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBVH_ABI_VERSION 11

/* ---- status codes ------------------------------------------------------------------------- */
typedef int32_t lbvh_status;
#define LBVH_OK                 0
#define LBVH_ERR_INVALID_ARG   -1   /* null pointer, n < 2, n > capacity, bad tile rectangle ...   */
#define LBVH_ERR_OUT_OF_MEMORY -2
#define LBVH_ERR_HIP           -3   /* a HIP runtime call failed, or a device-side wait gave up (the next lbvh_sync /
                                       lbvh_buffer_download reports it ONCE: what was enqueued before that call is
                                       invalid, later work is judged on its own); see lbvh_last_error  */
#define LBVH_ERR_NO_DEVICE     -4   /* no usable gfx950 device                                     */

/* ---- scene structs: the reference's buffer element layouts --------------------------------- */

/* Sh/Constants.cginc:9-15, Sc/SceneDataTypes.cs:4-16 — 32 bytes */
typedef struct lbvh_aabb {
    float min[3];
    float _dummy0;
    float max[3];
    float _dummy1;
} lbvh_aabb;

/* Sh/Constants.cginc:36-54, Sc/SceneDataTypes.cs:18-41 — 128 bytes */
typedef struct lbvh_triangle {
    float a[3];        float _dummy0;
    float b[3];        float _dummy1;
    float c[3];        float _dummy2;
    float a_uv[2];
    float b_uv[2];
    float c_uv[2];
    float _dummy3[2];
    float a_normal[3]; float _dummy4;
    float b_normal[3]; float _dummy5;
    float c_normal[3]; float _dummy6;
} lbvh_triangle;

/* Sh/Constants.cginc:17-18 */
#define LBVH_INTERNAL_NODE 0u
#define LBVH_LEAF_NODE     1u
/* every word of an unwritten node slot (Sc/SceneDataTypes.cs:63-71,85-89); also root.parent */
#define LBVH_NULL          0xFFFFFFFFu

/* Sh/Constants.cginc:20-28, Sc/SceneDataTypes.cs:43-72 — 24 bytes */
typedef struct lbvh_internal_node {
    uint32_t leftNode;
    uint32_t leftNodeType;
    uint32_t rightNode;
    uint32_t rightNodeType;
    uint32_t parent;
    uint32_t index;
} lbvh_internal_node;

/* Sh/Constants.cginc:30-34, Sc/SceneDataTypes.cs:74-89 — 8 bytes */
typedef struct lbvh_leaf_node {
    uint32_t parent;
    uint32_t index;
} lbvh_leaf_node;

/* MAX_FLOAT is the INTEGER literal 0x7F7FFFFF converted to float (Sh/Constants.cginc:7):
 * 2139095040.0f, not FLT_MAX.  A miss carries exactly this value in lbvh_hit.t. */
#define LBVH_MAX_FLOAT 2139095040.0f

/* Per-ray result = the reference's RaycastResult (Sh/Raytracing/Raytracing.compute:30-35)
 * in its field order: distance, triangleIndex, uv.  16 bytes.
 * (The reference consumes it in-kernel for shading, :178-184; here it is the kernel output.) */
typedef struct lbvh_hit {
    float    t;      /* distance; LBVH_MAX_FLOAT on a miss                       */
    uint32_t tri;    /* ORIGINAL triangle index (into triangleData); 0 on a miss */
    float    u, v;   /* barycentrics of b and c; (0,0) on a miss                 */
} lbvh_hit;

/* The uniforms RaytracingMeshDrawer.Update sets each frame (Sc/RaytracingMeshDrawer.cs:78-81)
 * plus the implicit _ProjectionParams.y (camera near plane) the kernel reads
 * (Sh/Raytracing/Raytracing.compute:108). */
typedef struct lbvh_camera {
    int32_t screen_width;        /* screenWidth                                               */
    int32_t screen_height;       /* screenHeight                                              */
    float   camera_fov;          /* cameraFov = tan(fovY/2), already the tangent              */
    float   near_plane;          /* _ProjectionParams.y                                       */
    float   camera_to_world[16]; /* cameraToWorldMatrix, row-major m00,m01,m02,m03,m10,...    */
} lbvh_camera;

/* Traversal flavours of lbvh_trace_primary. */
#define LBVH_TRACE_REFERENCE 0  /* the reference's visit order, no pruning, separate node arrays */
#define LBVH_TRACE_FAST      1  /* 8x8 packets over fused 64-B nodes, near-first, t-pruned; same min-t (see the note below) */
#define LBVH_TRACE_FAST_EXACT 2 /* LBVH_TRACE_FAST with the reference's choice on exact ties: every record equals, word for
                                 * word, the record of the reference's loop under the accept rule of the note below (the
                                 * oracle's orc_trace_primary_rule with fast_rule = 1) — that is LBVH_TRACE_REFERENCE's record
                                 * at every pixel whose reference winner is not a t in front of its own triangle's box
                                 * (every pixel of every scene in the test suite but one, which is pinned:
                                 * tests/golden/grazing_ray_case.json).  A ray that meets two triangles at EXACTLY the same t
                                 * (the case in which the fast walk's order-independent choice — lowest triangle index — can
                                 * differ from the triangle the reference's visit order meets first) is given to the triangle
                                 * that order meets first: the order is read off the scene's internalNodes / leafNodes
                                 * (parent words, child types; leaf j's `index` is j, as TreeConstructor writes it,
                                 * BVH.compute:116-120).  No d_stats with this mode. */
/* Where both fast modes differ from LBVH_TRACE_REFERENCE — by a rule, not by chance (tests/test_grazing_ray.py).
 * The reference prunes nothing, so its record is the minimum COMPUTED t over every triangle whose box the ray's line passes —
 * including, for a ray within ~0.01 degree of a triangle's plane, a t that is noise of the fp32 triangle test
 * (Raytracing.compute:37-73: det ~ 1e-4, the dot products cancel) and lies IN FRONT OF the distance at which the ray enters that
 * triangle's own padded box.  A walk that skips boxes entered beyond its best hit would report such a record or not depending
 * on the order in which it meets the leaves (packet shape, shard count, dispatch history).  The fast modes therefore do not
 * count a computed t that is smaller than the slab test's entry distance of the triangle's own box: their record is the
 * nearest hit that is not in front of its own box, the same whatever the order (and whatever the number of GPUs), and equal
 * to the reference's wherever the reference's winner is not such a t.  The CPU oracle carries the rule as an option
 * (orc_trace_primary_rule) and the fast modes are tested equal to THAT frame bit for bit; an application that wants the
 * reference's artefacts too has LBVH_TRACE_REFERENCE.  Frequency: one pixel in the order of 10^9 randomised rays
 * (tools/fuzz_parity.py), none of the 2 073 600 of the benchmark's frame.  The secondary-ray calls (lbvh_trace_rays, the path
 * tracer) use the same rule. */

/* Optional per-launch traversal statistics (sums over all rays of the launch), in the
 * reference's visit semantics for LBVH_TRACE_REFERENCE: P nodes popped, B internal boxes hit,
 * L leaf-AABB tests, T triangle tests.  Used for the algorithmic-bytes figure.
 * LBVH_TRACE_FAST walks one 8x8-pixel packet per wave: there `pops` = 64-byte node fetches and
 * `leaf_tests` = triangle-line fetches per PACKET (each shared by the packet's 64 rays),
 * `box_hits` and `tri_tests` stay per ray. */
typedef struct lbvh_trace_stats {
    uint64_t pops;
    uint64_t box_hits;
    uint64_t leaf_tests;
    uint64_t tri_tests;
    uint64_t hits;
} lbvh_trace_stats;

typedef struct lbvh_context lbvh_context;

/* ---- library / context ---------------------------------------------------------------------- */

/* ABI version of the loaded library (== LBVH_ABI_VERSION of the header it was built from). */
int32_t lbvh_abi_version(void);

/* Number of visible HIP devices; does not create a context.  Returns <0 on error. */
int32_t lbvh_device_count(void);

/* Create a context on HIP device `device_id` with its own non-blocking stream.
 * Replaces: the implicit Unity graphics device + IShaderContainer kernel registry
 * (Sc/ShaderContainer.cs:6-40, FindKernel calls Sc/ComputeBufferSorter.cs:64-82,
 * Sc/BVHConstructor.cs:45-46, Sc/RaytracingMeshDrawer.cs:59-60). */
lbvh_status lbvh_create(int32_t device_id, lbvh_context** out_ctx);

/* Same, but enqueue on a caller-owned hipStream_t (e.g. torch's current stream); the context
 * never destroys that stream. */
lbvh_status lbvh_create_on_stream(int32_t device_id, void* hip_stream, lbvh_context** out_ctx);

/* Frees the context's scratch (sort ping-pong, histograms, refit scratch) and its stream.
 * Replaces the Dispose chains (Sc/ComputeBufferSorter.cs:274-281, Sc/BVHConstructor.cs:71-74). */
lbvh_status lbvh_destroy(lbvh_context* ctx);

/* Text of the last error on this context ("" if none).  ctx may be NULL for creation errors. */
const char* lbvh_last_error(const lbvh_context* ctx);

/* Block until everything enqueued on the context's stream has finished. */
lbvh_status lbvh_sync(lbvh_context* ctx);

/* ---- buffers: DataBuffer<T> / ComputeBuffer (Sc/DataBuffer.cs) ------------------------------ */

/* new ComputeBuffer(count, stride, Structured) — Sc/DataBuffer.cs:25-30. Contents undefined. */
lbvh_status lbvh_buffer_alloc(lbvh_context* ctx, size_t count, size_t stride, void** out_d_ptr);
/* ComputeBuffer.Release — Sc/DataBuffer.cs:72-75 */
lbvh_status lbvh_buffer_free(lbvh_context* ctx, void* d_ptr);
/* DataBuffer(size, initialValue) for word-patterned values — Sc/DataBuffer.cs:14-23, used with
 * 0xFFFFFFFF for keys/indices/NullLeaf nodes (Sc/MeshBufferContainer.cs:108-109,114-115) and 0
 * for the refit flags (Sc/BVHConstructor.cs:41).  Stream-ordered. */
lbvh_status lbvh_buffer_fill_u32(lbvh_context* ctx, void* d_ptr, uint32_t value, size_t n_words);
/* ComputeBuffer.SetData — Sc/DataBuffer.cs:56-60.  Stream-ordered, host buffer is consumed
 * before the call returns. */
lbvh_status lbvh_buffer_upload(lbvh_context* ctx, void* d_dst, const void* h_src, size_t bytes);
/* ComputeBuffer.GetData — Sc/DataBuffer.cs:50-54.  Blocking. */
lbvh_status lbvh_buffer_download(lbvh_context* ctx, void* h_dst, const void* d_src, size_t bytes);

/* ---- stage a-1: Morton codes + per-triangle AABBs ------------------------------------------ */

/* Replaces the CPU loop of MeshBufferContainer's constructor (Sc/MeshBufferContainer.cs:123-146
 * with GetCentroidAndAABB :52-71, NormalizeCentroid :73-83, Morton3D/ExpandBits :32-50).
 * For i < n: d_keys[i] = Morton3D of the padded-AABB centre normalised to the scene box
 * [box_min, box_max] (the reference hard-wires +-125, :9-15), d_indices[i] = i,
 * d_aabb[i] = {min3-0.001, 0, max3+0.001, 0}.  Strict fp32, no FMA contraction.
 * For n <= i < capacity: d_keys[i] = d_indices[i] = 0xFFFFFFFF (the fill of :108-109);
 * d_aabb is left untouched there.  Requires capacity >= n. */
lbvh_status lbvh_morton_aabb(lbvh_context* ctx, const lbvh_triangle* d_triangles, uint32_t n,
                             uint32_t capacity, const float h_box_min[3], const float h_box_max[3],
                             uint32_t* d_keys, uint32_t* d_indices, lbvh_aabb* d_aabb);

/* ---- stage a-2..a-5: radix sort of (key, value) pairs --------------------------------------- */

/* Replaces ComputeBufferSorter<uint,uint>.Sort() (Sc/ComputeBufferSorter.cs:100-126) and its five
 * kernels (Sh/Sorting/LocalRadixSort.compute:53-134, Sh/Sorting/Scan.compute:15-96,
 * Sh/Sorting/GlobalRadixSort.compute:20-40): sorts `count` (key,value) pairs in place, ascending
 * by key, STABLE (equal keys keep their input order) — the unique result of the reference's
 * 4-pass LSD radix sort.  The reference always sorts its whole padded capacity; pass the capacity
 * as `count` to reproduce that (0xFFFFFFFF pads end up last).  Any count >= 0 is accepted.
 * LATENCY (the result never depends on it): for 2^15 <= count < 2^21 a context whose last THREE sorts of this size class had
 * their keys spread over the 12-bit key prefixes (no more than ~12 K pairs under one prefix) takes a two-level form — 49 us
 * instead of 62 at 1 M pairs — whose one weak case is the FIRST input after such a streak that puts more than 16 384 pairs
 * under one prefix: that one call is sorted by a single workgroup per oversized bucket (2 M pairs under one prefix: 13 ms
 * against 0.12 ms; all keys equal: 1.2 ms; profiles/r6/n_sort_cliff.txt), the following calls take the four passes again.
 * An input that alternates between the two kinds never leaves the four passes; a sort captured into a hipGraph (the build
 * chain of lbvh_build_scene when it is replayed) always takes them. */
lbvh_status lbvh_sort_pairs(lbvh_context* ctx, uint32_t* d_keys, uint32_t* d_values,
                            uint32_t count);

/* ---- cfg4: building blocks of the multi-GPU (key-range sharded) sort, SURVEY 8(e) ------------- *
 * The reference has no multi-GPU path; these are the local kernels of the sharded sort that
 * unitysimpleraytracing_amd/sharded_sort.py drives (one process per GPU): every rank sorts its own
 * block, the ranks agree on W-1 splitter keys by all-reducing (RCCL) MSD digit histograms,
 * exchange key ranges with one all-to-all and sort what they received.  The concatenation over
 * ranks is bit-identical to lbvh_sort_pairs over the whole array (stability: ties never straddle
 * ranks and arrive in source-rank order). */

/* d_hist[p * 256 + d] = number of keys k among d_keys[0..count) with ((k >> shift) & 255) == d and,
 * when prefix_shift < 32, (k >> prefix_shift) == h_prefixes[p].  prefix_shift == 32 selects every
 * key (then n_prefixes must be 1 and h_prefixes may be NULL).  n_prefixes <= 16.  d_hist is
 * overwritten.  Keys need not be sorted. */
lbvh_status lbvh_key_histogram(lbvh_context* ctx, const uint32_t* d_keys, uint32_t count,
                               const uint32_t* h_prefixes, uint32_t n_prefixes, uint32_t prefix_shift,
                               uint32_t shift, uint32_t* d_hist);

/* d_positions[j] = the first i in [0, count] with d_sorted_keys[i] >= h_probes[j] (count if none);
 * n_probes <= 64. */
lbvh_status lbvh_lower_bound(lbvh_context* ctx, const uint32_t* d_sorted_keys, uint32_t count,
                             const uint32_t* h_probes, uint32_t n_probes, uint32_t* d_positions);

/* The same two with the prefixes / probes read from DEVICE memory (u32 arrays of n entries): the sharded sort keeps
 * its splitter search on the device between the RCCL all-reduces — digit histogram, all-reduce, digit selection
 * (a few torch operations on the [W-1][256] table), next histogram — with no host round trip per round. */
lbvh_status lbvh_key_histogram_device(lbvh_context* ctx, const uint32_t* d_keys, uint32_t count,
                                      const uint32_t* d_prefixes, uint32_t n_prefixes, uint32_t prefix_shift,
                                      uint32_t shift, uint32_t* d_hist);
lbvh_status lbvh_lower_bound_device(lbvh_context* ctx, const uint32_t* d_sorted_keys, uint32_t count,
                                    const uint32_t* d_probes, uint32_t n_probes, uint32_t* d_positions);

/* ---- cfg4: the key-range sharded sort as ONE call over N contexts of this process -------------------------------------- *
 * The same algorithm as sharded_sort.py (one process per GPU, RCCL), with the collectives replaced by peer-mapped memory and
 * sync events, all of it HIP: every context sorts its block; four MSD rounds of 8-bit digit histograms, summed on every context
 * from every context's table, pick the W - 1 splitters; each context's sorted block is cut at the splitters and its runs are
 * stored straight into the destination contexts' output buffers (over xGMI on distinct GPUs); every destination sorts what it
 * received.
 *
 * Input.     Block i is h_counts[i] pairs at d_keys[i] / d_values[i], memory of ctxs[i]'s device.  The global sequence is the
 *            concatenation of the blocks in context order.
 * Contexts.  1 <= n_ctx <= LBVH_SORT_SHARDED_MAX_CONTEXTS (16: the n_prefixes <= 16 of the histogram kernel holds the W - 1
 *            splitter rows).  Pairwise distinct contexts; their devices may repeat (logical ranks on one GPU).  The call enables
 *            peer access itself (lbvh_peer_enable's semantics) and returns LBVH_ERR_HIP when two devices cannot reach each other.
 * Result, slice mode (flags == 0).  Slice q is d_out_keys[q][0 .. h_out_counts[q]) with its values.  The concatenation of the
 *            slices in context order equals lbvh_sort_pairs over the global sequence, word for word, keys and values (stable).
 *            Slice q holds exactly the keys in [s_q, s_{q+1}): s_q = the key at global sorted position floor(q * N / W), s_0 = 0,
 *            s_W = infinity (the splitters of ShardedSorter.find_splitters), so equal keys never straddle slices.  Words of the
 *            output buffers past a slice are not written.
 * Result, LBVH_SORT_SHARDED_REPLICATE.  Every d_out_keys[i] / d_out_values[i] receives the whole sorted sequence (N pairs) —
 *            the layout of a replicated tree build; h_out_counts still receives the slice lengths.
 * Inputs are clobbered: they come back locally sorted.  Outputs must not overlap any input; overlap on the same context (or of a
 *            context's two outputs) is LBVH_ERR_INVALID_ARG.  Each output array holds h_out_capacity[q] words.
 * Capacity.  Any slice can hold all N pairs (all keys equal).  If a slice needs more than h_out_capacity[q] (under REPLICATE:
 *            N > h_out_capacity[i] for some i), the call returns LBVH_ERR_INVALID_ARG naming the slice and the count it needs,
 *            with h_out_counts filled and nothing written to any output; a retry with larger buffers succeeds (re-sorting
 *            locally sorted blocks is still correct).
 * Limits.    Total pairs <= 2^30 - 1 (the per-call count of lbvh_sort_pairs); a total of 0 is accepted (counts 0, nothing
 *            enqueued).  Every pointer 4-byte aligned; a block of 0 pairs may have NULL pointers, an output of capacity 0 too.
 * Ordering.  The work is enqueued on every context's stream behind what is already there.  A store into another context's
 *            buffer happens only after everything that context had enqueued before the call.  On return, work enqueued later on
 *            ctxs[i] sees d_out_*[i] complete (a device-side wait, no host wait).  The host blocks ONCE per call (n_ctx >= 2), to
 *            read the W x W send-count table — the single synchronisation of sharded_sort.py.
 * Caches.    Every buffer the call writes is a write in lbvh_note_write's sense (as lbvh_sort_pairs): derived scenes and
 *            live-path lists built from them are dropped.
 * The sorts inside the call always take the four-pass form and neither read nor publish lbvh_sort_pairs' two-level hint (a
 * received slice is a narrow key range by construction): a context's later lbvh_sort_pairs behaves as before the call.
 * Errors: lbvh_last_error of every context gives the text. */
#define LBVH_SORT_SHARDED_MAX_CONTEXTS 16
#define LBVH_SORT_SHARDED_REPLICATE    1u

lbvh_status lbvh_sort_pairs_sharded(lbvh_context* const* ctxs, uint32_t n_ctx,
                                    uint32_t* const* d_keys, uint32_t* const* d_values, const uint32_t* h_counts,
                                    uint32_t* const* d_out_keys, uint32_t* const* d_out_values,
                                    const uint32_t* h_out_capacity, uint32_t* h_out_counts, uint32_t flags);

/* ---- stage a-6: DistributeKeys ---------------------------------------------------------------- */

/* Replaces MeshBufferContainer.DistributeKeys (Sc/MeshBufferContainer.cs:154-169), a serial CPU
 * pass between two full-buffer transfers in the reference: on the first n SORTED keys,
 * new[0] = 0, new[i] = new[i-1] + max(old[i] - old[i-1], 1)  (u32 arithmetic), in place. */
lbvh_status lbvh_distribute_keys(lbvh_context* ctx, uint32_t* d_keys, uint32_t n);

/* ---- stage a-7: Karras LBVH topology ---------------------------------------------------------- */

/* Replaces BVHConstructor.ConstructTree -> kernel TreeConstructor
 * (Sc/BVHConstructor.cs:61-64, Sh/BVH/BVH.compute:18-149).  d_sorted_keys[0..n) must be strictly
 * increasing (true after lbvh_distribute_keys).  Writes internal nodes [0, n-1) and leaf nodes
 * [0, n); words the reference never writes (root.parent) are left as they are — fill the buffers
 * with 0xFFFFFFFF first, as the reference does.  n >= 2 (the reference underflows for n < 2,
 * BVH.compute:101). */
lbvh_status lbvh_build_tree(lbvh_context* ctx, uint32_t n, const uint32_t* d_sorted_keys,
                            lbvh_internal_node* d_internal, lbvh_leaf_node* d_leaf);

/* ---- stage a-8: bottom-up AABB refit ------------------------------------------------------------ */

/* Replaces BVHConstructor.ConstructBVH -> kernel BVHConstructor
 * (Sc/BVHConstructor.cs:66-69, Sh/BVH/BVH.compute:152-220): d_bvh[i] = union of the leaf AABBs under
 * internal node i (min/max are exact, so the result equals the reference's arrival-order merge bit for
 * bit).  The reference's per-node arrival flags (atomicsData, Sc/BVHConstructor.cs:41, zeroed once) have
 * no counterpart: the context owns the scratch of the refit and every call is self-contained, so the
 * tree can be rebuilt per frame.  d_internal / d_leaf must hold a tree in ConstructTree's numbering
 * (left child index = split, right = split + 1, root = node 0); the root's parent word is not read.
 * d_triangle_aabb is in ORIGINAL triangle order and is gathered through d_sorted_indices, as in the
 * reference (:203,:212). */
lbvh_status lbvh_refit(lbvh_context* ctx, uint32_t n, const lbvh_internal_node* d_internal,
                       const lbvh_leaf_node* d_leaf, const lbvh_aabb* d_triangle_aabb,
                       const uint32_t* d_sorted_indices, lbvh_aabb* d_bvh);

/* ---- the whole build chain in one call ----------------------------------------------------------- */

#define LBVH_BUILD_FAST_SCENE  1u   /* also build the derived traversal scene (= lbvh_build_fast_scene)        */
#define LBVH_BUILD_RESET_NODES 2u   /* d_internal / d_leaf come out as after a refill with 0xFFFFFFFF           *
                                     * (capacity slots: the slots past the tree and the root's parent word are  *
                                     * written, every other word is the tree's)                                 */

/* RaytracingMeshDrawer.Awake()'s build chain (Sc/RaytracingMeshDrawer.cs:34-51) = lbvh_morton_aabb ->
 * lbvh_sort_pairs(capacity) -> lbvh_distribute_keys -> lbvh_build_tree -> lbvh_refit (+ lbvh_build_fast_scene
 * with LBVH_BUILD_FAST_SCENE), with identical results.  After the sort the reference's arrays and the derived
 * traversal scene are two independent chains of short latency-bound kernels; this call runs them side by side —
 * sharing three launches on the context's stream (up to 2 M triangles), or on the stream and an internal side
 * stream joined before control returns to the stream — so later calls on the context see both.  For per-frame
 * rebuilds of dynamic scenes. */
lbvh_status lbvh_build_scene(lbvh_context* ctx, const lbvh_triangle* d_triangles, uint32_t n, uint32_t capacity,
                             const float h_box_min[3], const float h_box_max[3], uint32_t* d_keys,
                             uint32_t* d_indices, lbvh_aabb* d_aabb, lbvh_internal_node* d_internal,
                             lbvh_leaf_node* d_leaf, lbvh_aabb* d_bvh, uint32_t flags);

/* ---- stage a-9: primary-ray traversal ------------------------------------------------------------ */

/* The scene buffers RaytracingMeshDrawer binds to the Raytracing kernel
 * (Sc/RaytracingMeshDrawer.cs:65-70).  All device pointers. */
typedef struct lbvh_scene {
    uint32_t                  n;                 /* triangle count                                 */
    const uint32_t*           sorted_indices;    /* sortedTriangleIndices                          */
    const lbvh_aabb*          triangle_aabb;     /* triangleAABB (original order)                  */
    const lbvh_internal_node* internal_nodes;    /* internalNodes                                  */
    const lbvh_leaf_node*     leaf_nodes;        /* leafNodes                                      */
    const lbvh_aabb*          bvh;               /* bvhData                                        */
    const lbvh_triangle*      triangles;         /* triangleData (original order)                  */
} lbvh_scene;

/* LBVH_TRACE_FAST and the secondary-ray calls work from a derived traversal scene the context caches.  The cache is
 * keyed: it answers only for the scene it was built from — same triangles / sorted_indices / triangle_aabb pointers and
 * n — and only while no library call has written into those buffers since (lbvh_morton_aabb, lbvh_sort_pairs,
 * lbvh_buffer_upload / fill_u32, lbvh_animate, lbvh_build_scene without LBVH_BUILD_FAST_SCENE ...).  Otherwise the
 * trace returns LBVH_ERR_INVALID_ARG ("stale") instead of hits from old geometry: the reference's Dispatch has no hidden
 * state (Sc/RaytracingMeshDrawer.cs:65-70).  Writes the library cannot see (the caller's own kernels on those buffers)
 * are the caller's to follow with lbvh_build_fast_scene.
 *
 * Build the derived traversal structure used by LBVH_TRACE_FAST for `scene`: its own "traversal
 * tree" over the scene's SORTED triangle order (Karras topology over minimally perturbed Morton
 * keys k'_i = i + max_{j<=i}(k_j - j) instead of DistributeKeys' shifted ones — tighter boxes — and
 * its own refit), flattened to fused 64-B nodes (both child boxes + child references) plus the sorted
 * triangles as 64-B lines (first vertex, two edge vectors, original index) in the same array.  At most 2^30 - 1
 * triangles.  h_box_min/max = the scene box given to
 * lbvh_morton_aabb (the raw Morton code of a sorted position is recomputed from its triangle AABB).
 * Owned by the context, rebuilt on each call; call it after lbvh_sort_pairs (+ lbvh_morton_aabb) and
 * before the first LBVH_TRACE_FAST launch.  The scene's internalNodes / leafNodes / bvhData are not
 * read.  No reference counterpart: hit results are those of the reference arrays (every leaf keeps
 * the slab test of its own AABB), only the order and number of node visits differ. */
lbvh_status lbvh_build_fast_scene(lbvh_context* ctx, const lbvh_scene* h_scene, const float h_box_min[3],
                                  const float h_box_max[3]);

/* Replaces RaytracingMeshDrawer.Update's Dispatch of kernel Raytracing
 * (Sc/RaytracingMeshDrawer.cs:76-84, Sh/Raytracing/Raytracing.compute:105-185) up to and
 * including the traversal loop: for every pixel (x, y) with x0 <= x < x1, y0 <= y < y1 generates
 * the camera ray (:108-126), traverses (:133-176) and writes the RaycastResult to
 * d_hits[(y - y0) * (x1 - x0) + (x - x0)].  The full frame is (0, 0, W, H); rectangles are one way to
 * shard rays across GPUs (lbvh_trace_primary_shard below is the other).  Pixels outside the screen are never computed (the reference
 * over-dispatches and relies on D3D dropping out-of-bounds writes, RaytracingMeshDrawer.cs:83).
 * d_stats may be NULL; if not it receives the launch's lbvh_trace_stats (device memory). */
lbvh_status lbvh_trace_primary(lbvh_context* ctx, const lbvh_camera* h_camera,
                               int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                               const lbvh_scene* h_scene, int32_t mode,
                               lbvh_hit* d_hits, lbvh_trace_stats* d_stats);

/* Ray sharding across GPUs in ONE launch per GPU: traces the pixels of shard `shard_index` of
 * `shard_count` of the FULL frame — every shard_count-th group of 8 adjacent 8x8-pixel tiles (a 64x8-
 * pixel strip), so every shard samples the whole frame evenly — and writes them at their full-frame
 * positions d_hits[y * W + x]; pixels of other shards are not touched.  d_hits holds W*H records on
 * every GPU.  The BVH is replicated; no collective is involved.  The union over all shards equals
 * lbvh_trace_primary(0, 0, W, H). */
lbvh_status lbvh_trace_primary_shard(lbvh_context* ctx, const lbvh_camera* h_camera, uint32_t shard_index,
                                     uint32_t shard_count, const lbvh_scene* h_scene, int32_t mode,
                                     lbvh_hit* d_hits, lbvh_trace_stats* d_stats);

/* ---- one frame from N GPUs (BASELINE configs[2]; SURVEY 8(e): "hit records gathered to GPU 0") ----------------------- *
 * The reference renders ONE image per Update() (Sc/RaytracingMeshDrawer.cs:76-89).  With the rays sharded over N GPUs
 * (lbvh_trace_primary_shard, BVH replicated) the frame is whole only once every share's records sit in one full-frame
 * buffer on the GPU that shades / displays it.  Two ways to get them there, no collective on either:
 *   peer-mapped stores   d_hits of lbvh_trace_primary_shard may be memory of ANOTHER GPU of the node (the frame buffer of
 *                        GPU 0): after lbvh_peer_enable the trace kernel's stores travel over xGMI as the tiles finish — no
 *                        second pass, the transfer overlaps the walk.  One process: the owner waits with lbvh_event_wait on
 *                        the tracing contexts' events.  One process per GPU: the buffer crosses with lbvh_ipc_export /
 *                        lbvh_ipc_import and completion with lbvh_frame_signal / lbvh_frame_wait (flag words in the
 *                        owner's memory, written over xGMI, waited for on the device — no host round trip per frame);
 *   packed shares        lbvh_trace_primary_shard_packed writes a share contiguously (work-item order, 64 records per
 *                        8x8 tile) so that any transport can move it as one block (hipMemcpyPeerAsync, an RCCL
 *                        send / recv); lbvh_frame_unpack on the owner puts every share's records at their pixels. */

/* Kernels of this context may read and write memory that lives on `peer_device` (hipDeviceEnablePeerAccess; a no-op for
 * the context's own device or when already enabled).  LBVH_ERR_HIP when the two GPUs cannot reach each other. */
lbvh_status lbvh_peer_enable(lbvh_context* ctx, int32_t peer_device);

/* An event for ORDERING work between contexts (lbvh_event_create's are for timing: they skip the system-scope release
 * that makes a GPU's stores visible to another one).  Created with hipEventDisableTiming | hipEventReleaseToSystem: its record
 * IS a system-scope release whatever the runtime's default for plain events is.  Recorded with lbvh_event_record, destroyed
 * with lbvh_event_destroy; lbvh_event_elapsed_ms does not take it. */
lbvh_status lbvh_sync_event_create(lbvh_context* ctx, void** out_event);
/* The context's stream waits (on the device, the host does not block) for `event` — an event of lbvh_sync_event_create
 * recorded with lbvh_event_record on ANY context of this process, e.g. the end of another GPU's share of the frame. */
lbvh_status lbvh_event_wait(lbvh_context* ctx, void* event);

/* Cross-process handle of a buffer of lbvh_buffer_alloc (hipIpcGetMemHandle, 64 bytes, to be sent to the other process by
 * any means) / the same memory mapped into this process and usable as a d_ pointer on this context (after
 * lbvh_peer_enable when it lives on another GPU) / unmapped again.  The exporting process keeps ownership. */
#define LBVH_IPC_HANDLE_BYTES 64
lbvh_status lbvh_ipc_export(lbvh_context* ctx, void* d_ptr, uint8_t h_handle[LBVH_IPC_HANDLE_BYTES]);
lbvh_status lbvh_ipc_import(lbvh_context* ctx, const uint8_t h_handle[LBVH_IPC_HANDLE_BYTES], void** out_d_ptr);
lbvh_status lbvh_ipc_close(lbvh_context* ctx, void* d_ptr);

/* Memory for the completion flags below: n_words zeroed 32-bit words that a RUNNING kernel may poll while another GPU or
 * process stores into them.  Ordinary device memory (lbvh_buffer_alloc: coarse-grained) only promises visibility of another
 * device's stores at kernel boundaries, so a flag polled inside a kernel could be served stale from this GPU's L2 for as long
 * as the kernel runs; these words are allocated uncached (hipExtMallocWithFlags, hipDeviceMallocUncached — what RCCL uses for
 * its own flags): every load and store goes to the memory itself.  Exported / imported / freed like any other buffer
 * (lbvh_ipc_export, lbvh_ipc_import, lbvh_buffer_free). */
lbvh_status lbvh_flags_alloc(lbvh_context* ctx, size_t n_words, uint32_t** out_d_flags);
/* d_flags[slot] := value once everything enqueued on this context so far has finished and its stores are visible system
 * wide (a release store at system scope; d_flags may be another GPU's memory: words of lbvh_flags_alloc).  Values of one slot
 * must grow (frame numbers). */
lbvh_status lbvh_frame_signal(lbvh_context* ctx, uint32_t* d_flags, uint32_t slot, uint32_t value);
/* Work enqueued on this context after the call starts only when d_flags[s] >= value (as signed distance: wrap-around safe)
 * for every s < n_slots — e.g. every other rank has signalled this frame.  The wait runs on the device and is bounded by WALL
 * CLOCK (20 s of the GPU's constant 100 MHz counter — a rank may still be starting up when the wait is enqueued; a poll count
 * would make the bound depend on how fast the polls come back): if a flag has not arrived by then the next lbvh_sync /
 * lbvh_buffer_download returns LBVH_ERR_HIP, the GPU does not hang.  n_slots <= 64.
 * d_flags may be another GPU's memory (polled over xGMI: the ranks that wait for the owner's "frame read" word). */
lbvh_status lbvh_frame_wait(lbvh_context* ctx, const uint32_t* d_flags, uint32_t n_slots, uint32_t value);

/* lbvh_trace_primary_shard with the share written CONTIGUOUSLY: record of lane l (pixel (l & 7, l >> 3) of the tile) of the
 * share's k-th work item at d_packed[k * 64 + l]; work item k is tile ((k / 8) * shard_count + shard_index) * 8 + k % 8 of the
 * full frame in row-major tile order.  lbvh_shard_records gives the number of records a share occupies (whole tiles: lanes
 * outside the screen and tiles past the frame's last one are never written). */
lbvh_status lbvh_trace_primary_shard_packed(lbvh_context* ctx, const lbvh_camera* h_camera, uint32_t shard_index,
                                            uint32_t shard_count, const lbvh_scene* h_scene, int32_t mode,
                                            lbvh_hit* d_packed, lbvh_trace_stats* d_stats);
/* Records of shard `shard_index`'s packed share of a width x height frame (pure function; the same for every call site). */
uint64_t lbvh_shard_records(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count);
/* Packed shares -> the full frame: share s (s in [first_shard, first_shard + n_shards)) starts at
 * d_packed[(s - first_shard) * share_stride] (share_stride in records, >= lbvh_shard_records of any of them); its records
 * go to d_frame_hits[y * width + x].  Pixels of other shards are not touched. */
lbvh_status lbvh_frame_unpack(lbvh_context* ctx, const lbvh_hit* d_packed, uint64_t share_stride, uint32_t first_shard,
                              uint32_t n_shards, uint32_t shard_count, int32_t width, int32_t height, lbvh_hit* d_frame_hits);

/* ---- stage a-9, tail: shading -------------------------------------------------------------------- */

/* Replaces the rest of kernel Raytracing's body (Sh/Raytracing/Raytracing.compute:178-184) for `count`
 * RaycastResults in any layout:  t = triangleData[hit.tri] (triangle 0 on a miss, as in the reference),
 * uv = (1-u-v) a_uv + u b_uv + v c_uv, normal likewise (:179-180), lightDir = the SCALAR 0.57735026
 * (normalize(float3(1,1,1)) assigned to a `float`, :181), colour = texture(uv).rgb * max(0.4,
 * dot(lightDir, normal)) (:183), output float4(colour, hit ? 1 : 0) stored as RGBA16F like the
 * reference's render target (Sc/RaytracingMeshDrawer.cs:56).
 * Texture: d_texture_rgba8 = tex_h rows of tex_w RGBA8 texels, row 0 at v = 0 (Unity's convention), no
 * sRGB decode (the project is in Gamma colour space, ProjectSettings.asset:50), sampled like
 * SampleLevel(linearClampSampler, uv, 0): bilinear on texel centres in fp32, clamp addressing, mip 0.
 * Clamp addressing holds for every finite uv: one so large that uv * size overflows fp32 gives the edge texel (the texel
 * coordinate is clamped to +-2^24 before its floor is taken, which changes no finite result).  A NaN uv stays a NaN colour.
 * A miss record carries triangle 0 and is shaded with it.  The record lbvh_path_bounce leaves for an ended path,
 * {LBVH_MAX_FLOAT, 0xFFFFFFFF, 0, 0}, is safe to shade: it reads triangle 0 and gives what {LBVH_MAX_FLOAT, 0, 0, 0} gives.
 * d_rgba16f receives count x 4 IEEE half floats: the fp32 value rounded to nearest even, 65520 and up to infinity.  Of a NaN
 * only the class is specified (lbvh_shade, lbvh_compose, lbvh_path_resolve): the GPU's conversion keeps the sign and the top
 * payload bits, the CPU oracle returns 0x7E00 / 0xFE00. */
lbvh_status lbvh_shade(lbvh_context* ctx, const lbvh_hit* d_hits, size_t count, const lbvh_triangle* d_triangles,
                       const uint8_t* d_texture_rgba8, int32_t tex_w, int32_t tex_h, uint16_t* d_rgba16f);

/* Replaces the full-screen pass of Hidden/ImageComposer (Sh/ImageComposer.shader:44-52, driven by
 * RaytracingMeshDrawer.OnRenderImage, Sc/RaytracingMeshDrawer.cs:86-90): the traced image is laid over the camera's
 * own rendering, one texel over the same pixel:  out.rgb = lerp(background.rgb, object.rgb, object.a)
 * = background + object.a * (object - background)  in fp32, out.a = 1.  All three images: count x 4 IEEE halfs
 * (RGBA16F, the format of lbvh_shade's output).  d_out may alias d_background. */
lbvh_status lbvh_compose(lbvh_context* ctx, const uint16_t* d_background_rgba16f, const uint16_t* d_object_rgba16f,
                         size_t count, uint16_t* d_out_rgba16f);

/* ---- dynamic scenes and secondary rays (extension; no reference counterpart) ----
 * The reference traces primary rays of a static mesh only (Sh/Raytracing/Raytracing.compute has no
 * secondary rays and no RNG; Sc/BVHConstructor.cs:41 zeroes the refit flags once, so it cannot even
 * rebuild).  BASELINE configs[4] asks for a per-frame rebuild + 4-bounce 1-spp path trace; the pieces
 * below provide it.  Parity for them is against this repo's own CPU restatement (oracle/), bit for bit:
 * everything is strict fp32, trig-free, and driven by a counter-based RNG. */

/* Rigid per-body animation: triangle i of the rest pose belongs to body d_body[i]; its three positions
 * and normals are rotated about the Y axis through that body's centre h/d_centres[body] by the angle
 * whose cosine / sine the HOST passes (no device trig), uv copied.  d_out may not alias d_rest. */
lbvh_status lbvh_animate(lbvh_context* ctx, const lbvh_triangle* d_rest, uint32_t n, const uint32_t* d_body,
                         const float* d_centres /* n_bodies x 4 floats (xyz, pad) */, float cos_angle, float sin_angle,
                         lbvh_triangle* d_out);

/* lbvh_animate followed by lbvh_build_scene as one call, with identical results: the moved triangles go to d_triangles AND
 * straight into the Morton / AABB stage (one kernel: as two, the 128-byte records were written and read back for the 36 bytes
 * of their positions).  The per-frame chain of a dynamic scene (BASELINE configs[4]); every other argument as lbvh_build_scene. */
lbvh_status lbvh_animate_build_scene(lbvh_context* ctx, const lbvh_triangle* d_rest, const uint32_t* d_body, const float* d_centres,
                                     float cos_angle, float sin_angle, lbvh_triangle* d_triangles, uint32_t n, uint32_t capacity,
                                     const float h_box_min[3], const float h_box_max[3], uint32_t* d_keys, uint32_t* d_indices,
                                     lbvh_aabb* d_aabb, lbvh_internal_node* d_internal, lbvh_leaf_node* d_leaf, lbvh_aabb* d_bvh,
                                     uint32_t flags);

/* One path vertex per pixel: 64 bytes. */
typedef struct lbvh_path_state {
    float origin[3];     uint32_t alive;     /* 1 while the path continues                      */
    float dir[3];        float    pad0;      /* unit direction of the ray to trace next          */
    float throughput[3]; float    pad1;
    float radiance[3];   float    alpha;     /* alpha = 1 if the primary ray hit, as Raytracing.compute:184 */
} lbvh_path_state;

/* Closest hit for `count` arbitrary rays taken from the path states (origin, dir; dead paths are skipped and
 * get a miss record): one ray per lane over the derived traversal scene (lbvh_build_fast_scene) in its four-wide
 * form — every node of that tree with its largest children opened once or twice: up to four child boxes per 128-byte
 * line, half the steps of the binary walk; made by the first call after a rebuild (collapse_wide_kernel, 0.06 ms at
 * 1 M triangles) — nearest child first, t-pruned, per-lane stack of 128 entries (three siblings can wait per level;
 * the reference's binary walk has 64, Raytracing.compute:113; the first 16 in LDS, deeper ones in device memory).
 * Accept rule = the reference's (own-AABB slab test, Moeller-Trumbore, t < best) plus t > t_min, which secondary
 * rays need to leave their surface and the reference lacks (Raytracing.compute:70); two triangles hit at the same t:
 * the lower triangle index, whatever order the walk meets them in; a computed t in front of its own triangle's box
 * does not count (both as LBVH_TRACE_FAST: see the note at the traversal flavours). */
lbvh_status lbvh_trace_rays(lbvh_context* ctx, const lbvh_path_state* d_states, size_t count, float t_min,
                            const lbvh_scene* h_scene, lbvh_hit* d_hits);

/* A ray of the caller's own: 32 bytes; arrays of them 16-byte aligned. */
typedef struct lbvh_ray {
    float origin[3]; float t_min;
    float dir[3];    float t_max;
} lbvh_ray;

/* Closest hit and occlusion for `count` rays of the caller's own, each with its own distance range, over the derived
 * traversal scene — the walk of lbvh_trace_rays (and lbvh_debug_ray_walker's choice of kernel), reading lbvh_ray records
 * directly: no live-ray pass, no list.
 *   Active ray: t_min < t_max (false when either bound is NaN).  An inactive ray is never walked; it gets the miss record
 *   (lbvh_trace_closest) or 0 (lbvh_trace_occluded).
 *   Direction: need not be unit length; t is measured in units of dir.  Zero components are allowed (+-inf inverse, as in
 *   every walker of this library).
 *   Candidates: with T = min(t_max, LBVH_MAX_FLOAT), a triangle is a candidate iff the ray passes the slab test of the
 *   triangle's own AABB with entry distance e, passes the Moeller-Trumbore test with the reference's rejections, t >= e (the
 *   accept rule at the traversal flavours above) and t_min < t < T.
 *   lbvh_trace_closest: d_hits[k] = {t, tri, u, v} of ray k's candidate with the least t; on equal t the lower triangle index.
 *   No candidate: {LBVH_MAX_FLOAT, 0, 0, 0}, the miss record of lbvh_trace_rays — never T.
 *   lbvh_trace_occluded: d_occluded[k] = 1 if ray k has any candidate, else 0.  The walk is the closest-hit walk (same
 *   near-first order) cut off at its first accepted candidate: never more node fetches or triangle tests per ray.
 * Hence: lbvh_trace_closest with t_max >= LBVH_MAX_FLOAT (or +inf) equals lbvh_trace_rays on a live path state with the same
 * origin, dir and t_min, word for word; with a finite t_max it equals that record if its t < T and is the miss record otherwise;
 * lbvh_trace_occluded equals (active && that t < T).
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG, as for lbvh_trace_rays),
 * are asynchronous on the context's stream, and use the context's ray scratch: like lbvh_trace_rays they drop the path
 * tracer's live-path list (see lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_rays or d_hits not
 * 16-byte aligned, d_occluded not 4-byte aligned, count > 2^32 - 1. */
lbvh_status lbvh_trace_closest(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene,
                               lbvh_hit* d_hits);
lbvh_status lbvh_trace_occluded(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene,
                                uint32_t* d_occluded);

/* A point query: 16 bytes; arrays of them 16-byte aligned. */
typedef struct lbvh_point_query {
    float p[3];
    float max_dist2;                /* squared search radius; +inf or >= LBVH_MAX_FLOAT = unbounded */
} lbvh_point_query;

/* The answer to one: 16 bytes, the shape of lbvh_hit. */
typedef struct lbvh_closest_point {
    float    dist2;                 /* squared distance; LBVH_MAX_FLOAT if none */
    uint32_t tri;                   /* ORIGINAL triangle index; 0 if none */
    float    u, v;                  /* barycentrics of b and c of the closest point: a + e1 * u + e2 * v; (0, 0) if none */
} lbvh_closest_point;

/* Nearest triangle and "anything within r" for `count` points, over the derived traversal scene in its four-wide form (see
 * lbvh_trace_rays): one query per lane, the nearest child box first, boxes farther than the best distance so far skipped.
 *   Active query: max_dist2 > 0 (false for NaN).  An inactive query is never walked; it gets the none-record
 *   {LBVH_MAX_FLOAT, 0, 0, 0} (lbvh_closest_point_query) or 0 (lbvh_within_distance).  So does, without a walk, a point with a
 *   NaN coordinate: all its distances are NaN and it has no candidate.  R = min(max_dist2, LBVH_MAX_FLOAT): LBVH_MAX_FLOAT is
 *   2139095040, so "unbounded" still means dist2 < 2.14e9 — a point farther than about 46 000 units from every triangle gets
 *   the none-record.
 *   Distance of a point to a triangle: defined on what the triangle line of the derived scene holds, a, e1 = b - a and
 *   e2 = c - a (the fp32 differences taken at build time), in strict fp32, every operation rounded on its own,
 *   dot(x, y) = (x0*y0 + x1*y1) + x2*y2.  The region test of Ericson, Real-Time Collision Detection 5.1.5, on a, e1, e2:
 *       ap = p - a
 *       d1 = dot(e1, ap)   d2 = dot(e2, ap)
 *       a11 = dot(e1, e1)  a12 = dot(e1, e2)  a22 = dot(e2, e2)
 *       d3 = d1 - a11   d4 = d2 - a12   d5 = d1 - a12   d6 = d2 - a22
 *       vc = d1*d4 - d3*d2    vb = d5*d2 - d1*d6    va = d3*d6 - d5*d4
 *       the first case that holds, in this order, gives (u, v):
 *         d1 <= 0 && d2 <= 0                       -> (0, 0)                     vertex a
 *         d3 >= 0 && d4 <= d3                      -> (1, 0)                     vertex b
 *         vc <= 0 && d1 >= 0 && d3 <= 0            -> (d1 / (d1 - d3), 0)        edge ab
 *         d6 >= 0 && d5 <= d6                      -> (0, 1)                     vertex c
 *         vb <= 0 && d2 >= 0 && d6 <= 0            -> (0, d2 / (d2 - d6))        edge ac
 *         va <= 0 && d4-d3 >= 0 && d5-d6 >= 0      -> w = (d4-d3) / ((d4-d3) + (d5-d6));  (1 - w, w)   edge bc
 *         otherwise                                -> den = 1 / ((va + vb) + vc);  (vb*den, vc*den)    face
 *       r = ap - (e1*u + e2*v)          (per component: ap_k - (e1_k*u + e2_k*v))
 *       dist2 = dot(r, r)
 *   (a comparison with a NaN is false: a degenerate triangle whose test reaches the face case has a NaN dist2.)
 *   Distance of a point to a box: per axis g = max(max(lo - p, p - hi), 0); box2 = (gx*gx + gy*gy) + gz*gz.
 *   Candidate: triangle i is a candidate for a query iff dist2_i < R and !(dist2_i < box2(own AABB_i)), the own AABB being
 *   scene.triangle_aabb[i], the box the derived scene keeps for the triangle's leaf.  A NaN dist2 is never a candidate.
 *   lbvh_closest_point_query: d_out[k] = {dist2, tri, u, v} of query k's candidate with the least dist2; on equal dist2 the lower
 *   original triangle index, whatever order the walk meets them in.  No candidate: the none-record, never R.
 *   lbvh_within_distance: d_flags[k] = 1 if query k has any candidate, else 0.  The walk is the closest-point walk (same
 *   nearest-first order) cut off at its first accepted candidate: never more node fetches or triangle tests per query.
 * Why the record does not depend on the order of the walk (the argument of the accept rule for rays at the traversal flavours
 * above, with box2 in the place of the entry distance): fp32 subtraction, max, multiplication of non-negatives and addition are
 * monotone, and every box of the derived tree, binary or four-wide, is the exact min / max union of what is below it, so
 * box2(ancestor) <= box2(leaf) <= dist2 for every candidate.  A subtree skipped because box2 > best (strictly) cannot hold a
 * candidate at or below best.  A dist2 below its own box's distance is fp32 noise of the triangle arithmetic (the padded box
 * contains the triangle); on ordinary meshes the rule rejects nothing.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream, and use the context's ray scratch: like lbvh_trace_rays they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_queries or d_out not 16-byte aligned, d_flags not
 * 4-byte aligned, count > 2^32 - 1.
 * Pass active queries only where time matters: a wave takes a run of consecutive queries, and runs of inactive ones leave
 * some waves with little to do and others with all of it (as inactive rays do for lbvh_trace_closest). */
lbvh_status lbvh_closest_point_query(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                     lbvh_closest_point* d_out);
lbvh_status lbvh_within_distance(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                 uint32_t* d_flags);

/* The k nearest triangles of `count` points, 1 <= k <= LBVH_K_CLOSEST_MAX, over the same scene by the same walk.
 *   Active query, R = min(max_dist2, LBVH_MAX_FLOAT), dist2, box2 and the candidate predicate are exactly those of
 *   lbvh_closest_point_query above: dist2_i < R && !(dist2_i < box2(own AABB_i)); a NaN dist2 is never a candidate, a point with a
 *   NaN coordinate and an inactive query have none and are never walked.
 *   Order: a query's candidates are ordered by (dist2 ascending, original triangle index ascending) — a total order, a
 *   candidate's dist2 being a non-NaN, non-negative float.
 *   Output: d_out holds count * k records, query-major.  With m_q = min(k, the number of candidates of query q),
 *   d_out[q * k + j] = {dist2, tri, u, v} of query q's j-th candidate in that order for j < m_q, and the none-record
 *   {LBVH_MAX_FLOAT, 0, 0, 0} for m_q <= j < k.  Every one of the count * k records is written by the call — the caller does
 *   not pre-fill —, also for inactive queries.  d_found[q] = m_q; d_found may be NULL.
 *   Hence: with k = 1 the output equals lbvh_closest_point_query's word for word; record 0 of every row equals that query's
 *   record for every k; d_found[q] >= 1 exactly when lbvh_within_distance gives 1; and row q is the first m_q elements of
 *   segment q of lbvh_gather_within_distance sorted by (dist2, tri), with their distances.
 * Why the rows do not depend on the order of the walk (the argument at lbvh_closest_point_query, "best so far" read as "k-th
 * best so far"): a query's pruning bound is R while fewer than k candidates are held and the dist2 of the k-th held after
 * that; a slot is skipped only if box2 > bound, strictly.  Every candidate below a skipped slot has dist2 >= box2(leaf) >=
 * box2(slot) > bound, so it sorts after the k-th held whatever its index; a candidate with dist2 == bound is never skipped,
 * and the index comparison decides it.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the
 * context's stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL d_queries / h_scene / d_out, k == 0 or k > LBVH_K_CLOSEST_MAX,
 * d_queries or d_out not 16-byte aligned, d_found not 4-byte aligned, count > 2^32 - 1.  The index q * k is formed in 64 bits.
 * One query per lane, each with a list of k entries in the wave's LDS (768 * k bytes per wave, sized from k at the call): the
 * cost grows with k through the wider bound (more boxes entered), the insertions, and, from k = 16 up, fewer waves per CU. */
#define LBVH_K_CLOSEST_MAX 32
lbvh_status lbvh_k_closest_points(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count, uint32_t k,
                                  const lbvh_scene* h_scene, lbvh_closest_point* d_out, uint32_t* d_found);

/* Overlap queries: WHICH triangles are here — all triangles whose box touches a box, all triangles within a distance of a point —
 * as a CSR list, over the derived traversal scene in its four-wide form (the scene lbvh_closest_point_query walks).
 *   lbvh_box_overlaps: query k is an lbvh_aabb (_dummy0 / _dummy1 are not read).  Active query: min[a] <= max[a] on all three
 *   axes (false when a bound is NaN).  Triangle i is a candidate of an active query Q iff, with A = scene.triangle_aabb[i] (the
 *   padded own box the derived scene keeps for the triangle's leaf), Q.min[a] <= A.max[a] && A.min[a] <= Q.max[a] for a = 0, 1, 2.
 *   Closed intervals: touching boxes overlap.  Comparisons only, nothing is rounded.  A broad phase on the triangles' BOXES by
 *   design (no exact triangle-against-box test): the array lbvh_morton_aabb writes for ANOTHER mesh can be passed unchanged as
 *   d_boxes, which gives the candidate pairs of a mesh-against-mesh test in one call.
 *   lbvh_gather_within_distance: active query, R, dist2, box2 and the candidate predicate are exactly those of
 *   lbvh_within_distance above: dist2_i < R && !(dist2_i < box2(own AABB_i)); a NaN dist2 is never a candidate, a point with a
 *   NaN coordinate and an inactive query have none.  Segment k is non-empty exactly when lbvh_within_distance gives 1, and the
 *   triangle lbvh_closest_point_query reports is in it.
 *   Why the list does not depend on the walk: every box of the derived tree, binary or four-wide, is the exact min / max union of
 *   what lies below it, so every ancestor of a candidate's leaf passes the same comparisons (box form) or has box2 <= box2(leaf)
 *   <= dist2 < R (distance form, the argument at lbvh_closest_point_query without the shrinking bound).  The walk skips exactly
 *   the slots that fail; each triangle is one leaf, so each candidate appears once.
 * Output, the same for both:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[k] = the number of candidates of queries 0 .. k-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_tris, `capacity` words of 32 bits: segment k = d_tris[d_offsets[k] .. d_offsets[k+1]) = the ORIGINAL triangle indices of
 *   query k's candidates, each exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT (the
 *   four-wide form does not keep children in range order); sort a segment if a canonical order is needed.
 *   Overflow: no word at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; words
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn whether everything fitted and, if
 *   not, what to allocate.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_tris may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill).  d_tris == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream, and use the context's ray scratch: they drop the path tracer's live-path list (see lbvh_path_bounce).
 * count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL d_boxes /
 * d_queries / h_scene / d_offsets, queries not 16-byte aligned, d_offsets not 8-byte aligned, d_tris not 4-byte aligned,
 * count > 2^32 - 1.
 * One query per lane: a query with very many candidates keeps its lane busy while the rest of its wave idles — many small
 * queries run far better than a few huge ones. */
lbvh_status lbvh_box_overlaps(lbvh_context* ctx, const lbvh_aabb* d_boxes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);
lbvh_status lbvh_gather_within_distance(lbvh_context* ctx, const lbvh_point_query* d_queries, size_t count,
                                        const lbvh_scene* h_scene, uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);

/* How many surfaces a ray crosses, and crossing parities of points along fixed directions (inside / outside tests).
 *   lbvh_count_hits: active ray, candidate set and T = min(t_max, LBVH_MAX_FLOAT) exactly those of lbvh_trace_closest (the
 *   own-box slab test with entry e, Moeller-Trumbore with the reference's rejections, t >= e, t_min < t < T).  d_counts[k] =
 *   the number of triangles that are candidates of ray k, every member counted once: two triangles at the same t count 2, a
 *   ray through a shared edge counts every triangle that passes the test.  0 for an inactive ray.  Hence d_counts[k] >= 1
 *   exactly when lbvh_trace_occluded gives 1.  The walk is lbvh_trace_rays' (lbvh_debug_ray_walker's choice of kernel)
 *   without the shrinking bound: boxes entered beyond T are skipped, none is skipped for the candidates found so far.
 *   lbvh_point_crossings: for point k and direction j, the ray {origin = p_k, t_min = 0, dir = dirs[j], t_max = +inf}; bit j
 *   of d_parity[k] is that ray's lbvh_count_hits count AND 1, bits >= n_dirs are 0.  max_dist2 is not read: the buffer given
 *   to lbvh_closest_point_query can be passed unchanged (closest point + parity = a signed distance).  No
 *   special cases: a point with a NaN coordinate fails every box test and gets 0 from the definition itself.  Four-wide walk
 *   only (lbvh_debug_ray_walker does not apply): one lane walks its point's directions one after the other, the rays are
 *   made on the fly (never written to memory) and d_parity[k] is written with one plain store per point — the caller does
 *   not pre-zero it.  h_dirs: n_dirs x 3 floats on the host, read during the call; need not be unit length.
 * Why the count does not depend on the walk (the argument of the accept rule at the traversal flavours above, without the
 * shrinking bound): every box of the derived tree, binary or four-wide, is the exact min / max union of what lies below it and
 * the slab arithmetic is monotone, so every ancestor of a candidate's leaf passes its slab test with entry <= e <= t < T.  The
 * walk may therefore skip only boxes that the ray misses, or whose entry is > T; it must never prune on the exit distance,
 * since a candidate's computed t may lie beyond its own box's exit.  Each triangle is exactly one leaf, so each candidate is
 * counted exactly once.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream, and use the context's ray scratch: they drop the path tracer's live-path list (see lbvh_path_bounce).
 * count == 0 is a no-op.  Rejected: NULL pointers (h_dirs included), d_rays or d_points not 16-byte aligned, d_counts or
 * d_parity not 4-byte aligned, count > 2^32 - 1, n_dirs outside 1 .. LBVH_CROSSING_MAX_DIRS, a direction with a non-finite
 * component or with all three components zero. */
lbvh_status lbvh_count_hits(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene,
                            uint32_t* d_counts);

#define LBVH_CROSSING_MAX_DIRS 32
lbvh_status lbvh_point_crossings(lbvh_context* ctx, const lbvh_point_query* d_points, size_t count,
                                 const float* h_dirs /* n_dirs x 3 */, uint32_t n_dirs, const lbvh_scene* h_scene,
                                 uint32_t* d_parity);

/* The first k hits along `count` rays, 1 <= k <= LBVH_K_CLOSEST_MAX (the same list as lbvh_k_closest_points), over the same
 * scene by the four-wide closest-hit walk.
 *   Active ray, T = min(t_max, LBVH_MAX_FLOAT) and the candidate set are exactly those of lbvh_trace_closest and lbvh_count_hits:
 *   the own-box slab test with entry e, Moeller-Trumbore with the reference's rejections, t >= e, t_min < t < T.  A NaN t is never
 *   a candidate; an inactive ray (!(t_min < t_max), NaN bounds included) has none and is never walked.
 *   Order: a ray's candidates are ordered by (t ascending, original triangle index ascending).  t is compared as fp32 values:
 *   -0 and +0 are equal and the index decides between them.
 *   Output: d_hits holds count * k records, ray-major.  With m_q = min(k, the number of candidates of ray q),
 *   d_hits[q * k + j] = {t, tri, u, v} of ray q's j-th candidate in that order for j < m_q, and the miss record
 *   {LBVH_MAX_FLOAT, 0, 0, 0} for m_q <= j < k.  Every one of the count * k records is written by the call — the caller does
 *   not pre-fill —, also for inactive rays (rows of miss records).  d_found[q] = m_q; d_found may be NULL.
 *   Hence: with k = 1 the output equals lbvh_trace_closest's word for word; record 0 of every row equals that call's record for
 *   every k; d_found[q] == min(k, lbvh_count_hits' d_counts[q]); and d_found[q] >= 1 exactly when lbvh_trace_occluded gives 1.
 * Why the rows do not depend on the order of the walk (the argument at lbvh_k_closest_points with entry distances in place of
 * box2): a ray's pruning bound is T while fewer than k candidates are held and the t of the k-th held after that; a slot is
 * skipped only if the ray misses its box or its entry is > bound, strictly.  Every candidate below a skipped slot has
 * t >= e(leaf) >= e(slot) > bound, so it sorts after the k-th held whatever its index; a candidate with t == bound is never
 * skipped, and the index comparison decides it.  Nothing is pruned on a box's exit distance (see the note at lbvh_count_hits).
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the
 * context's stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path list (see
 * lbvh_path_bounce); a failed growth of that scratch is LBVH_ERR_OUT_OF_MEMORY with nothing written.  count == 0 is a no-op.
 * Rejected: NULL ctx / d_rays / h_scene / d_hits, k == 0 or k > LBVH_K_CLOSEST_MAX, d_rays or d_hits not 16-byte aligned,
 * d_found not 4-byte aligned, count > 2^32 - 1.  The index q * k is formed in 64 bits.  Four-wide walk only
 * (lbvh_debug_ray_walker does not apply).  One ray per lane, each with a list of k entries in the wave's LDS (768 * k bytes per
 * wave, sized from k at the call): the cost grows with k through the wider bound (more boxes entered), the insertions, and, at
 * large k, fewer waves per CU. */
lbvh_status lbvh_trace_k_closest(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, uint32_t k,
                                 const lbvh_scene* h_scene, lbvh_hit* d_hits, uint32_t* d_found);

/* EVERY hit along `count` rays as a CSR list — the "all" form of the ray queries (nearest: lbvh_trace_closest, any:
 * lbvh_trace_occluded, how many: lbvh_count_hits, first k <= 32: lbvh_trace_k_closest) —, over the same scene by the four-wide walk
 * of lbvh_count_hits, in the count -> device-side scan -> fill shape of the overlap queries.
 *   Active ray, T = min(t_max, LBVH_MAX_FLOAT) and the candidate set are exactly those of lbvh_trace_closest and lbvh_count_hits:
 *   the own-box slab test with entry e, Moeller-Trumbore with the reference's rejections, t >= e, t_min < t < T.  A NaN t is never
 *   a candidate; an inactive ray (!(t_min < t_max), NaN bounds included) has none and is never walked.
 * Output:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[q] = the number of candidates of rays 0 .. q-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_hits, `capacity` records of 16 bytes: segment q = d_hits[d_offsets[q] .. d_offsets[q+1]) = {t, tri, u, v} of every candidate
 *   of ray q, each exactly once; the four words are the ones lbvh_trace_closest would write if that candidate were the nearest.
 *   THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT (the convention of the overlap queries: the four-wide
 *   form does not keep children in range order, and the walk enters boxes in slot order, not by distance).  Every record carries
 *   its t: sort a segment by (t, tri) if an order is needed — two candidates of a ray never share a triangle index, so that
 *   order is canonical.  lbvh_sort_hit_segments (below) puts every segment into that order on the device, in place; the first 32
 *   in order are lbvh_trace_k_closest.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[q+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn whether everything fitted and, if
 *   not, what to allocate.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_hits may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill).  d_hits == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Hence, for every ray q with m = d_offsets[q+1] - d_offsets[q]: m == lbvh_count_hits' d_counts[q]; m >= 1 exactly when
 * lbvh_trace_occluded gives 1; the least element of segment q by (t, tri) is lbvh_trace_closest's record (the miss record when
 * m == 0); and its first min(k, m) elements by (t, tri) are the first min(k, m) records of row q of lbvh_trace_k_closest, word
 * for word (t compared as fp32 values, as there).
 * Why the list does not depend on the walk: the argument at lbvh_count_hits.  Every ancestor of a candidate's leaf passes its
 * slab test with entry <= e <= t < T, and the walk skips only boxes that the ray misses or whose entry is > T; the bound is T
 * from the first step to the last — nothing shrinks —, and nothing is pruned on a box's exit distance.  Each triangle is
 * exactly one leaf, so each candidate is met exactly once.  The count walk and the fill walk are the same kernel making the same
 * decisions, so a segment never outgrows its slot.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the
 * context's stream, and uses the context's ray scratch: it drops the path tracer's live-path list (see lbvh_path_bounce); a
 * failed growth of that scratch is LBVH_ERR_OUT_OF_MEMORY with nothing written.  count == 0 is a no-op: nothing is enqueued and
 * no buffer is touched, d_offsets[0] included.  Rejected: NULL ctx / d_rays / h_scene / d_offsets, d_rays or d_hits not 16-byte
 * aligned, d_offsets not 8-byte aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply);
 * lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the overlap
 * queries (the stats of both walks are added: the full form reports twice the count-only form's).
 * One ray per lane: a ray with very many hits keeps its lane busy while the rest of its wave idles — many ordinary rays run far
 * better than a few that cross thousands of layers. */
lbvh_status lbvh_gather_hits(lbvh_context* ctx, const lbvh_ray* d_rays, size_t count, const lbvh_scene* h_scene,
                             uint64_t* d_offsets, lbvh_hit* d_hits, uint64_t capacity);

/* Every segment of a CSR list put into ascending key order, in place, on the device: the pass after lbvh_gather_hits
 * (lbvh_sort_hit_segments) and after lbvh_box_overlaps / lbvh_gather_within_distance (lbvh_sort_index_segments), for a consumer
 * that needs the segments ordered.  A stand-alone pass over any CSR list: it needs no scene.
 *   d_offsets: count + 1 words of 64 bits, exactly as the three queries write them; read only.  `capacity`: the number of records
 *   (d_hits) or words (d_tris) of the data buffer — the capacity that was given to the query.
 *   What is sorted: every segment q with d_offsets[q] <= d_offsets[q+1] <= capacity is rearranged in place into ascending key
 *   order; after the call it is a permutation of what it was.
 *   What is left alone: a segment that does not fit the capacity is left untouched (its records are unspecified anyway), and so is
 *   one whose pair of offsets decreases; no record at index >= capacity is ever read or written; d_offsets is never written.
 *   (Offsets that the queries cannot produce — fitting segments that overlap each other — leave the records of the overlap
 *   unspecified, still inside the capacity.)
 *   Key of a hit record: the 64-bit pair (K(t), tri), K(t) the more significant half.  K maps the fp32 value to an unsigned word
 *   that orders as the values do; with w = the 32 bits of t, operation by operation:
 *     if ((w & 0x7FFFFFFF) > 0x7F800000) K = 0xFFFFFFFF          every NaN: one class, after +inf (K(+inf) = 0xFF800000)
 *     else { if (w == 0x80000000) w = 0;                           -0 and +0 map to the same word
 *            K = (w & 0x80000000) ? ~w : (w | 0x80000000); }       negative values reversed below the positive ones
 *   This is the order of lbvh_trace_k_closest (t compared as fp32 values, the index decides), made total: lbvh_gather_hits never
 *   writes a NaN, but the call is defined on any input.  u and v travel with their record and are not compared.
 *   Key of an index segment: the 32-bit word, ascending.
 *   Records of equal key come out in an unspecified relative order: THE SORT IS NOT STABLE.
 * Hence: after lbvh_gather_hits followed by lbvh_sort_hit_segments with the same d_offsets and capacity, every fitting segment q
 * is in (t, tri) order — two candidates of a ray never share a triangle index, so the order is canonical and the segment equals
 * the brute force's (tests/gather_hits_reference.py) word for word; with m its length, its first min(k, m) records are the first
 * min(k, m) records of row q of lbvh_trace_k_closest, and its first record is lbvh_trace_closest's.  After lbvh_box_overlaps or
 * lbvh_gather_within_distance followed by lbvh_sort_index_segments, every fitting segment is strictly ascending (each candidate
 * appears once).
 * Asynchronous on the context's stream with no host wait: segment lengths are only ever read on the device.  Takes NO context
 * scratch: it does not touch the ray scratch and does NOT drop the path tracer's live-path list (see lbvh_path_bounce) — unless
 * the data buffer is that frame's d_hits, which it then writes like any other call.  No derived scene is needed: a context that
 * never built one may call it.  count == 0 is a no-op; capacity == 0 is a no-op that still returns LBVH_OK.  Rejected with
 * LBVH_ERR_INVALID_ARG: NULL ctx / d_offsets / d_hits / d_tris, d_offsets not 8-byte aligned, d_hits not 16-byte aligned, d_tris
 * not 4-byte aligned, count > 2^32 - 1.  A segment may have any length up to the capacity; positions are formed in 64 bits.
 * Segments of up to 256 records are sorted 64 queries at a time by one wave, in LDS; a longer one is sorted by ONE workgroup (up
 * to 4 096 records in LDS, beyond that in O(n log^2 n) exchanges partly on device memory): many ordinary segments run far better
 * than one of a million records. */
lbvh_status lbvh_sort_hit_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, lbvh_hit* d_hits, uint64_t capacity);
lbvh_status lbvh_sort_index_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count, uint32_t* d_tris, uint64_t capacity);

/* The same pass for the CSR lists of 32-byte records: lbvh_contact (lbvh_capsule_contacts), lbvh_box_contact (lbvh_obb_contacts),
 * lbvh_tri_closest (lbvh_triangle_gather_within_distance), lbvh_tri_segment (lbvh_triangle_intersection_segments) and
 * lbvh_plane_segment (lbvh_plane_sections), all declared below.  d_records holds `capacity` records of 32 bytes, read as eight
 * 32-bit words (word 0 first); the array is 16-byte aligned, like every 32-byte record array of the library.
 * The contract is that of the two calls above, word for word, with "record" for "hit": which segments count as fitting
 * (d_offsets[q] <= d_offsets[q+1] <= capacity) and come out as a permutation of what they were; that a segment which does not fit
 * or whose pair of offsets decreases is left untouched, that no record at index >= capacity is ever read or written and that
 * d_offsets is never written; that THE SORT IS NOT STABLE; asynchronous with no host wait, NO context scratch, no scene, the path
 * tracer's live-path list kept (unless the buffer is that frame's d_hits); count == 0 is a no-op and capacity == 0 is a no-op that
 * returns LBVH_OK.  Rejected with LBVH_ERR_INVALID_ARG: NULL ctx / d_offsets / d_records, d_offsets not 8-byte aligned, d_records
 * not 16-byte aligned, count > 2^32 - 1, and order > 2 (checked first: also with count == 0).
 *   Key under `order`, K the K of lbvh_sort_hit_segments, operation by operation:
 *     LBVH_SORT_RECORDS_ASCENDING   the 64-bit pair (K(word 0), word 1), K(word 0) the more significant half.  Word 0 is dist2 or
 *                                   depth as an fp32 value: -0 sorts with +0, every NaN is one class after +inf.  Word 1 is `tri` in
 *                                   lbvh_contact, lbvh_box_contact and lbvh_tri_closest, and decides ties.
 *     LBVH_SORT_RECORDS_DESCENDING  (D(word 0), word 1) ascending, with D = 0xFFFFFFFF for a NaN and ~K(word 0) otherwise.  K of a
 *                                   value that is not a NaN is never 0xFFFFFFFF and never 0, so D reverses K below the NaNs: the
 *                                   greatest value first, on equal values (-0 and +0 are equal) the lower word 1 first, NaNs still
 *                                   last.
 *     LBVH_SORT_RECORDS_BY_TRI      word 3, ascending: the `tri` of lbvh_tri_segment and lbvh_plane_segment.
 *   Words that are not in the key travel with their record and are not compared.
 * Hence — a candidate appears once per segment, so all three orders are canonical on what the five queries write:
 *   after lbvh_triangle_gather_within_distance + ASCENDING (same d_offsets and capacity), the first record of a non-empty fitting
 *   segment is lbvh_triangle_closest_point's record for that query in all eight words (least dist2, then the lower index: the same
 *   rule; a candidate's dist2 is below the bound, never a NaN);
 *   after lbvh_capsule_contacts or lbvh_obb_contacts + DESCENDING, the first record is lbvh_capsule_deepest's / lbvh_obb_deepest's
 *   in all eight words — AS LONG AS NO DEPTH OF THE SEGMENT IS A NaN: the deepest rule replaces its record when the new depth is
 *   greater, or is not less and the index is lower, so a NaN depth compares as equal to everything there and which record wins
 *   depends on the walk, while here a NaN always sorts last;
 *   after lbvh_triangle_intersection_segments or lbvh_plane_sections + BY_TRI, the `tri` words of a fitting segment are strictly
 *   ascending and the segment equals the numpy restatement sorted by `tri` (tests/record_sort_reference.py).
 * Segments of up to 256 records are sorted 64 queries at a time by one wave; a longer one by ONE workgroup, in chunks of 1 024
 * records in LDS and, beyond one chunk, in O(n log^2 n) exchanges partly on device memory.  The network orders 16-byte entries
 * (key, source slot, rank), not the records: every record is moved once per pass over its chunk. */
#define LBVH_SORT_RECORDS_ASCENDING   0u   /* key (K(word 0), word 1)          */
#define LBVH_SORT_RECORDS_DESCENDING  1u   /* key (D(word 0), word 1)          */
#define LBVH_SORT_RECORDS_BY_TRI      2u   /* key word 3                       */
lbvh_status lbvh_sort_record_segments(lbvh_context* ctx, const uint64_t* d_offsets, size_t count,
                                      void* d_records, uint64_t capacity, uint32_t order);

/* A moving sphere: 32 bytes, arrays 16-byte aligned: lbvh_ray with the radius where t_min is. */
typedef struct lbvh_sphere_ray {
    float origin[3]; float radius;
    float dir[3];    float t_max;
} lbvh_sphere_ray;

/* First contact of `count` moving spheres with the mesh (a sweep, "sphere cast"), over the derived traversal scene in its four-wide
 * form by the per-lane walk of lbvh_trace_closest.  The sphere's centre moves as c(t) = origin + dir * t for 0 <= t < T,
 * T = min(t_max, LBVH_MAX_FLOAT); dir need not be unit length and t is in units of dir.
 *   Active cast: radius > 0 and radius < +inf, t_max > 0, no NaN in origin, every dir component finite, dot(dir, dir) > 0 (the
 *   fp32 value; all false for NaN).  An inactive cast is never walked; it gets the miss record {LBVH_MAX_FLOAT, 0, 0, 0}
 *   (lbvh_sphere_cast) or 0 (lbvh_sphere_cast_any).
 *   Time of contact with one triangle: defined on a, e1, e2 of the triangle's line of the derived scene, in strict fp32, every
 *   operation rounded on its own, dot as at lbvh_closest_point_query, cross(x, y) per component x1*y2 - x2*y1 (two products, one
 *   difference), sqrtf and / correctly rounded.  With o = origin, d = dir, r = radius, R2 = r*r, dd = dot(d, d), and a11, a12, a22
 *   of lbvh_closest_point_query:
 *     start overlap   d0 = dist2 of lbvh_closest_point_query for the point o.  If d0 <= R2 the time is 0 (+0) and no other
 *                     feature is looked at.
 *     Otherwise the time is the least t among the features below that are valid and have t >= 0, taken in this order, a later
 *     one replacing an earlier one only when strictly less (which fixes the sign of a zero); no such feature: no time.
 *     face            n = cross(e1, e2)   h = r * sqrtf(dot(n, n))   m = o - a   s = dot(m, n)   dn = dot(d, n)
 *                     sg = (s >= 0 ? 1 : -1)   s' = s*sg   dn' = dn*sg   t = (h - s') / dn'
 *                     q = c(t) - a  (per component (o_k + d_k*t) - a_k)   d1 = dot(e1, q)   d2 = dot(e2, q)
 *                     det = a11*a22 - a12*a12   u = (a22*d1 - a12*d2) / det   v = (a11*d2 - a12*d1) / det
 *                     valid iff s' > h && dn' < 0 && u >= 0 && v >= 0 && u + v <= 1
 *     three edges     (P, E) = (a, e1), (a, e2), (a + e1, e2 - e1), P and E per component in fp32:   m = o - P
 *                     ee = dot(E, E)   me = dot(m, E)   de = dot(d, E)
 *                     A = ee*dd - de*de   B = ee*dot(m, d) - de*me   Cq = ee*(dot(m, m) - R2) - me*me   disc = B*B - A*Cq
 *                     t = (-B - sqrtf(disc)) / A   s = me + t*de
 *                     valid iff A > 0 && disc >= 0 && 0 <= s && s <= ee
 *     three vertices  P = a, a + e1, a + e2:   m = o - P   B = dot(m, d)   Cq = dot(m, m) - R2   disc = B*B - dd*Cq
 *                     t = (-B - sqrtf(disc)) / dd          valid iff disc >= 0
 *   (a comparison with a NaN is false: a NaN t never counts.)  The face is the slab of thickness r on the side the sphere starts
 *   on, the edges are infinite cylinders cut to the segment, the vertices are spheres; a start inside a cylinder or a sphere that
 *   is not a start overlap has a negative root there and the contact comes from another feature.
 *   Candidate: triangle i is a candidate iff it has a time t_i, t_i < T, the ray (origin, dir) passes the slab test of the
 *   triangle's own box grown by r — scene.triangle_aabb[i] with min - r and max + r, one fp32 operation per bound, the slab test of
 *   every walker of this library — with entry distance e_i, and !(t_i < e_i).  A ray that misses the grown box has no candidate there.
 *   lbvh_sphere_cast: d_hits[k] = {t, tri, u, v} of cast k's candidate with the least t (compared as fp32 values: -0 and +0 are
 *   equal); on equal t the lower original triangle index, whatever order the walk meets them in.  (u, v) are those
 *   lbvh_closest_point_query's definition gives for the point c(t) (per component o_k + d_k*t) and this triangle: the barycentrics
 *   of the contact point a + e1*u + e2*v; the contact normal is (c(t) - contact point) / r.  No candidate: the miss record, never T.
 *   lbvh_sphere_cast_any: d_flags[k] = 1 if cast k has any candidate, else 0.  The walk is the same (same near-first order) cut off
 *   at its first accepted candidate: never more node fetches or triangle tests per cast.
 * Why the record does not depend on the order of the walk (the argument of lbvh_trace_closest with grown boxes): lo - r and hi + r
 * are monotone in lo and hi, and every box of the derived tree is the exact min / max union of what is below it, so the grown box
 * of an ancestor contains the grown box of everything below it exactly in fp32; slab entries grow from a box to any box inside
 * it, so e(ancestor) <= e(leaf) <= t for every candidate.  A slot is skipped only if the ray misses its grown box or its entry is
 * > best, strictly: a subtree skipped that way holds no candidate at or below best.  Nothing is pruned on a box's exit distance.
 * A time in front of its own grown box is fp32 noise (the sphere touching the triangle at c(t) puts c(t) inside the grown box); on
 * ordinary meshes the rule rejects next to nothing.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_casts or d_hits not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_stack_split,
 * lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the point queries.  The cost grows with the radius: every box
 * is r larger on each side. */
lbvh_status lbvh_sphere_cast(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                             lbvh_hit* d_hits);
lbvh_status lbvh_sphere_cast_any(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                 uint32_t* d_flags);

/* A moving capsule: 48 bytes, arrays 16-byte aligned: lbvh_sphere_ray and the axis. */
typedef struct lbvh_capsule_ray {
    float origin[3]; float radius;     /* p: one end of the axis */
    float dir[3];    float t_max;
    float axis[3];   uint32_t _pad;    /* h: the other end is origin + axis; _pad is not read */
} lbvh_capsule_ray;

/* First contact of `count` moving capsules with the mesh (a "capsule cast": the shape a character controller sweeps), over the
 * derived traversal scene in its four-wide form by the walk of lbvh_sphere_cast.  A capsule is every point within `radius` of its
 * axis, the segment [c, c + h] with h = axis.  The axis moves without turning: c(t) = origin + dir * t for 0 <= t < T,
 * T = min(t_max, LBVH_MAX_FLOAT); dir need not be unit length and t is in units of dir.
 *   Active cast: the conditions of lbvh_sphere_cast on radius, t_max, origin and dir, and every component of axis finite.  axis = 0
 *   is allowed (a sphere, by this definition's arithmetic).  An inactive cast is never walked; it gets the miss record
 *   {LBVH_MAX_FLOAT, 0, 0, 0} (lbvh_capsule_cast) or 0 (lbvh_capsule_cast_any).
 *   The definition goes through lbvh_sphere_cast: the capsule touches a triangle exactly when the sphere (c, radius) touches the
 *   prism "triangle + segment [0, -h]", and the surface of that prism is eight triangles.
 *   Derived triangles of a scene triangle with the line a, e1, e2: A = a, B = a + e1, C = a + e2, A' = A - h, B' = B - h,
 *   C' = C - h, each per component in fp32.  Derived triangle j has a_j = P, e1_j = Q - P, e2_j = R - P, per component in fp32, for
 *     j = 0   (P, Q, R) = (A, B, C): the line's own a, e1, e2 as stored, not formed again
 *     j = 1   (A', B', C')
 *     j = 2   (A, B, A')      j = 3   (B', A', B)        the side over AB
 *     j = 4   (B, C, B')      j = 5   (C', B', C)        the side over BC
 *     j = 6   (C, A, C')      j = 7   (A', C', A)        the side over CA
 *   (each side is a parallelogram cut along one diagonal: the two triangles share it and cover the side).
 *   Time with one scene triangle: t_j = the time lbvh_sphere_cast defines for the sphere (origin, radius, dir) against derived
 *   triangle j (+0 on a start overlap there; none if that definition gives none).  The triangle's time is the least t_j, taken in
 *   the order j = 0 .. 7, a later one replacing an earlier one only when strictly less, compared as fp32 values.  If no t_j equals
 *   0 and pierce(origin, axis; a, e1, e2) of lbvh_triangle_intersections passes with its t = t_p (0 <= t_p <= 1), the time is +0:
 *   the axis goes through the face at the start with both ends and all edges farther than the radius (the sphere's centre is inside
 *   the prism).  A NaN never counts.
 *   Candidate: triangle i is a candidate iff it has a time t_i, t_i < T, the ray (origin, dir) passes the slab test of the
 *   triangle's own box grown by the axis and the radius — scene.triangle_aabb[i] with, per axis k,
 *   min' = (min_k - max(h_k, 0)) - r and max' = (max_k - min(h_k, 0)) + r, two fp32 operations per bound, the slab test of every
 *   walker of this library — with entry distance e_i, and !(t_i < e_i).  (c is in the grown box exactly when some point of the
 *   axis is within r of the own box, per axis.)
 *   lbvh_capsule_cast: d_hits[k] = {t, tri, u, v} of cast k's candidate with the least t (compared as fp32 values); on equal t the
 *   lower original triangle index, whatever order the walk meets them in.  With j the derived triangle that gave the time, (u', v')
 *   lbvh_closest_point_query's barycentrics of the point c(t) (per component o_k + d_k*t) on derived triangle j, the axis parameter
 *   of the touching point is s = 0 for j = 0, 1 for j = 1, v' for j = 2, 4, 6, 1 - v' for j = 3, 5, 7, and t_p in the pierce case;
 *   (u, v) are lbvh_closest_point_query's for the point x = c(t) + h*s (per component (o_k + d_k*t) + h_k*s) and the scene triangle.
 *   The contact point on the mesh is q = a + e1*u + e2*v; x is the point of the axis nearest to it, s = clamp(dot(q - c(t), h) /
 *   dot(h, h), 0, 1) recovers it, and the contact normal is (x - q) / r (for t = 0: any separating direction; x - q may be 0).
 *   No candidate: the miss record, never T.
 *   lbvh_capsule_cast_any: d_flags[k] = 1 if cast k has any candidate, else 0.  The walk is the same (same near-first order) cut
 *   off at its first accepted candidate: never more node fetches or triangle tests per cast.
 * Why the record does not depend on the order of the walk (the argument of lbvh_sphere_cast): (lo - max(h, 0)) - r and
 * (hi - min(h, 0)) + r are each two operations monotone in lo and hi, and every box of the derived tree is the exact min / max union
 * of what is below it, so the grown box of an ancestor contains the grown box of everything below it exactly in fp32; slab entries
 * grow from a box to any box inside it, so e(ancestor) <= e(leaf) <= t for every candidate.  A slot is skipped only if the ray
 * misses its grown box or its entry is > best, strictly: a subtree skipped that way holds no candidate at or below best.  Nothing
 * is pruned on a box's exit distance.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_casts or d_hits not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_stack_split,
 * lbvh_debug_ray_stack_limit, lbvh_ray_stats_target and lbvh_debug_ray_waves apply as to the sphere cast.  The cost grows with the
 * radius and the axis (every box is larger by both) and each tested triangle costs up to eight sphere tests. */
lbvh_status lbvh_capsule_cast(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                              lbvh_hit* d_hits);
lbvh_status lbvh_capsule_cast_any(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                  uint32_t* d_flags);

/* A moving box: 80 bytes, arrays 16-byte aligned. */
typedef struct lbvh_box_ray {
    float centre[3]; float t_max;
    float dir[3];    uint32_t _pad0;
    float ax[3];     uint32_t _pad1;   /* three half-axis vectors: the box is                */
    float ay[3];     uint32_t _pad2;   /* { centre + s0*ax + s1*ay + s2*az : |s_i| <= 1 }   */
    float az[3];     uint32_t _pad3;   /* pads are not read                                  */
} lbvh_box_ray;

/* lbvh_box_cast's record, 16 bytes: the time, the ORIGINAL triangle index and the separating axis that gave the time. */
typedef struct lbvh_box_hit { float t; uint32_t tri; uint32_t axis; uint32_t _zero; } lbvh_box_hit;

#define LBVH_BOX_AXIS_START 13u   /* lbvh_box_hit.axis of a box that overlaps the triangle at the start (t = +0) */

/* First contact of `count` moving boxes with the mesh (a "box cast": crates, hulls, doors, placement previews), over the derived
 * traversal scene in its four-wide form by the walk of lbvh_sphere_cast.  The half-axis VECTORS make the box: three orthogonal
 * ones an oriented box, three axis-aligned ones an AABB, any three independent ones a sheared box (a parallelepiped) — nothing
 * below assumes orthogonality and nothing is normalised.  The box moves without turning: c(t) = centre + dir * t for 0 <= t < T,
 * T = min(t_max, LBVH_MAX_FLOAT); dir need not be unit length and t is in units of dir.
 *   Active cast: the conditions of lbvh_sphere_cast on t_max, centre (for its origin) and dir; every component of ax, ay, az
 *   finite; and the fp32 value det = dot(ax, cross(ay, az)) finite and != 0 (the box is solid; flat boxes are out of scope).  An
 *   inactive cast is never walked; it gets the miss record {LBVH_MAX_FLOAT, 0, 0, 0} (lbvh_box_cast) or 0 (lbvh_box_cast_any).
 *   Time of contact with one triangle: a swept separating-axis test on a, e1, e2 of the triangle's line of the derived scene, in
 *   strict fp32, every operation rounded on its own, dot and cross as at lbvh_sphere_cast, / correctly rounded, min and max as
 *   fminf and fmaxf (of a NaN and a number: the number), |x| exact.  With b_0, b_1, b_2 = ax, ay, az and E_0, E_1, E_2 = e1, e2,
 *   e2 - e1 (per component), the thirteen axes L_j in this order:
 *     j = 0            cross(e1, e2)                                      the triangle's face
 *     j = 1, 2, 3      cross(ay, az), cross(az, ax), cross(ax, ay)        the box's faces
 *     j = 4 + 3*i + k  cross(b_i, E_k), i = 0 .. 2, k = 0 .. 2            a box edge against a triangle edge
 *   Per axis, with L = L_j:
 *     m = a - centre (per component)   p0 = dot(m, L)   p1 = p0 + dot(e1, L)   p2 = p0 + dot(e2, L)
 *     lo = min(p0, min(p1, p2))   hi = max(p0, max(p1, p2))           the triangle's interval, from the box's centre
 *     rb = (|dot(ax, L)| + |dot(ay, L)|) + |dot(az, L)|                the box's half width
 *     v = dot(dir, L)
 *     if v > 0:      tin = (lo - rb) / v   tout = (hi + rb) / v
 *     else if v < 0: tin = (hi + rb) / v   tout = (lo - rb) / v
 *     else (v is 0 or a NaN): the axis gives no constraint if lo <= rb && -rb <= hi, and the triangle has NO TIME if not.
 *   Start with enter = +0, exit = +inf, axis = 13 (LBVH_BOX_AXIS_START).  In the order j = 0 .. 12: tin replaces enter, and j
 *   replaces axis, only when tin > enter; tout replaces exit only when tout < exit.  The triangle has the time enter iff
 *   enter <= exit after all thirteen.  Two consequences:
 *     a zero axis (parallel edges) has rb = lo = hi = v = 0 and constrains nothing;
 *     a near-zero axis is taken as the direction it is: the projections are accurate relative to the computed L, and two convex
 *     sets that overlap do so along every direction, so it cannot separate them beyond ordinary roundoff.
 *   NaN (only from infinities: an infinite centre, or products that overflow): a comparison with a NaN is false, so a NaN tin or
 *   tout replaces nothing, a NaN v takes the third branch, and there a NaN lo, hi or rb means no time.  enter and exit are
 *   never NaN, a time is never NaN, and enter is never -0: t = +0 exactly for a start in overlap.
 *   The thirteen axes suffice for a parallelepiped: it and the triangle are convex polytopes, and two convex polytopes are
 *   disjoint iff a face normal of one or the cross product of an edge of each separates them; a parallelepiped has three face
 *   normals and three edge directions whether or not they are orthogonal.  Moving the box by dir*t shifts its interval on every
 *   axis by v*t, which gives the interval of t in which that axis does not separate; the box touches the triangle from the
 *   largest entry on, while that is before the smallest exit.
 *   Candidate: with g_k = (|ax_k| + |ay_k|) + |az_k| per world axis k (the half extent of the box's own AABB), triangle i is a
 *   candidate iff it has a time t_i, t_i < T, the ray (centre, dir) passes the slab test of the triangle's own box grown by g —
 *   scene.triangle_aabb[i] with min_k - g_k and max_k + g_k, one fp32 operation per bound, the slab test of every walker of this
 *   library — with entry distance e_i, and !(t_i < e_i).
 *   lbvh_box_cast: d_hits[k] = {t, tri, axis, 0} of cast k's candidate with the least t (compared as fp32 values); on equal t the
 *   lower original triangle index, whatever order the walk meets them in.  axis = the j that gave the time (13: overlapping at
 *   the start).  The contact normal, pointing from the triangle to the box, is -sign(v_j) * L_j / |L_j| for axis = j < 13 (for
 *   13: none).  A contact POINT is not part of the record and is out of scope: a box touches a triangle in a point, a segment or
 *   a polygon.  No candidate: the miss record, never T.
 *   lbvh_box_cast_any: d_flags[k] = 1 if cast k has any candidate, else 0.  The walk is the same (same near-first order) cut
 *   off at its first accepted candidate: never more node fetches or triangle tests per cast.
 * Why the record does not depend on the order of the walk (the argument of lbvh_sphere_cast): lo - g and hi + g are each one
 * operation monotone in lo and hi, and every box of the derived tree is the exact min / max union of what is below it, so the
 * grown box of an ancestor contains the grown box of everything below it exactly in fp32; slab entries grow from a box to any box
 * inside it, so e(ancestor) <= e(leaf) <= t for every candidate.  A slot is skipped only if the ray misses its grown box or its
 * entry is > best, strictly: a subtree skipped that way holds no candidate at or below best.  Nothing is pruned on a box's exit
 * distance.  A time in front of its own grown box is fp32 noise (a box touching the triangle has its centre within g of the
 * triangle's box on every world axis); on ordinary meshes the rule rejects next to nothing.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_casts or d_hits not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_stack_split,
 * lbvh_debug_ray_stack_limit, lbvh_ray_stats_target and lbvh_debug_ray_waves apply as to the sphere cast.  The cost grows with the
 * box (every tree box is larger by g) and each tested triangle costs up to thirteen axes. */
lbvh_status lbvh_box_cast(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                          lbvh_box_hit* d_hits);
lbvh_status lbvh_box_cast_any(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                              uint32_t* d_flags);

/* EVERY contact along `count` sweeps as a CSR list — the "all" form of the three casts (first contact: lbvh_sphere_cast /
 * lbvh_capsule_cast / lbvh_box_cast, any: their _any forms), what lbvh_gather_hits is to lbvh_trace_closest —, over the same scene
 * by the four-wide walk of the casts, in the count -> device-side scan -> fill shape of lbvh_gather_hits.  Nothing below is new
 * arithmetic: every term is the one defined at the shape's cast.
 *   Active cast, T = min(t_max, LBVH_MAX_FLOAT), the time of contact with one triangle, the triangle's own grown box, its entry
 *   distance e_i and the candidate rule are exactly those of lbvh_sphere_cast / lbvh_capsule_cast / lbvh_box_cast: triangle i is a
 *   candidate iff it has a time t_i, t_i < T, the ray of the cast passes the slab test of the triangle's own grown box, and
 *   !(t_i < e_i).  A NaN never counts; an inactive cast has an empty segment and is never walked.
 * Output: lbvh_gather_hits' contract, verbatim.
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[q] = the number of candidates of casts 0 .. q-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_hits, `capacity` records of 16 bytes: segment q = d_hits[d_offsets[q] .. d_offsets[q+1]) = one record per candidate of cast
 *   q, each exactly once; the four words are the ones the first-contact call would write if that candidate were the nearest:
 *     lbvh_sphere_cast_all    {t, tri, u, v}, (u, v) lbvh_closest_point_query's for the point c(t) and this triangle;
 *     lbvh_capsule_cast_all   {t, tri, u, v}, (u, v) through the axis parameter s of the derived triangle that gave the time, or of
 *                             the pierce, as lbvh_capsule_cast defines them;
 *     lbvh_box_cast_all       {t, tri, axis, 0} (lbvh_box_hit).
 *   THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT.  Every record carries its t: sort a segment by
 *   (t, tri) if an order is needed — two candidates of a cast never share a triangle index, so that order is canonical.
 *   lbvh_sort_hit_segments applies unchanged and puts every segment into that order on the device, in place: lbvh_box_hit has t and
 *   tri in words 0 and 1 like lbvh_hit, and words 2 and 3 (axis, 0) travel with their record as u and v do — pass the box records
 *   to it as lbvh_hit*.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[q+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn whether everything fitted.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_hits may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill).  d_hits == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Hence, for every cast q with m = d_offsets[q+1] - d_offsets[q]: m >= 1 exactly when the shape's _cast_any gives 1; the least
 * element of segment q by (t, tri), t compared as fp32 values, is the first-contact call's record word for word (the miss record
 * when m == 0); and every triangle that lbvh_capsule_overlaps / lbvh_obb_overlaps lists for the shape where it stands at t = 0
 * (capsule {origin, radius, axis}, box {centre, ax, ay, az}) is in the segment with t = +0 (tests/test_cast_all.py asserts the
 * inclusion on its sets; DESIGN.md records whether equality held there).
 * Why the list does not depend on the walk: the grown-box containment argument of each cast with the fixed bound T in place of
 * best.  The grown box of an ancestor contains the grown box of everything below it exactly in fp32, slab entries grow from a box
 * to any box inside it, so every ancestor of a candidate's leaf passes its slab test with entry <= e <= t < T; the walk skips
 * only boxes that the ray misses or whose entry is > T.  The bound is T from the first step to the last — nothing shrinks, the
 * box cast's early out over its axes included, which is fed T —, and nothing is pruned on a box's exit distance.  Each triangle
 * is exactly one leaf, so each candidate is met exactly once.  The count walk and the fill walk are the same kernel making the
 * same decisions on t and the entry alone, so a segment never outgrows its slot.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the
 * context's stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path list (see
 * lbvh_path_bounce); a failed growth of that scratch is LBVH_ERR_OUT_OF_MEMORY with nothing written.  count == 0 is a no-op:
 * nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected, the message naming the entry point: NULL ctx /
 * d_casts / h_scene / d_offsets, d_casts or d_hits not 16-byte aligned, d_offsets not 8-byte aligned, count > 2^32 - 1.  Four-wide
 * walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit
 * and lbvh_ray_stats_target apply as to lbvh_gather_hits (the stats of both walks are added: the full form reports twice the
 * count-only form's).
 * One cast per lane.  The cost grows with the swept volume: every grown box the motion crosses before T is opened, where the
 * first-contact call stops opening boxes behind its best — give a move its real length as t_max, not +inf. */
lbvh_status lbvh_sphere_cast_all(lbvh_context* ctx, const lbvh_sphere_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                 uint64_t* d_offsets, lbvh_hit* d_hits, uint64_t capacity);
lbvh_status lbvh_capsule_cast_all(lbvh_context* ctx, const lbvh_capsule_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, lbvh_hit* d_hits, uint64_t capacity);
lbvh_status lbvh_box_cast_all(lbvh_context* ctx, const lbvh_box_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, lbvh_box_hit* d_hits, uint64_t capacity);

/* A query triangle: 48 bytes; arrays of them 16-byte aligned. */
typedef struct lbvh_tri_query {
    float a[3]; uint32_t skip;     /* ORIGINAL index of a scene triangle that is never a candidate; LBVH_NULL = none */
    float b[3]; uint32_t _pad0;    /* not read */
    float c[3]; uint32_t _pad1;    /* not read */
} lbvh_tri_query;

/* Triangle queries: WHICH scene triangles does a triangle intersect — the narrow phase behind lbvh_box_overlaps —, as a CSR list
 * (lbvh_triangle_intersections) or as one flag per query (lbvh_triangle_intersects_any), over the derived traversal scene in its
 * four-wide form by the walk of lbvh_box_overlaps.
 *   Active query: all nine coordinates of a, b and c are finite.  An inactive query is never walked; it gets an empty segment, or
 *   the flag 0.
 *   Query box: Q.min[k] = fminf(fminf(a[k], b[k]), c[k]), Q.max[k] = fmaxf(fmaxf(a[k], b[k]), c[k]): exact, not padded.
 *   Edge test: pierce(P, D; V, E1, E2) is the Moeller-Trumbore test of every ray walker of this library (lbvh_trace_closest), for the
 *   ray origin P, direction D (not normalised) against the triangle with first vertex V and edge vectors E1, E2, in strict fp32,
 *   every operation rounded on its own, dot(x, y) = (x0*y0 + x1*y1) + x2*y2, cross(x, y) per component x1*y2 - x2*y1:
 *       p = cross(D, E2)      det = dot(E1, p)      if (det < 1e-8 && det > -1e-8) miss
 *       inv = 1 / det         s = P - V             u = dot(s, p) * inv           if (u < 0 || u > 1) miss
 *       q = cross(s, E1)      v = dot(D, q) * inv                                 if (v < 0 || u + v > 1) miss
 *       t = dot(E2, q) * inv
 *   A miss has t = LBVH_MAX_FLOAT.  The test PASSES iff 0 <= t && t <= 1 (false for a miss and for a NaN t).
 *   Candidate: scene triangle i — first vertex v0 and edge vectors e1 = v1 - v0, e2 = v2 - v0 as its line of the derived scene
 *   holds them (the fp32 differences taken at build time) — is a candidate of an active query iff
 *     (1) its ORIGINAL index is not `skip`, and
 *     (2) its own box A = scene.triangle_aabb[i] overlaps Q in closed intervals, Q.min[k] <= A.max[k] && A.min[k] <= Q.max[k] for
 *         k = 0, 1, 2 (the six comparisons of lbvh_box_overlaps), and
 *     (3) at least one of these six edge tests passes, every P and D formed per component in fp32:
 *         the query's edges against the scene triangle:     pierce(a, b - a; v0, e1, e2)   pierce(b, c - b; v0, e1, e2)
 *                                                           pierce(c, a - c; v0, e1, e2)
 *         the scene triangle's edges against the query:     pierce(v0, e1; a, b - a, c - a)   pierce(v0, e2; a, b - a, c - a)
 *                                                           pierce(v0 + e1, e2 - e1; a, b - a, c - a)
 *         (the edge list of lbvh_sphere_cast).
 *   What follows from this definition:
 *     Coplanar overlapping triangles are generally NOT reported: an edge parallel to the other triangle's plane has det ~ 0 and is
 *     rejected by the det test.  Exact coplanar overlap is out of scope.
 *     Triangles that only touch (a shared vertex or edge) are reported exactly when the arithmetic above says so — u, v or t at a
 *     bound after rounding —, not by a rule of their own.  `skip` removes the query's own triangle when a mesh is tested against
 *     itself (skip = the triangle's original index); removing neighbours that share a vertex is the caller's job on the returned pairs.
 *     A pierce computed for a pair whose boxes do not overlap is fp32 noise and is not a candidate (rule (2)): the analogue of the
 *     accept rule of the ray walkers.
 *   Why the list does not depend on the walk (the argument at lbvh_box_overlaps): every box of the derived tree, binary or
 *   four-wide, is the exact min / max union of what lies below it, so every ancestor of a candidate's leaf passes the same six
 *   comparisons; the walk skips exactly the slots that fail.  (1) and (3) are functions of (query, triangle) only.  Each triangle is
 *   one leaf, so each candidate appears once.
 * Output of lbvh_triangle_intersections — the CSR contract of lbvh_box_overlaps, word for word:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[k] = the number of candidates of queries 0 .. k-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_tris, `capacity` words of 32 bits: segment k = d_tris[d_offsets[k] .. d_offsets[k+1]) = the ORIGINAL triangle indices of
 *   query k's candidates, each exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT;
 *   lbvh_sort_index_segments applies unchanged and leaves every fitting segment strictly ascending.
 *   Overflow: no word at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; words
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_tris may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill: the same kernel making the same decisions, so a segment never outgrows its slot).
 *   d_tris == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Output of lbvh_triangle_intersects_any: d_flags[k] = 1 exactly when segment k would be non-empty, else 0; every one of the `count`
 * words is written.  The walk is the same, cut off at a query's first candidate.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL
 * ctx / d_queries / h_scene / d_offsets / d_flags, d_queries not 16-byte aligned, d_offsets not 8-byte aligned, d_tris or d_flags
 * not 4-byte aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves,
 * lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the overlap queries (triangle_tests
 * counts the triangles that reached the edge tests; the full form reports twice the count-only form's).
 * One query per lane; the cost is that of lbvh_box_overlaps on the queries' boxes plus one 64-byte triangle line and up to six
 * edge tests per box-overlapping triangle: a query much larger than the scene's triangles keeps its lane busy for long. */
lbvh_status lbvh_triangle_intersections(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                        uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);
lbvh_status lbvh_triangle_intersects_any(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                         uint32_t* d_flags);

/* A moving triangle: 64 bytes, arrays 16-byte aligned. */
typedef struct lbvh_tri_ray {
    float a[3];   uint32_t skip;     /* ORIGINAL index of a scene triangle that is never reported; LBVH_NULL = none */
    float b[3];   float    t_max;
    float c[3];   uint32_t _pad0;    /* not read */
    float dir[3]; uint32_t _pad1;    /* not read */
} lbvh_tri_ray;

/* lbvh_triangle_cast's record, 16 bytes (the shape of lbvh_hit): the time, the ORIGINAL triangle index, the feature pair that
 * gave the time and, for an edge against an edge, the position on the scene triangle's edge. */
typedef struct lbvh_tri_cast_hit { float t; uint32_t tri; uint32_t feature; float w; } lbvh_tri_cast_hit;

#define LBVH_TRI_CAST_START 16u   /* lbvh_tri_cast_hit.feature & 16: the triangles intersect at the start (t = +0) */

/* First contact of `count` moving triangles with the mesh (a "triangle cast": how far a second mesh, a piece of debris or cloth
 * may move along a direction before it touches the scene; the sweep test of a mesh collider), over the derived traversal scene in
 * its four-wide form by the walk of lbvh_sphere_cast.  The query triangle moves without turning: its vertices are a + dir*t,
 * b + dir*t, c + dir*t for 0 <= t < T, T = min(t_max, LBVH_MAX_FLOAT); dir need not be unit length and t is in units of dir.
 *   Active cast: the nine coordinates of a, b and c are finite, every component of dir is finite, dot(dir, dir) > 0 and t_max > 0
 *   (all false for a NaN).  An inactive cast is never walked; it gets the miss record {LBVH_MAX_FLOAT, 0, 0, +0}
 *   (lbvh_triangle_cast) or 0 (lbvh_triangle_cast_any).
 *   Two tests, in strict fp32, every operation rounded on its own, dot and cross as at lbvh_triangle_intersections:
 *     pierce(P, D; V, E1, E2) is the edge test of lbvh_triangle_intersections, unchanged, with its u, v and t.
 *     pierce_quad(P, D; V, E1, E2) is the same arithmetic with the rejections u < 0 || u > 1 and v < 0 || v > 1 in place of
 *     u < 0 || u > 1 and v < 0 || u + v > 1: the ray against the parallelogram V + E1*u + E2*v, not the triangle.  The rejection
 *     det < 1e-8 && det > -1e-8 stays.  A rejected test has t = LBVH_MAX_FLOAT in both.
 *   Time with one scene triangle, v0, e1, e2 as its line of the derived scene holds them, every vector below formed per component
 *   in fp32 (a negation is exact):
 *     Start overlap.  If rules (2) and (3) of lbvh_triangle_intersections hold for the query {a, b, c} — the triangle's own box
 *     overlaps the query's exact box, and one of the six edge tests passes with 0 <= t <= 1 — the time is +0, feature = 16 | j
 *     with j = 0 .. 5 the first passing test in that call's order, and w = +0.
 *     Otherwise the time is the least t with 0 <= t && t < LBVH_MAX_FLOAT among fifteen features, taken in this order, a later
 *     one replacing an earlier one only when strictly less, compared as fp32 values; a NaN never counts; w = +0 except where
 *     stated.  With E_ab = b - a, E_bc = c - b, E_ca = a - c:
 *       feature 0, 1, 2        a moving vertex onto the scene face: pierce(X, dir; v0, e1, e2) for X = a, b, c
 *       feature 3, 4, 5        a scene vertex onto the moving face: pierce(Y, -dir; a, b - a, c - a) for Y = v0, v0 + e1, v0 + e2
 *       feature 6 + 3*m + n    moving edge m against scene edge n: pierce_quad(P, dir; Q, F, -E) with (P, E) = (a, E_ab), (b, E_bc),
 *                              (c, E_ca) for m = 0, 1, 2 and (Q, F) = (v0, e1), (v0, e2), (v0 + e1, e2 - e1) for n = 0, 1, 2 (the
 *                              edge list of lbvh_sphere_cast).  P + E*s + dir*t = Q + F*u is the ray from P meeting the
 *                              parallelogram Q + F*u - E*s: the test's u is the position on the scene edge and is the record's w,
 *                              its v the position s on the moving edge.
 *     No feature with such a t: the triangle has no time.
 *   What the definition gives and what it leaves out: two triangles that translate relative to each other and start apart first
 *   touch with a vertex of one on the face of the other or with an edge of one on an edge of the other, and every passing feature
 *   is a real common point of the two triangles at its t; so in exact arithmetic the least of the fifteen is the time of first
 *   contact.  Parallel edges and a coplanar approach (an edge sliding into an edge of the same line, a face onto a face) have
 *   det ~ 0 and fall to the det rejection, as coplanar overlap does at lbvh_triangle_intersections: they are reported only through
 *   the other features that touch at the same time, if any does.  The time may be -0 only where the arithmetic gives a feature
 *   t = -0; a start overlap is +0 exactly.
 *   Candidate: triangle i is a candidate iff its ORIGINAL index is not `skip`, it has a time t_i, t_i < T, the ray (a, dir) passes
 *   the slab test of the triangle's own box grown by the query's extent relative to a — scene.triangle_aabb[i] with, per axis k
 *   and h1 = b - a, h2 = c - a,
 *       min' = min_k - fmaxf(fmaxf(h1_k, h2_k), 0)      max' = max_k - fminf(fminf(h1_k, h2_k), 0),
 *   one fp32 operation per bound, the slab test of every walker of this library — with entry distance e_i, and !(t_i < e_i).  (a
 *   is in the grown box exactly when some point of the query's box is in the own box, per axis.)
 *   lbvh_triangle_cast: d_hits[k] = {t, tri, feature, w} of cast k's candidate with the least t (compared as fp32 values); on
 *   equal t the lower original triangle index, whatever order the walk meets them in.  The contact point and normal follow from
 *   the feature: 0 - 2 the moved vertex X + dir*t and the scene face's normal cross(e1, e2); 3 - 5 the scene vertex Y and the
 *   moving face's normal cross(b - a, c - a); 6 - 14 the point Q + F*w and cross(E, F); each normal turned against dir.  No
 *   candidate: the miss record, never T.
 *   lbvh_triangle_cast_any: d_flags[k] = 1 if cast k has any candidate, else 0.  The walk is the same (same near-first order) cut
 *   off at its first accepted candidate: never more node fetches or triangle tests per cast.
 * Why the record does not depend on the order of the walk (the argument of lbvh_capsule_cast): lo - max(h1, h2, 0) and
 * hi - min(h1, h2, 0) are each one operation monotone in lo and hi, and every box of the derived tree is the exact min / max union
 * of what is below it, so the grown box of an ancestor contains the grown box of everything below it exactly in fp32; slab entries
 * grow from a box to any box inside it, so e(ancestor) <= e(leaf) <= t for every candidate.  A slot is skipped only if the ray
 * misses its grown box or its entry is > best, strictly: a subtree skipped that way holds no candidate at or below best.  Nothing
 * is pruned on a box's exit distance.  `skip`, the start rule and the fifteen features are functions of (cast, triangle) only.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_casts or d_hits not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_stack_split,
 * lbvh_debug_ray_stack_limit, lbvh_ray_stats_target and lbvh_debug_ray_waves apply as to the sphere cast (triangle_tests counts the
 * triangle lines that reached the narrow phase: `skip` is not counted).  The cost grows with the query (every tree box is larger
 * by its extent) and each tested triangle costs fifteen Moeller-Trumbore tests, twenty-one where the boxes overlap.  A whole mesh
 * is one cast per triangle with the same dir, the least record taken by the caller.  Every contact along the way
 * (lbvh_triangle_cast_all) is out of scope; the record has the shape of lbvh_hit so that lbvh_sort_hit_segments would apply. */
lbvh_status lbvh_triangle_cast(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                               lbvh_tri_cast_hit* d_hits);
lbvh_status lbvh_triangle_cast_any(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                   uint32_t* d_flags);

/* Every triangle a moving triangle touches, as a CSR list — the "all" form of lbvh_triangle_cast / lbvh_triangle_cast_any, what
 * lbvh_sphere_cast_all is to lbvh_sphere_cast (a sweep-test-all of a mesh collider: filter triggers or the body's own triangles by
 * index, debris that cuts through several sheets, every pair of a cloth step that comes into contact during the step).  The call
 * that the block above names as out of scope now exists; this is it.  Over the same scene by the four-wide walk of the cast, in
 * the count -> device-side scan -> fill shape of lbvh_gather_hits.  Nothing below is new arithmetic: every term is the one
 * defined at lbvh_triangle_cast.
 *   Active cast, T = min(t_max, LBVH_MAX_FLOAT), `skip`, the time with one scene triangle (the start overlap by rules (2) and (3)
 *   of lbvh_triangle_intersections, else the least of the fifteen features), the triangle's own grown box, its entry distance e_i
 *   and the candidate rule are exactly lbvh_triangle_cast's: triangle i is a candidate iff its ORIGINAL index is not `skip`, it
 *   has a time t_i, t_i < T, the ray (a, dir) passes the slab test of the triangle's own grown box, and !(t_i < e_i).  A NaN never
 *   counts; an inactive cast has an empty segment and is never walked.
 * Output: lbvh_gather_hits' contract, verbatim as at lbvh_sphere_cast_all.
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[q] = the number of candidates of casts 0 .. q-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_hits, `capacity` records of 16 bytes: segment q = d_hits[d_offsets[q] .. d_offsets[q+1]) = one record per candidate of cast
 *   q, each exactly once: the {t, tri, feature, w} that lbvh_triangle_cast would write were that candidate the nearest.
 *   THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT.  Sort a segment by (t, tri) if an order is needed —
 *   two candidates of a cast never share a triangle index, so that order is canonical.  lbvh_sort_hit_segments applies unchanged
 *   and puts every segment into that order on the device, in place: t and tri are words 0 and 1 as in lbvh_hit, and feature and w
 *   travel with their record as u and v do — pass the records to it as lbvh_hit*.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[q+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn whether everything fitted.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_hits may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill).  d_hits == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Hence, for every cast q with m = d_offsets[q+1] - d_offsets[q] records:
 *   m >= 1 exactly when lbvh_triangle_cast_any gives 1;
 *   the least record of segment q by (t as an fp32 value, tri) is lbvh_triangle_cast's record word for word, and when m == 0
 *   that call writes the miss record {LBVH_MAX_FLOAT, 0, 0, +0};
 *   a triangle that lbvh_triangle_intersections lists for {a, b, c, skip} is in the segment with t == +0 and
 *   feature & LBVH_TRI_CAST_START wherever the grown-box rule admits it.  That last relation can fail in the definition itself:
 *   the intersection call has no grown box and no !(t_i < e_i) — a start overlap has t = +0, and where fp32 puts the entry of the
 *   triangle's own grown box above 0, or makes the ray miss that box, the pair is no candidate of either cast form
 *   (tests/test_triangle_cast.py documents this for the first-contact call; DESIGN.md records the count on the test sets).
 * Why the list does not depend on the walk: the grown-box containment argument of lbvh_triangle_cast with the fixed bound T in
 * place of best.  lo - max(h1, h2, 0) and hi - min(h1, h2, 0) are monotone, so the grown box of an ancestor contains the grown box
 * of everything below it exactly in fp32, slab entries grow from a box to any box inside it, and every ancestor of a candidate's
 * leaf passes its slab test with entry <= e <= t < T; the walk skips only boxes that the ray misses or whose entry is > T.  The
 * bound is T from the first step to the last: nothing shrinks and nothing is pruned on a box's exit distance.  Each triangle is
 * exactly one leaf, so each candidate is met exactly once.  The count walk and the fill walk are the same kernel making the same
 * decisions, so a segment never outgrows its slot.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the
 * context's stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path list (see
 * lbvh_path_bounce); a failed growth of that scratch is LBVH_ERR_OUT_OF_MEMORY with nothing written.  count == 0 is a no-op:
 * nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected, the message naming lbvh_triangle_cast_all: NULL
 * ctx / d_casts / h_scene / d_offsets, d_casts or d_hits not 16-byte aligned, d_offsets not 8-byte aligned, count > 2^32 - 1.
 * Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves, lbvh_debug_ray_stack_split,
 * lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to lbvh_sphere_cast_all (the stats of both walks are added: the
 * full form reports twice the count-only form's; triangle_tests counts the triangle lines that reached the narrow phase: `skip`
 * is not counted).
 * One cast per lane.  The cost grows with the swept volume — every grown box the motion crosses before T is opened — and every
 * tested triangle costs fifteen Moeller-Trumbore tests, twenty-one where the boxes overlap, in each of the two walks: give a move
 * its real length as t_max, not +inf. */
lbvh_status lbvh_triangle_cast_all(lbvh_context* ctx, const lbvh_tri_ray* d_casts, size_t count, const lbvh_scene* h_scene,
                                   uint64_t* d_offsets, lbvh_tri_cast_hit* d_hits, uint64_t capacity);

/* Where a query triangle cuts one scene triangle: 32 bytes, arrays 16-byte aligned; written as two 16-byte stores. */
typedef struct lbvh_tri_segment {
    float p0[3]; uint32_t tri;     /* one end of the segment; ORIGINAL index of the scene triangle */
    float p1[3]; uint32_t edges;   /* the other end; which edge tests passed, and which gave p0 / p1 (below) */
} lbvh_tri_segment;

/* Triangle intersection segments: WHERE does a triangle cut each scene triangle it intersects (the contact polyline between two
 * meshes, the cut curve of a CSG or slicing step, a cross-section, self-intersection repair), as a CSR list of records over the
 * derived traversal scene in its four-wide form by the walk of lbvh_triangle_intersections.  The active rule, the query box, `skip`,
 * rules (1) to (3) and therefore the candidate set are lbvh_triangle_intersections' exactly, from the same operations on the same
 * values: "is a candidate" there and "has a record" here never disagree, and a caller need not redo the edge arithmetic on the host
 * (whose roundings would differ from the library's exactly at the bounds).
 *   The record of a candidate pair, in strict fp32, every operation rounded on its own, dot and pierce as defined above:
 *     All six edge tests of rule (3) are evaluated, in the order they are listed there, j = 0 .. 5 (j = 0, 1, 2 the query's edges
 *     from a, b, c; j = 3, 4, 5 the scene triangle's edges (v0, e1), (v0, e2), (v0 + e1, e2 - e1)).  No test ends the sequence.
 *     For every j that PASSES (0 <= t_j <= 1):   X_j = P_j + D_j * t_j   per component, one multiplication and one addition, with
 *     the P_j, D_j and t_j the test itself used.
 *     A running pair (p0, p1) is kept over the passing j in ascending order:
 *       the first passing j:    p0 = p1 = X_j;
 *       the second passing j:   p1 = X_j;
 *       every later passing j:  d01 = dot(p0 - p1, p0 - p1), d0 = dot(p0 - X_j, p0 - X_j), d1 = dot(p1 - X_j, p1 - X_j), the
 *                               differences per component in fp32;
 *                               if (d0 > d01 && d0 >= d1) p1 = X_j;   else if (d1 > d01) p0 = X_j;   else nothing changes.
 *     The passing points lie on the line in which the two triangles' planes meet, so in exact arithmetic this update keeps the two
 *     extreme points: the segment the triangles share.  In generic position exactly two tests pass and (p0, p1) are those two
 *     points in the order of j.  A pair with one passing test (a touch at a bound) has p0 == p1, bit for bit.
 *     edges: bit j (0 .. 5) is set iff test j passed; bits 8 .. 10 hold the j that gave p0, bits 12 .. 14 the j that gave p1; every
 *     other bit is zero.  A caller stitching a cut polyline can match the ends of neighbouring records by (triangle, edge) — an end
 *     from j = 0, 1, 2 lies on that edge of the QUERY triangle, one from j = 3, 4, 5 on that edge of scene triangle `tri` — and
 *     need not compare floats.
 *   The record is a function of (query, triangle) only, so the list does not depend on the walk by the argument at
 *   lbvh_triangle_intersections, unchanged.  Coplanar overlap is not reported there and has no segment here.
 * Output — lbvh_triangle_intersections' CSR contract with a record in place of an index:
 *   d_offsets: count + 1 words of 64 bits, the SAME words lbvh_triangle_intersections writes for these queries.  Always written in
 *   full, whatever `capacity` is.
 *   d_segments, `capacity` records of 32 bytes: segment k = d_segments[d_offsets[k] .. d_offsets[k+1]) = one record per candidate of
 *   query k, each triangle exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT (sort by `tri` on
 *   the host if an order is needed: lbvh_sort_index_segments and lbvh_sort_hit_segments are for 4- and 16-byte records).
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_segments may be NULL) — it IS
 *   lbvh_triangle_intersections' count-only form; otherwise the scene is walked twice (that count walk, the device-side scan, a fill
 *   walk that takes the candidate decision from the same six t and forms the records, so a segment never outgrows its slot).
 *   d_segments == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the context's
 * stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path list (see lbvh_path_bounce).
 * count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL ctx / d_queries /
 * h_scene / d_offsets, d_queries or d_segments not 16-byte aligned, d_offsets not 8-byte aligned, count > 2^32 - 1.  Four-wide walk
 * only; lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to
 * lbvh_triangle_intersections (triangle_tests of the full form is twice the count-only form's).
 * Cost: the fill walk visits what lbvh_triangle_intersections' visits, but evaluates all six tests for every box-overlapping
 * triangle where that call stops at the first that passes, and a record is 32 bytes.
 * Out of scope: a device-side sort of 32-byte record segments; exact coplanar overlap; merging records into polylines; a contact
 * normal or depth for triangle pairs; an _any form (it is lbvh_triangle_intersects_any) or a form for one huge query.  (Out of
 * scope of THIS call: the device-side sort of 32-byte record segments by `tri` is lbvh_sort_record_segments with
 * LBVH_SORT_RECORDS_BY_TRI, above.) */
lbvh_status lbvh_triangle_intersection_segments(lbvh_context* ctx, const lbvh_tri_query* d_queries, size_t count,
                                                const lbvh_scene* h_scene, uint64_t* d_offsets,
                                                lbvh_tri_segment* d_segments, uint64_t capacity);

/* A capsule where it stands: 32 bytes, arrays 16-byte aligned: every point within `radius` of the segment [origin, origin + axis]
 * (lbvh_capsule_ray without the motion).  _pad is not read. */
typedef struct lbvh_capsule { float origin[3]; float radius; float axis[3]; uint32_t _pad; } lbvh_capsule;
/* An oriented box where it stands: 64 bytes, arrays 16-byte aligned: { centre + s0*ax + s1*ay + s2*az : |s_i| <= 1 }, the three
 * half-axis VECTORS of lbvh_box_ray — a parallelepiped, nothing normalised, nothing assumed orthogonal.  The pads are not read. */
typedef struct lbvh_obb { float centre[3]; uint32_t _pad0; float ax[3]; uint32_t _pad1;
                          float ay[3]; uint32_t _pad2; float az[3]; uint32_t _pad3; } lbvh_obb;

/* Shape overlaps: WHICH triangles does a capsule or an oriented box touch where it stands (what a character controller asks
 * right after a sweep: move, list what the shape now touches, push out; Physics.OverlapCapsule / OverlapBox, and CheckCapsule /
 * CheckBox without an invented direction), as a CSR list (lbvh_capsule_overlaps, lbvh_obb_overlaps) or as one flag per shape
 * (lbvh_capsule_overlaps_any, lbvh_obb_overlaps_any), over the derived traversal scene in its four-wide form by the walk of
 * lbvh_triangle_intersections.  The definition is the start overlap of lbvh_capsule_cast / lbvh_box_cast with the motion taken
 * out, in strict fp32, every operation rounded on its own, with the operations, the order and the names of those definitions.
 * Triangle i, with the line a, e1, e2 of the derived scene and its own box A = scene.triangle_aabb[i], is a candidate of an
 * ACTIVE shape iff rule 1 and rule 2 below both hold.  An inactive shape is never walked; it gets an empty segment, or the flag 0.
 *   Capsule (o = origin, h = axis, r = radius):
 *     Active: radius > 0 and radius < +inf, no NaN in origin, every component of axis finite (lbvh_capsule_cast's conditions on
 *     radius, origin and axis; all false for NaN).  axis = 0 is allowed.
 *     Rule 1, own box: for each world axis k
 *         (A.min[k] - max(h_k, 0)) - r <= o_k && o_k <= (A.max[k] - min(h_k, 0)) + r
 *     lbvh_capsule_cast's grown bounds, two fp32 operations each, max and min as fmaxf and fminf, in closed comparisons.
 *     Rule 2, touch: for some derived triangle j = 0 .. 7 of lbvh_capsule_cast (a_j, e1_j, e2_j formed as there, j = 0 the line as
 *     stored), dist2 of lbvh_closest_point_query for the point o against it is <= R2, R2 = r*r (one operation); OR
 *     pierce(o, h; a, e1, e2) of lbvh_triangle_intersections passes, 0 <= t <= 1 (the axis goes through the face with both ends
 *     and all edges farther than the radius).
 *   Box (c = centre, b_0, b_1, b_2 = ax, ay, az):
 *     Active: no NaN in centre, every component of ax, ay, az finite, and the fp32 value det = dot(ax, cross(ay, az)) finite and
 *     != 0 (lbvh_box_cast's conditions on centre, ax, ay, az and det; flat boxes are out of scope).
 *     Rule 1, own box: with g_k = (|ax_k| + |ay_k|) + |az_k| as in lbvh_box_cast, for each world axis k
 *         A.min[k] - g_k <= c_k && c_k <= A.max[k] + g_k                 one fp32 operation per bound, closed comparisons.
 *     Rule 2, touch: for EVERY one of the thirteen axes L_j of lbvh_box_cast, in its order, with m = a - c, p0, p1, p2, lo, hi and
 *     rb exactly as there:   lo <= rb && -rb <= hi.   That definition's v = 0 branch on all thirteen axes: no axis separates.
 *   A NaN never counts: a comparison with a NaN is false, so a NaN dist2 or t passes nothing and a NaN lo, hi or rb means not a
 *   candidate.  A zero axis L_j (parallel edges) has lo = hi = rb = 0 and passes.
 *   Why the list does not depend on the walk (the argument at lbvh_triangle_intersections with grown boxes): the grown bounds are
 *   monotone in lo and hi — (lo - max(h, 0)) - r, (hi - min(h, 0)) + r, lo - g, hi + g, every operation monotone —, and every box
 *   of the derived tree, binary or four-wide, is the exact min / max union of what lies below it; so every ancestor of a
 *   candidate's leaf passes rule 1 on its own box, and the walk skips exactly the slots that fail it.  Rule 2 is a function of
 *   (shape, triangle) only.  Each triangle is one leaf, so each candidate appears once.
 *   The relation to the casts goes ONE WAY exactly: if triangle i is a candidate here, lbvh_capsule_cast (lbvh_box_cast) of the
 *   same origin (centre), radius and axes gives t = +0 for every active dir whose three components are non-zero and normal and every
 *   t_max > 0 — rule 2 is that definition's start overlap, and rule 1 puts the origin in the closed grown box, where the slab test
 *   of such a dir passes with an entry <= 0 — for the box with axis = LBVH_BOX_AXIS_START.  The cast's triangle index is therefore
 *   <= the least index of the segment.  The converse is NOT promised: a cast may also report t = 0 from a feature root or a
 *   quotient that rounds to zero (the sphere starts one rounding outside and touches within less than the smallest time), and such
 *   a triangle is no candidate here.
 *   A capsule with axis = 0 is allowed: a sphere by this arithmetic (every derived triangle lies in the scene triangle, and the
 *   pierce has det = 0).  Its list is a SUBSET of lbvh_gather_within_distance's for the point origin with r2 = r*r, up to pairs
 *   at the bound itself: dist2 == R2 exactly (closed here, open there), and a derived triangle j >= 1, whose corners are formed
 *   again from a + e, passing one rounding beside j = 0.
 * Output of lbvh_capsule_overlaps / lbvh_obb_overlaps — the CSR contract of lbvh_triangle_intersections, word for word:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[k] = the number of candidates of shapes 0 .. k-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_tris, `capacity` words of 32 bits: segment k = d_tris[d_offsets[k] .. d_offsets[k+1]) = the ORIGINAL triangle indices of
 *   shape k's candidates, each exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT;
 *   lbvh_sort_index_segments applies unchanged and leaves every fitting segment strictly ascending.
 *   Overflow: no word at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; words
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_tris may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill: the same kernel making the same decisions, so a segment never outgrows its slot).
 *   d_tris == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Output of lbvh_capsule_overlaps_any / lbvh_obb_overlaps_any: d_flags[k] = 1 exactly when segment k would be non-empty, else 0;
 * every one of the `count` words is written.  The walk is the same, cut off at a shape's first candidate.
 * All four need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL
 * ctx / d_shapes / h_scene / d_offsets / d_flags, d_shapes not 16-byte aligned, d_offsets not 8-byte aligned, d_tris or d_flags
 * not 4-byte aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves,
 * lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the triangle queries (`rays` =
 * active shapes; triangle_tests counts the triangle lines read, whatever number of derived triangles or axes is tested; the full
 * form reports twice the count-only form's).
 * One shape per lane; the cost is that of a box overlap walk on boxes larger by the shape, plus one 64-byte triangle line and up
 * to eight point tests and a pierce (capsule) or thirteen axes (box) per triangle that passes rule 1.  The capsule's penetration
 * depth and push-out direction per touched triangle are lbvh_capsule_contacts / lbvh_capsule_deepest below.  Out of scope: the
 * box's penetration depth or direction, a contact manifold, flat boxes, a form that spreads one huge shape over the device.
 * (Out of scope of THESE four calls: the box's depth and push-out direction per touched triangle are lbvh_obb_contacts /
 * lbvh_obb_deepest below.) */
lbvh_status lbvh_capsule_overlaps(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);
lbvh_status lbvh_capsule_overlaps_any(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                      uint32_t* d_flags);
lbvh_status lbvh_obb_overlaps(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);
lbvh_status lbvh_obb_overlaps_any(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint32_t* d_flags);

/* One contact of a capsule with a triangle: 32 bytes, arrays 16-byte aligned. */
typedef struct lbvh_contact {
    float    depth;                /* radius - distance of the axis from the triangle; >= radius when the axis reaches the face */
    uint32_t tri;                  /* ORIGINAL triangle index; LBVH_NULL in the none-record */
    float    u, v;                 /* contact point on the triangle: a + e1*u + e2*v */
    float    normal[3];            /* unit push-out direction, from the triangle towards the axis */
    float    s;                    /* contact point on the axis: origin + axis*s, 0 <= s <= 1 */
} lbvh_contact;

/* Capsule contacts: HOW DEEP is a capsule in each triangle it touches, and WHICH WAY OUT (what a character controller asks after
 * lbvh_capsule_overlaps: Physics.ComputePenetration; the per-triangle contacts of a mesh collider), as a CSR list of records
 * (lbvh_capsule_contacts) or as the deepest record per shape (lbvh_capsule_deepest), over the derived traversal scene in its
 * four-wide form by the walk of lbvh_capsule_overlaps.  The active rule, rule 1, rule 2 and therefore the candidate set are
 * lbvh_capsule_overlaps' exactly, from the same operations on the same values: "touches" there and a record here never disagree.
 *   The contact of a candidate (o = origin, h = axis, r = radius; the triangle line a, e1, e2), in strict fp32, every operation
 *   rounded on its own, dot, cross, pierce, dist2 and the derived triangles as defined above:
 *     1. Pierce first.  pierce(o, h; a, e1, e2) of lbvh_triangle_intersections is evaluated for every candidate.  If it passes,
 *        0 <= t_p <= 1, the axis goes through the face: a FACE CONTACT (step 4) with s = t_p.  The centre lies inside the prism
 *        "triangle + segment [0, -h]" exactly in this case, and only then are the distances to the prism's surface not the
 *        distance of the axis from the triangle; so the pierce comes before the distances here, not after all eight fail.
 *     2. Otherwise the nearest derived triangle: d_j = dist2 of lbvh_closest_point_query for o against derived triangle j = 0 .. 7
 *        of lbvh_capsule_cast, with its barycentrics (u', v').  Start with least = +inf and j* = 0; in the order j = 0 .. 7, d_j
 *        replaces least, and j replaces j*, only when d_j < least (strictly; false for a NaN).  s from j* exactly as
 *        lbvh_capsule_cast derives it: 0 for j* = 0, 1 for j* = 1, v' for j* = 2, 4, 6 and 1 - v' for j* = 3, 5, 7.
 *     3. On the scene triangle: x = o + h*s per component; (u, v), ap = x - a, the residual rv = ap - (e1*u + e2*v) per component
 *        and dist2 = dot(rv, rv) are lbvh_closest_point_query's for x against a, e1, e2 — the residual is the vector from the
 *        contact point to the axis.  If dist2 == 0 or dist2 is NaN: a face contact with this s, u, v (step 4).  Otherwise
 *            dist = sqrt(dist2)      normal = rv / dist per component      depth = r - dist.
 *        depth may be a rounding below zero for a candidate at the bound; it is NOT clamped, so that the list stays
 *        lbvh_capsule_overlaps'.
 *     4. Face contact.  N = cross(e1, e2), len = sqrt(dot(N, N)).  If len is 0 or NaN (a degenerate triangle): normal = (0, 0, 0),
 *        depth = r.  Otherwise
 *            g0 = dot(N, o - a)      g1 = dot(N, (o + h) - a)      sign = +1 if g0 + g1 >= 0, else -1
 *            normal = (sign * N) / len per component      depth = r + fmaxf(fmaxf(-sign * g0, -sign * g1), 0) / len
 *        sign is the side the middle of the axis is on, and depth the push along normal that brings the whole axis to the distance
 *        r from the triangle's plane.  In the pierce case (u, v) are lbvh_closest_point_query's for x = o + h*t_p, as in the cast.
 * Output of lbvh_capsule_contacts — lbvh_capsule_overlaps' CSR contract with a record in place of an index:
 *   d_offsets: count + 1 words of 64 bits, the SAME words lbvh_capsule_overlaps writes for these shapes.  Always written in full.
 *   d_contacts, `capacity` records of 32 bytes: segment k = d_contacts[d_offsets[k] .. d_offsets[k+1]) = one record per candidate
 *   of shape k, each triangle exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_contacts may be NULL) — it IS lbvh_capsule_overlaps'
 *   count-only form; otherwise the scene is walked twice (that count walk, the device-side scan, a fill walk that makes the
 *   same decisions from the same values and forms the records).  d_contacts == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Output of lbvh_capsule_deepest: d_out[k] = the contact of shape k with the greatest depth (compared as fp32 values); on equal
 *   depth the lower original triangle index, whatever order the walk meets them in.  A shape with no candidate, or an inactive
 *   shape: the none-record {0, LBVH_NULL, 0, 0, {0, 0, 0}, 0}.  Every one of the `count` records is written.  One walk, no scan.
 *   Nothing can be pruned beyond rule 1: depth has no bound from a box that is monotone in the box — the depth of a face contact
 *   grows with how far the axis reaches THROUGH the triangle, which a box around the triangle says nothing about, and a shallow
 *   contact found first excludes no subtree —, so the walk is lbvh_capsule_overlaps' and visits every candidate.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL
 * ctx / d_shapes / h_scene / d_offsets / d_out, d_shapes, d_contacts or d_out not 16-byte aligned, d_offsets not 8-byte aligned,
 * count > 2^32 - 1.  Four-wide walk only; lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and
 * lbvh_ray_stats_target apply as to lbvh_capsule_overlaps (the full form reports the count walk's plus the fill walk's triangle
 * lines: twice the count-only form's).
 * Cost: a walk of these two visits what lbvh_capsule_overlaps' visits, but no derived triangle ends the loop over the eight, the
 * pierce is evaluated for every triangle that passes rule 1, a candidate takes a ninth point test, and a record is 32 bytes.
 * Out of scope: box and sheared-box contacts (the least-overlap axis of the thirteen); a manifold of more than one point per
 * triangle; a device-side sort of contact segments (lbvh_sort_hit_segments is for 16-byte records); a form that spreads one huge
 * capsule over the device.  (The box and the sheared box have calls of their own: lbvh_obb_contacts / lbvh_obb_deepest below.  The
 * device-side sort of contact segments has one too: lbvh_sort_record_segments, above; with LBVH_SORT_RECORDS_DESCENDING the first
 * record of a segment is lbvh_capsule_deepest's.) */
lbvh_status lbvh_capsule_contacts(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                  uint64_t* d_offsets, lbvh_contact* d_contacts, uint64_t capacity);
lbvh_status lbvh_capsule_deepest(lbvh_context* ctx, const lbvh_capsule* d_shapes, size_t count, const lbvh_scene* h_scene,
                                 lbvh_contact* d_out);

/* A segment query: 32 bytes, arrays 16-byte aligned: lbvh_capsule with a search bound in place of the radius. */
typedef struct lbvh_segment_query {
    float origin[3]; float max_dist2;  /* squared search radius; +inf or >= LBVH_MAX_FLOAT = unbounded */
    float axis[3];   uint32_t _pad;    /* the segment is [origin, origin + axis]; _pad is not read */
} lbvh_segment_query;

/* The answer to one: 32 bytes, arrays 16-byte aligned; written as two 16-byte stores. */
typedef struct lbvh_segment_closest {
    float    dist2;                /* squared distance of the segment from the triangle; LBVH_MAX_FLOAT if none */
    uint32_t tri;                  /* ORIGINAL triangle index; 0 if none */
    float    u, v;                 /* nearest point on the triangle: a + e1*u + e2*v */
    float    delta[3];             /* from that point to the nearest point of the segment; (0, 0, 0) if pierced / none */
    float    s;                    /* nearest point on the segment: origin + axis*s */
} lbvh_segment_closest;

/* Segment closest-point queries: HOW FAR is a segment from the mesh, WHERE and IN WHICH DIRECTION (a capsule's clearance when it
 * touches nothing: Physics.ClosestPoint and the separated case of Physics.ComputePenetration, agent clearance, speculative
 * contacts inside a margin, the nearest surface to a bone, a cable or an edge), as the nearest record per segment
 * (lbvh_segment_closest_point) or as one flag per segment (lbvh_segment_within_distance), over the derived traversal scene in its
 * four-wide form by the walk of lbvh_closest_point_query: one segment per lane, the nearest child box first, boxes farther than
 * the best distance so far skipped.  lbvh_closest_point_query at sample points along the axis misses the nearest feature between
 * samples; lbvh_capsule_deepest with the radius blown up to the search distance prunes nothing beyond its rule 1.  Distance,
 * unlike depth, has a box bound that is monotone in the box.
 *   Active query (o = origin, h = axis): max_dist2 > 0 (false for NaN), no NaN in origin, every component of axis finite.
 *   axis = 0 is allowed (a point, by this definition's arithmetic).  An inactive query is never walked; it gets the none-record
 *   {LBVH_MAX_FLOAT, 0, 0, 0, {0, 0, 0}, 0} (lbvh_segment_closest_point) or 0 (lbvh_segment_within_distance).
 *   R = min(max_dist2, LBVH_MAX_FLOAT), as at the point queries.
 *   Distance of the segment to one triangle (the line a, e1, e2 of the derived scene), in strict fp32, every operation rounded on
 *   its own: steps 1 - 3 of lbvh_capsule_contacts, with dot, pierce, dist2 and the derived triangles as defined above.
 *     1. Pierce first.  pierce(o, h; a, e1, e2) of lbvh_triangle_intersections is evaluated first.  If it passes, 0 <= t_p <= 1:
 *        dist2 = +0, s = t_p, delta = (0, 0, 0), and (u, v) are lbvh_closest_point_query's for x = o + h*t_p (per component
 *        o_k + h_k*t_p) against a, e1, e2.
 *     2. Otherwise the nearest derived triangle: d_j = dist2 of lbvh_closest_point_query for o against derived triangle j = 0 .. 7
 *        of lbvh_capsule_cast, with its barycentrics (u', v').  Start with least = +inf and j* = 0; in the order j = 0 .. 7, d_j
 *        replaces least, and j replaces j*, only when d_j < least (strictly; false for a NaN).  s from j* exactly as
 *        lbvh_capsule_cast derives it: 0 for j* = 0, 1 for j* = 1, v' for j* = 2, 4, 6 and 1 - v' for j* = 3, 5, 7.
 *     3. On the scene triangle: x = o + h*s per component; (u, v), ap = x - a, the residual rv = ap - (e1*u + e2*v) per component
 *        and dist2 = dot(rv, rv) are lbvh_closest_point_query's for x against a, e1, e2.  delta = rv: the vector from the nearest
 *        point of the triangle to the nearest point of the segment.
 *   No square root and no division beyond the point test's own.  A NaN dist2 never counts (every comparison with it is false).
 *   Distance to a box: the box grown by the axis only, one fp32 operation per bound, max and min as fmaxf and fminf,
 *       lo'_k = lo_k - max(h_k, 0)      hi'_k = hi_k - min(h_k, 0)
 *   and box2g = box2 of lbvh_closest_point_query for the point o against (lo', hi'): per axis g = max(max(lo' - o, o - hi'), 0),
 *   (gx*gx + gy*gy) + gz*gz.  (Some point of the segment is in the box, per axis, exactly when o is in the grown box.)
 *   Candidate: triangle i is a candidate for a query iff dist2_i < R and !(dist2_i < box2g(own AABB_i)), the own AABB being
 *   scene.triangle_aabb[i].
 *   lbvh_segment_closest_point: d_out[k] = {dist2, tri, u, v, delta, s} of query k's candidate with the least dist2 (compared as
 *   fp32 values); on equal dist2 the lower original triangle index, whatever order the walk meets them in.  No candidate: the
 *   none-record, never R.  Every one of the `count` records is written, as two 16-byte stores.
 *   lbvh_segment_within_distance: d_flags[k] = 1 if query k has any candidate, else 0.  The walk is the closest walk (same
 *   nearest-first order) cut off at its first accepted candidate: never more node fetches or triangle tests per query.
 * Why the record does not depend on the order of the walk (the argument at lbvh_closest_point_query with grown boxes): the grown
 * bounds lo - max(h, 0) and hi - min(h, 0) are monotone in lo and hi, fp32 subtraction, max, multiplication of non-negatives and
 * addition are monotone, and every box of the derived tree, binary or four-wide, is the exact min / max union of what is below it;
 * so box2g(ancestor) <= box2g(leaf) <= dist2 for every candidate.  A slot is skipped only if box2g > best, strictly: a subtree
 * skipped that way holds no candidate at or below best.  The grown box contains box + segment [0, -h], so box2g is a true lower
 * bound of the distance in exact arithmetic; a dist2 below its own box's box2g is fp32 noise of the triangle arithmetic, which
 * the accept rule removes, as at the point query (on ordinary meshes it rejects nothing).
 * Relations (tests/test_segment_closest.py holds each):
 *   (a) the flag is 1 exactly when the record's dist2 != LBVH_MAX_FLOAT.
 *   (b) with axis = (+0, +0, +0), the same point and the same max_dist2, the first four words {dist2, tri, u, v} equal
 *       lbvh_closest_point_query's record word for word: x = o + 0*s is o exactly, the box is not grown, and the pierce has
 *       det = 0.  (A derived triangle j >= 1, formed again from a + e, may win by a rounding and give another s; x is o all the
 *       same.  Not covered: an origin component that is -0, where o + 0*s is +0.)
 *   (c) per pair: if the capsule {o, r, h} lists the winning triangle in lbvh_capsule_contacts, that contact's s, u, v equal this
 *       record's; when that contact is not a face contact, its depth == r - sqrtf(dist2) and its normal == delta / sqrtf(dist2)
 *       per component, word for word.
 *   (d) the converse of "touching" is NOT promised: rule 2 of lbvh_capsule_overlaps compares d_j <= r*r on the derived triangles;
 *       dist2 here is the ninth test, on the scene triangle at x, and may lie one rounding on the other side of r*r.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_queries or d_out not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves,
 * lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the capsule contacts (`rays` =
 * active queries; triangle_tests counts the triangle lines read, whatever number of derived triangles is tested).
 * Cost: a point query's walk on boxes larger by the axis, and per triangle line the pierce and up to nine point tests.  Pass
 * active queries only where time matters, as at the point queries.
 * Out of scope: the k nearest triangles of a segment; a gather of every triangle within the distance (lbvh_capsule_overlaps with
 * the radius as the distance lists them); oriented boxes (the library has no closed per-pair distance for them yet); a unit
 * normal in the record (delta / sqrtf(dist2) where dist2 > 0; the caller's square root). */
lbvh_status lbvh_segment_closest_point(lbvh_context* ctx, const lbvh_segment_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                       lbvh_segment_closest* d_out);
lbvh_status lbvh_segment_within_distance(lbvh_context* ctx, const lbvh_segment_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                         uint32_t* d_flags);

/* A triangle distance query: 48 bytes, arrays 16-byte aligned: lbvh_tri_query with a search bound (lbvh_tri_query._pad0 stays
 * "not read": that is why this is a struct of its own). */
typedef struct lbvh_tri_distance_query {
    float a[3]; uint32_t skip;       /* ORIGINAL index never a candidate; LBVH_NULL = none (as lbvh_tri_query) */
    float b[3]; float max_dist2;     /* squared search radius; +inf or >= LBVH_MAX_FLOAT = unbounded */
    float c[3]; uint32_t _pad;       /* not read */
} lbvh_tri_distance_query;

/* The answer to one: 32 bytes, arrays 16-byte aligned; written as two 16-byte stores. */
typedef struct lbvh_tri_closest {
    float    dist2;                /* squared distance of the two triangles; LBVH_MAX_FLOAT if none */
    uint32_t tri;                  /* ORIGINAL triangle index; 0 if none */
    uint32_t edge;                 /* m = 0..5: which edge test gave the record; | 8 when that edge pierces */
    float    s;                    /* nearest point on that edge: P_m + D_m * s */
    float    delta[3];             /* from the scene triangle's nearest point to the query's nearest point; 0 if pierced / none */
    uint32_t _zero;                /* written as 0 */
} lbvh_tri_closest;

/* Triangle closest-point queries: HOW FAR is a triangle from the mesh, WHERE and IN WHICH DIRECTION (the minimum distance between
 * two meshes: clearance and tolerance checks, assembly planning; proximity pairs for cloth and self-collision, a mesh against
 * itself with `skip`; speculative contacts for mesh colliders inside a margin), as the nearest record per query triangle
 * (lbvh_triangle_closest_point) or as one flag per query (lbvh_triangle_within_distance), over the derived traversal scene in its
 * four-wide form by the walk of lbvh_segment_closest_point: one query per lane, the nearest child box first, boxes farther than
 * the best distance so far skipped.  Three lbvh_segment_closest_point calls on the query's edges miss every case where a scene
 * vertex or edge is nearest to the interior of the query's face (the usual case when the query is larger than the scene's
 * triangles); rows of lbvh_closest_point_query samples miss features between samples; lbvh_box_overlaps with a padded box and a
 * host narrow phase prunes nothing by distance.
 *   Active query: all nine coordinates of a, b, c finite and max_dist2 > 0 (false for NaN).  a == b == c is allowed (by this
 *   definition's arithmetic; see (d)).  An inactive query is never walked; it gets the none-record
 *   {LBVH_MAX_FLOAT, 0, 0, 0, {0, 0, 0}, 0} (lbvh_triangle_closest_point) or 0 (lbvh_triangle_within_distance).
 *   R = min(max_dist2, LBVH_MAX_FLOAT), as at the point queries.
 *   Query box: Q.min_k = min(min(a_k, b_k), c_k), Q.max_k = max(max(a_k, b_k), c_k), exactly as lbvh_triangle_intersections forms
 *   them: exact, not padded.
 *   Distance of the query to one triangle (the line v0, e1, e2 of the derived scene), in strict fp32, every operation rounded on
 *   its own: the distance between two triangles is zero if an edge of one pierces the other, else the least distance between an
 *   edge of one and the other triangle.  Six edge tests, in the order and with the P, D of lbvh_triangle_intersections, every
 *   difference and sum one fp32 operation per component:
 *     m = 0, 1, 2: the query's edges (P, D) = (a, b - a), (b, c - b), (c, a - c) against the scene line (v0, e1, e2);
 *     m = 3, 4, 5: the scene's edges (P, D) = (v0, e1), (v0, e2), (v0 + e1, e2 - e1) against the query's line (a, b - a, c - a).
 *   Each test is the full per-pair distance of lbvh_segment_closest_point for the segment (o, h) = (P, D) against that line, its
 *   steps 1 - 3 (pierce first — the very pierce of lbvh_triangle_intersections' test m —, else the nearest derived triangle picks
 *   s, then the point test at x = P + D*s): it gives dist2_m, s_m, the residual rv_m (step 3's rv) and whether it pierced.
 *   Pair result: start with least = +inf; in the order m = 0 .. 5, test m replaces the running result only when dist2_m < least,
 *   strictly (false for a NaN).  The record takes dist2 = dist2_m, s = s_m, edge = m | (pierced ? 8 : 0), and delta = rv_m for
 *   m < 3, -rv_m per component for m >= 3 (an fp32 sign flip: it may produce -0), (+0, +0, +0) where pierced: delta always points
 *   from the scene triangle's nearest point to the query's nearest point.  With no dist2_m below +inf the pair's dist2 is +inf:
 *   never a candidate.
 *   Early exit: an implementation may stop at the first m with dist2_m == +0: nothing after it is strictly less.
 *   Distance to a box B (box against box): per axis g_k = fmaxf(fmaxf(B.lo_k - Q.max_k, Q.min_k - B.hi_k), 0) and
 *   box2q(B) = (gx*gx + gy*gy) + gz*gz.
 *   Candidate: triangle i is a candidate for a query iff its ORIGINAL index != skip, dist2_i < R and
 *   !(dist2_i < box2q(own AABB_i)), the own AABB being scene.triangle_aabb[i].
 *   lbvh_triangle_closest_point: d_out[k] = {dist2, tri, edge, s, delta, 0} of query k's candidate with the least dist2 (compared as
 *   fp32 values); on equal dist2 the lower original triangle index, whatever order the walk meets them in.  No candidate: the
 *   none-record, never R.  Every one of the `count` records is written, as two 16-byte stores.
 *   lbvh_triangle_within_distance: d_flags[k] = 1 if query k has any candidate, else 0.  The walk is the closest walk (same
 *   nearest-first order) cut off at its first accepted candidate: never more node fetches or triangle tests per query.
 * Why the record does not depend on the order of the walk (the argument at lbvh_segment_closest_point with box2q for box2g): box2q
 * is monotone in B.lo and B.hi — fp32 subtraction, max, multiplication of non-negatives and addition are monotone — and every box
 * of the derived tree, binary or four-wide, is the exact min / max union of what is below it; so
 * box2q(ancestor) <= box2q(leaf) <= dist2 for every candidate.  A slot is skipped only if box2q > best, strictly: a subtree
 * skipped that way holds no candidate at or below best.  Both triangles lie in their boxes, so box2q is a true lower bound of the
 * distance in exact arithmetic; a dist2 below its own box's box2q is fp32 noise of the triangle arithmetic, which the accept rule
 * removes (on ordinary meshes it rejects nothing).
 * Relations (tests/test_triangle_closest.py holds each):
 *   (a) the flag is 1 exactly when the record's dist2 != LBVH_MAX_FLOAT.
 *   (b) if lbvh_triangle_intersections lists any triangle for {a, b, c, skip}, the record has dist2 == +0, edge & 8 set and
 *       tri <= the least listed index: the pierce tests are the same six calls, and overlapping boxes have box2q = 0.
 *   (c) with skip = LBVH_NULL, for m = 0, 1, 2 the record's dist2 is <= the dist2 of lbvh_segment_closest_point on edge m
 *       ({P_m, max_dist2, D_m}) wherever the accept rule rejected nothing for that query; where the record has edge == m < 3 and the
 *       same tri as that segment record, dist2, s and delta are equal word for word.
 *   (d) NOT promised: that a degenerate query (a == b == c) equals lbvh_closest_point_query at a.  Tests m >= 3 run the point
 *       test against a degenerate triangle (a, 0, 0) and may give another rounding of the same distance.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op.  Rejected: NULL pointers, d_queries or d_out not 16-byte aligned, d_flags not 4-byte
 * aligned, count > 2^32 - 1.  Four-wide walk only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves,
 * lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and lbvh_ray_stats_target apply as to the segment queries (`rays` =
 * active queries; triangle_tests counts the triangle lines read and tested, whatever number of edge tests each takes; a line whose
 * index is `skip` is not counted, as at lbvh_triangle_intersections).
 * Cost: up to six segment tests (54 point tests) per triangle line read: several times lbvh_segment_closest_point's narrow phase on
 * boxes grown by the whole query.  Pass active queries only where time matters, and a search radius where one is known.
 * Every triangle within the distance, not only the nearest: lbvh_triangle_gather_within_distance below.
 * Out of scope: the k nearest triangles of a triangle; a two-tree (mesh-BVH against mesh-BVH) descent; exact coplanar-overlap
 * handling beyond what the arithmetic gives; oriented-box distance; a unit normal in the record (delta / sqrtf(dist2) where
 * dist2 > 0; the caller's square root). */
lbvh_status lbvh_triangle_closest_point(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                        lbvh_tri_closest* d_out);
lbvh_status lbvh_triangle_within_distance(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count, const lbvh_scene* h_scene,
                                          uint32_t* d_flags);

/* Triangle proximity: EVERY scene triangle within a distance of a triangle, each with its distance, witness feature and direction
 * (what a cloth or contact solver asks: proximity pairs for cloth and self-collision, a mesh against itself with `skip`; speculative
 * contacts for mesh colliders inside a margin — one record per PAIR, where lbvh_triangle_closest_point gives one per query), as a
 * CSR list of lbvh_tri_closest records over the derived traversal scene in its four-wide form, one query per lane.  The last cell
 * of the distance family: lbvh_gather_within_distance for a point, lbvh_capsule_contacts for a segment, this call for a triangle.
 * Everything is defined by reference to lbvh_triangle_closest_point above:
 *   Arithmetic: the active query, R, the query box, the six edge tests, the pair result (dist2, edge, s, delta) and box2q are that
 *   call's, unchanged; so is the early exit at the first dist2_m == +0.
 *   Candidate: triangle i is a candidate for a query iff its ORIGINAL index != skip, dist2_i < R and
 *   !(dist2_i < box2q(own AABB_i)): the same predicate as the closest call's.  The radius is open: dist2 == R is not listed.
 *   Record: the record of a candidate is what lbvh_triangle_closest_point would write were that triangle the only one:
 *   {dist2, tri, edge, s, delta, 0}.
 *   Slot test: a slot of the tree is entered iff box2q(slot) < R (false for a NaN).  There is no nearest-first order and no
 *   shrinking bound: every passing slot is visited.
 * Why the list does not depend on the walk (the argument at lbvh_gather_within_distance with box2q for box2): box2q is monotone in
 * the box and every box of the derived tree is the exact min / max union of what is below it, so
 * box2q(ancestor) <= box2q(leaf) <= dist2 < R for every candidate, against a fixed bound: every slot on the way to a candidate is
 * entered, whatever the order.  Each triangle is one leaf, so each candidate appears exactly once.
 * Output — the CSR contract of lbvh_gather_within_distance / lbvh_capsule_contacts with a 32-byte record:
 *   d_offsets: count + 1 words of 64 bits, segment k = d_records[d_offsets[k] .. d_offsets[k+1]), d_offsets[count] = the total.
 *   Always written in full.
 *   d_records, `capacity` records of 32 bytes, each written as two 16-byte stores: one record per candidate of query k.  THE ORDER
 *   INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT (sort on the host by (dist2, tri) where an order is needed).
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_records may be NULL); otherwise the scene is walked twice
 *   (a count walk, the device-side scan, a fill walk that makes the same decisions from the same values and forms delta).
 *   d_records == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.  Two calls on the same input write the same bytes.
 *   An inactive query gets an empty segment.
 * Relations (tests/test_triangle_proximity.py holds each):
 *   (a) segment k is non-empty exactly when lbvh_triangle_within_distance gives 1 for query k.
 *   (b) the least record of a non-empty segment by (dist2 as an fp32 value, tri) equals lbvh_triangle_closest_point's record in
 *       all eight words.
 *   (c) every triangle lbvh_triangle_intersections lists for {a, b, c, skip} is in the segment with dist2 == +0 and edge & 8 set.
 *       The converse is NOT promised (a pair at distance +0 without a pierce, a touching vertex, is listed here and not there).
 *   (d) the capacity == 0 form writes the same offsets as the full form.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG with this entry point's name), is
 * asynchronous on the context's stream with no host wait, and uses the context's ray scratch: it drops the path tracer's live-path
 * list (see lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.
 * Rejected: NULL ctx / d_queries / h_scene / d_offsets, d_queries or d_records not 16-byte aligned, d_offsets not 8-byte aligned,
 * count > 2^32 - 1.  Four-wide walk only; lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and
 * lbvh_ray_stats_target apply as to lbvh_capsule_contacts (`rays` = active queries per walk; triangle_tests counts the triangle
 * lines read after `skip`; the full form reports the count walk's plus the fill walk's: twice the count-only form's).
 * Cost: an unbounded query lists the whole mesh.  There is no shrinking bound, so every pair whose boxes are inside R pays up to
 * six segment tests (54 point tests) in BOTH walks; pass the margin the solver needs, not more.
 * Out of scope: a device-side sort of 32-byte records (the host sorts; lbvh_sort_hit_segments is for 16-byte records); the k
 * nearest triangles of a triangle; a two-tree (mesh-BVH against mesh-BVH) descent; removing the (i, j) / (j, i) duplicates or the
 * adjacent triangles of a self-query on the device (the host does, from the returned list).  (Out of scope of THIS call: the
 * device-side sort of 32-byte records is lbvh_sort_record_segments, above; with LBVH_SORT_RECORDS_ASCENDING the first record of a
 * segment is lbvh_triangle_closest_point's.) */
lbvh_status lbvh_triangle_gather_within_distance(lbvh_context* ctx, const lbvh_tri_distance_query* d_queries, size_t count,
                                                 const lbvh_scene* h_scene, uint64_t* d_offsets, lbvh_tri_closest* d_records,
                                                 uint64_t capacity);

/* One contact of an oriented box with a triangle: 32 bytes, arrays 16-byte aligned; written as two 16-byte stores. */
typedef struct lbvh_box_contact {
    float    depth;                /* least push, along normal, that separates the box from the triangle; >= 0 */
    uint32_t tri;                  /* ORIGINAL triangle index; LBVH_NULL in the none-record */
    uint32_t axis;                 /* the j of lbvh_box_cast's thirteen axes that gave depth; LBVH_BOX_AXIS_START if none counted */
    float    back;                 /* the push that separates along -normal on the same axis; >= depth */
    float    normal[3];            /* unit push-out direction for the BOX, from the triangle towards the box */
    uint32_t _zero;
} lbvh_box_contact;

/* Box contacts: HOW DEEP is an oriented box in each triangle it touches, and WHICH WAY OUT (what a crate, a hull or a placement
 * preview asks after lbvh_obb_overlaps: Physics.ComputePenetration for a BoxCollider), as a CSR list of records
 * (lbvh_obb_contacts) or as the deepest record per shape (lbvh_obb_deepest), over the derived traversal scene in its four-wide
 * form by the walk of lbvh_obb_overlaps.  The active rule, rule 1, rule 2 and therefore the candidate set are lbvh_obb_overlaps'
 * exactly, from the same operations on the same values: "touches" there and a record here never disagree.
 *   The contact of a candidate (c = centre, b_0, b_1, b_2 = ax, ay, az; the triangle line a, e1, e2), in strict fp32, every
 *   operation rounded on its own, dot, cross, min, max and / as at lbvh_box_cast, sqrt correctly rounded: the least-overlap axis
 *   of the thirteen.  For every axis j = 0 .. 12 of lbvh_box_cast, in its order, with L = L_j, m = a - c, lo, hi and rb exactly
 *   as there (the values rule 2 compares):
 *       len2 = dot(L, L)      pos = hi + rb      neg = rb - lo
 *   From the box's centre the triangle covers [lo, hi] on L and the box [-rb, rb]: moved by pos along +L the box's interval
 *   begins where the triangle's ends, moved by neg along -L it ends where the triangle's begins.  Both are >= 0 for a candidate
 *   (rule 2: -rb <= hi and lo <= rb, and a sum of two fp32 values whose exact sum is >= 0 rounds to a value >= 0).
 *   Axis j COUNTS only if len2 is a normal finite number, 2^-126 <= len2 < +inf.  A zero axis (parallel edges, a degenerate
 *   triangle) has no direction, and a denormal len2 no longer carries L's precision: both are skipped, and so is an overflow.
 *   A near-zero but normal axis is taken as the direction it is, as lbvh_box_cast takes it: the projections are accurate
 *   relative to the computed L, the push along ANY direction separates, and the least push over all directions is attained on
 *   one of the thirteen exact axes; a noisy extra direction therefore cannot undercut the answer beyond ordinary roundoff.
 *   For an axis that counts:
 *       len = sqrt(len2)      pen = fminf(pos, neg)      far = fmaxf(pos, neg)      d_j = pen / len
 *       sign = +1 if pos <= neg, else -1
 *   Start with least = +inf and axis = LBVH_BOX_AXIS_START.  In the order of j, d_j replaces least, and j replaces axis, only
 *   when d_j < least (strictly; false for a NaN).  For the winner j:
 *       depth = d_j      back = far / len      normal = (sign * L) / len per component
 *   depth and back come from the same axis: the box is free after depth along normal or after back along -normal, and
 *   back >= depth.  depth >= 0, and it is NOT the distance to travel along any other direction.  If no axis counts (every L_j
 *   zero, denormal or overflowing): the record {0, tri, LBVH_BOX_AXIS_START, 0, {0, 0, 0}, 0}.  The record is a function of
 *   (shape, triangle) only.
 *   For axis = 0 normal is the triangle's face normal, for 1 .. 3 a face normal of the box, for 4 + 3*i + k the common
 *   perpendicular of the box's edge b_i and the triangle's edge E_k.  This is the direction lbvh_box_cast reports for a box that
 *   arrives along -normal, with the sign chosen by the shorter way out instead of by a motion.
 * Output of lbvh_obb_contacts — lbvh_obb_overlaps' CSR contract with a record in place of an index:
 *   d_offsets: count + 1 words of 64 bits, the SAME words lbvh_obb_overlaps writes for these shapes.  Always written in full.
 *   d_contacts, `capacity` records of 32 bytes: segment k = d_contacts[d_offsets[k] .. d_offsets[k+1]) = one record per candidate
 *   of shape k, each triangle exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_contacts may be NULL) — it IS lbvh_obb_overlaps'
 *   count-only form; otherwise the scene is walked twice (that count walk, the device-side scan, a fill walk that makes the
 *   same decisions from the same values and forms the records).  d_contacts == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Output of lbvh_obb_deepest: d_out[k] = the contact of shape k with the greatest depth (compared as fp32 values); on equal
 *   depth the lower original triangle index, whatever order the walk meets them in.  A shape with no candidate, or an inactive
 *   shape: the none-record {0, LBVH_NULL, 0, 0, {0, 0, 0}, 0}.  Every one of the `count` records is written.  One walk, no scan.
 *   Nothing can be pruned beyond rule 1: the depth of a contact grows with how far the box reaches THROUGH the triangle, which a
 *   box around the triangle says nothing about, and a shallow contact found first excludes no subtree, so the walk is
 *   lbvh_obb_overlaps' and visits every candidate.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected: NULL
 * ctx / d_shapes / h_scene / d_offsets / d_out, d_shapes, d_contacts or d_out not 16-byte aligned, d_offsets not 8-byte aligned,
 * count > 2^32 - 1.  Four-wide walk only; lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and
 * lbvh_ray_stats_target apply as to lbvh_obb_overlaps (the full form reports the count walk's plus the fill walk's triangle
 * lines: twice the count-only form's).
 * Cost: a walk of these two visits what lbvh_obb_overlaps' visits; a triangle that passes rule 1 takes, per axis that counts
 * and until the first separating axis, one square root and one division more, a candidate four divisions more, and a record is
 * 32 bytes.
 * Out of scope: a contact point or a manifold for the box (a box touches a triangle in a point, a segment or a polygon); flat
 * boxes (det == 0 is inactive, as everywhere); a device-side sort of 32-byte segments (lbvh_sort_hit_segments is for 16-byte
 * records); a form that spreads one huge box over the device.  (Out of scope of THESE two calls: the device-side sort of 32-byte
 * segments is lbvh_sort_record_segments, above; with LBVH_SORT_RECORDS_DESCENDING the first record of a segment is
 * lbvh_obb_deepest's.) */
lbvh_status lbvh_obb_contacts(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                              uint64_t* d_offsets, lbvh_box_contact* d_contacts, uint64_t capacity);
lbvh_status lbvh_obb_deepest(lbvh_context* ctx, const lbvh_obb* d_shapes, size_t count, const lbvh_scene* h_scene,
                             lbvh_box_contact* d_out);

/* A convex region bounded by six planes: 96 bytes; arrays of them 16-byte aligned.  A plane {nx, ny, nz, d} keeps the half space
 * n . x + d >= 0; the region is the intersection of its six half spaces.  Normals need not be unit length.  A region with fewer
 * faces repeats a plane or pads with {0, 0, 0, 1}. */
#define LBVH_REGION_PLANES    6
#define LBVH_REGION_TOUCHING  0u   /* triangles whose box is not wholly outside any plane  */
#define LBVH_REGION_CONTAINED 1u   /* triangles whose box is wholly inside every plane     */
typedef struct lbvh_region { float plane[LBVH_REGION_PLANES][4]; } lbvh_region;   /* 96 bytes, arrays 16-byte aligned */

/* Region queries: WHICH triangles lie in a convex region bounded by planes — a camera or light frustum, an oriented box, an
 * editor's window / crossing selection —, as a CSR list (lbvh_region_overlaps) or as one flag per region
 * (lbvh_region_overlaps_any), over the derived traversal scene in its four-wide form by the walk of lbvh_box_overlaps.
 *   Arithmetic: strict fp32, every operation rounded on its own, no contraction, gradual underflow (what numpy does).  For a box
 *   [lo, hi] and a plane {nx, ny, nz, d} — the comparison n_a >= 0 is true for -0 and false for NaN —
 *       P = ((nx * (nx >= 0 ? hi.x : lo.x) + ny * (ny >= 0 ? hi.y : lo.y)) + nz * (nz >= 0 ? hi.z : lo.z)) + d
 *       N = ((nx * (nx >= 0 ? lo.x : hi.x) + ny * (ny >= 0 ? lo.y : hi.y)) + nz * (nz >= 0 ? lo.z : hi.z)) + d
 *   P is the plane's value at the box corner farthest along the normal, N at the nearest.
 *   Candidate: with A = scene.triangle_aabb[i], the padded own box the leaf slot holds, and P_j, N_j for plane j = 0 .. 5,
 *     mode LBVH_REGION_TOUCHING:  triangle i is a candidate iff P_j(A) >= 0 for all six planes;
 *     mode LBVH_REGION_CONTAINED: triangle i is a candidate iff N_j(A) >= 0 for all six planes.
 *   What follows from this definition:
 *     A NaN anywhere makes its comparison false, so there are no special cases and no "inactive query" rule: a region with a NaN
 *     plane simply has no candidates.  (An infinite word gives what the arithmetic gives: +-inf or, from inf - inf or 0 * inf, NaN.)
 *     TOUCHING is a broad phase on the triangles' BOXES by design: the standard conservative frustum test, which may accept a box
 *     near a corner of the region that no single plane rejects.  It is the box analogue of lbvh_box_overlaps.
 *     CONTAINED is exact in the useful direction: a triangle lies inside its own box, so a CONTAINED triangle is wholly inside
 *     the region.  A caller can skip clipping for it, and an editor gets window selection.
 *   Why the list does not depend on the walk: fp32 multiplication by a fixed factor and fp32 addition are monotone, and every box
 *   of the derived tree, binary or four-wide, is the exact min / max union of what lies below it.  So for a leaf box A below a slot
 *   box B, P_j(B) >= P_j(A): per axis the factor's sign picks hi, which only grows towards the root, or lo, which only shrinks.
 *   With lo <= hi, N_j(A) <= P_j(A).  Hence every ancestor slot of a candidate of EITHER mode passes the TOUCHING test.  The walk
 *   enters a slot iff all six P_j >= 0 and applies the mode's test at leaf slots only.  Each triangle is one leaf, so each
 *   candidate appears exactly once.
 * Output of lbvh_region_overlaps — the CSR contract of lbvh_box_overlaps, word for word:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[k] = the number of candidates of regions 0 .. k-1, d_offsets[count] = the
 *   total M.  Always written in full, whatever `capacity` is.
 *   d_tris, `capacity` words of 32 bits: segment k = d_tris[d_offsets[k] .. d_offsets[k+1]) = the ORIGINAL triangle indices of
 *   region k's candidates, each exactly once.  THE ORDER INSIDE A SEGMENT IS THE WALK'S AND IS NOT PART OF THE CONTRACT;
 *   lbvh_sort_index_segments applies unchanged and leaves every fitting segment strictly ascending.
 *   Overflow: no word at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; words
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets and walks once (d_tris may be NULL); otherwise the scene is walked twice
 *   (count, device-side scan, fill: the same kernel making the same decisions, so a segment never outgrows its slot).
 * Output of lbvh_region_overlaps_any: d_flags[k] = 1 exactly when segment k would be non-empty, else 0; every one of the `count`
 * words is written.  The walk is the same, cut off at a region's first candidate.
 * Both need the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), are asynchronous on the
 * context's stream with no host wait, and use the context's ray scratch: they drop the path tracer's live-path list (see
 * lbvh_path_bounce).  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected
 * (LBVH_ERR_INVALID_ARG): NULL ctx / d_regions / h_scene / d_offsets / d_flags, mode > 1, d_regions not 16-byte aligned, d_offsets
 * not 8-byte aligned, d_tris or d_flags not 4-byte aligned, d_tris == NULL with capacity > 0, count > 2^32 - 1.  Four-wide walk
 * only (lbvh_debug_ray_walker does not apply); lbvh_debug_ray_waves, lbvh_debug_ray_stack_split, lbvh_debug_ray_stack_limit and
 * lbvh_ray_stats_target apply as to the overlap queries (rays counts every region, triangle_tests the leaf slots that passed the
 * TOUCHING test; the full form reports twice the count-only form's).
 * One region per lane: a single camera frustum over the whole mesh keeps one lane busy while 63 idle.  The call is for MANY
 * regions (clusters, lights, oriented boxes, portals), not for one huge one: that is lbvh_region_overlaps_large below. */
lbvh_status lbvh_region_overlaps(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                 uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);
lbvh_status lbvh_region_overlaps_any(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                     uint32_t* d_flags);

/* lbvh_region_overlaps for FEW, LARGE regions — one camera or light frustum, a cascade, a marquee selection: every region is
 * spread over the device instead of over one lane.  The same lbvh_region, the same two modes, the same candidate predicate
 * operation by operation, the same CSR contract word for word: d_offsets (count + 1 words of 64 bits) is always written in full
 * and EQUALS lbvh_region_overlaps' d_offsets on the same inputs; segment k holds the same SET of ORIGINAL triangle indices, each
 * exactly once — after lbvh_sort_index_segments d_tris equals that call's sorted d_tris word for word; no word at index >=
 * capacity is ever written and every segment with d_offsets[k+1] <= capacity is complete; capacity == 0 is the count-only form
 * (d_tris may be NULL).  THE ORDER INSIDE A SEGMENT IS NOT PART OF THE CONTRACT (it differs from lbvh_region_overlaps'), but two
 * calls with the same inputs on the same scene write the same bytes: no atomic is on the output path.
 *   How: a region is cut into up to task_cap TASKS.  One workgroup per region opens the four-wide tree breadth first from the
 *   root with the slot test of lbvh_region_overlaps (an inner slot that passes all six P_j >= 0 replaces its parent; a leaf slot
 *   stays only if it is a candidate of the mode) until one more round could exceed task_cap entries or only leaves are left.
 *   By the monotonicity argument above, a region's candidates are the union of the candidates below the subtrees of ANY such
 *   frontier, and no two of them share a triangle.  Every task is then walked by one lane exactly as lbvh_region_overlaps
 *   walks a region, a leaf task is a candidate already; the per-task counts are scanned on the device into 64-bit task offsets,
 *   d_offsets picks every region's first, and the fill walk writes each task's candidates at the task's own offset.  No kernel
 *   waits for another workgroup.  task_cap is chosen by the host: the largest power of two not above min(65536, 2^22 / count),
 *   so count * task_cap <= 2^22 task slots; count <= LBVH_REGION_LARGE_MAX_COUNT keeps it at 64 or more.
 *   When to use which (MI355X, 1 M triangles, TOUCHING, tools/region_large_bench.py -> profiles/region_large/, table in DESIGN.md
 *   §30): use this call when there are at most 65 536 regions and a region holds hundreds of triangles or more.  One frustum
 *   over 50 % of the mesh: 0.38 ms count only and 0.68 ms full against lbvh_region_overlaps' 316 ms and 717 ms; one region of
 *   829 triangles: 0.044 ms against 0.49 ms; 4 096 regions of 47 000 triangles: 4.2 ms against 55 ms.  The gap closes as the
 *   regions get many and small: 65 536 regions of about 600 triangles take 2.18 ms against 2.68 ms count only (1.2x) and 4.00 ms
 *   against 6.13 ms full (1.5x), the smallest gain measured; it lost in no cell measured.  Below that size — regions of a few
 *   triangles, where the 64 task slots per region are mostly empty — and above 65 536 regions lbvh_region_overlaps is the call
 *   (2^20 regions of about 100 triangles: 1.99 ms there).
 * Everything else is lbvh_region_overlaps': the derived traversal scene is needed (a stale one is LBVH_ERR_INVALID_ARG),
 * asynchronous on the context's stream with no host wait, the path tracer's live-path list is dropped, count == 0 is a no-op that
 * touches no buffer.  It keeps count * task_cap * 16 bytes (up to 64 MB) of context scratch of its own beside the ray scratch;
 * a failed allocation is LBVH_ERR_OUT_OF_MEMORY and leaves the context usable.  Rejected (LBVH_ERR_INVALID_ARG, the message
 * names this entry point): NULL ctx / d_regions / h_scene / d_offsets, mode > 1, d_regions not 16-byte aligned, d_offsets not
 * 8-byte aligned, d_tris not 4-byte aligned, d_tris == NULL with capacity > 0, count > LBVH_REGION_LARGE_MAX_COUNT.
 * lbvh_debug_ray_waves, lbvh_debug_ray_stack_split and lbvh_debug_ray_stack_limit apply to the task walks;
 * lbvh_ray_stats_target: rays counts the tasks that are not empty, node_fetches the node lines of the task walks PLUS the nodes
 * the expansion opened, triangle_tests the leaf slots that passed the TOUCHING test in a task walk plus the leaf tasks; the
 * full form adds the walks' share twice.  There is no _any twin: lbvh_region_overlaps_any stops at a region's first candidate,
 * so a large region is its fast case already. */
#define LBVH_REGION_LARGE_MAX_COUNT 65536
lbvh_status lbvh_region_overlaps_large(lbvh_context* ctx, const lbvh_region* d_regions, size_t count, uint32_t mode, const lbvh_scene* h_scene,
                                       uint64_t* d_offsets, uint32_t* d_tris, uint64_t capacity);

/* A plane n . x + d = 0: 16 bytes, arrays 16-byte aligned.  The normal need not be unit length; the side n . x + d >= 0 is the
 * positive side. */
typedef struct lbvh_plane { float n[3]; float d; } lbvh_plane;

/* Where a plane cuts one scene triangle: 32 bytes, arrays 16-byte aligned; written as two 16-byte stores. */
typedef struct lbvh_plane_segment {
    float p0[3]; uint32_t tri;     /* the crossing on the edge that leaves the positive side; ORIGINAL index of the scene triangle */
    float p1[3]; uint32_t edges;   /* the crossing on the edge that returns to it; which edges, and the three sides (below) */
} lbvh_plane_segment;

/* Plane sections: WHERE does a plane cut the mesh — a cross-section or contour line, a slice for 3D printing, one image of a
 * CT-style stack, a water line, the outline of a clipping cap, a section view in an editor —, as a CSR list of one record per cut
 * triangle over the derived traversal scene in its four-wide form, every plane spread over the device in the frame of
 * lbvh_region_overlaps_large.
 *   Arithmetic: strict fp32, every operation rounded on its own, no contraction, gradual underflow (what numpy does).
 *       pv(x) = ((nx * x0 + ny * x1) + nz * x2) + d        the expression lbvh_region_overlaps uses for a plane's value
 *   Box test: for a box [lo, hi], P and N are exactly the P and N of lbvh_region_overlaps above for the plane {n, d} — the plane's
 *   value at the box corner farthest and nearest along n, each axis choosing by n_a >= 0 (true for -0, false for NaN).  A box
 *   passes iff P >= 0 && N <= 0.  Any NaN makes the test false, so a NaN plane has no candidates.  (An infinite word gives what
 *   the arithmetic gives; where a record then holds a NaN, which NaN is not specified.)
 *   Candidate: triangle i has the line (a, e1, e2) of the derived scene (e1 = b - a, e2 = c - a, fp32 differences taken once at
 *   build time) and the padded own box A = scene.triangle_aabb[i].  It is a candidate iff
 *     (1) A passes the box test, and
 *     (2) with V0 = a, V1 = a + e1, V2 = a + e2 (per component), s_k = pv(V_k) and side_k = (s_k >= 0) (true for -0, false for
 *         NaN), the three sides are not all equal.
 *   A triangle lying in the plane (all s_k == 0) has three equal sides and is not reported: coplanar faces are out of scope, as in
 *   the triangle queries.
 *   Record of a candidate: of the edges E0 = V0 -> V1, E1 = V1 -> V2, E2 = V2 -> V0 exactly two join different sides (true of any
 *   three booleans that are not all equal).  For such an edge let (Vp, sp) be its end with side true and (Vm, sm) the other end:
 *       t = sp / (sp - sm),    X = Vp + (Vm - Vp) * t     per component: one subtraction, one multiplication, one addition.
 *   The crossing is computed from the positive end whichever way the edge runs, so it is a function of the two endpoint values
 *   only.  p0 is the crossing on the edge that runs from the true side to the false side in the order above, p1 the crossing on
 *   the other edge (which runs from false to true).  tri is the ORIGINAL triangle index.  edges: bits 0 .. 2 the two crossing
 *   edges (bit k: E_k); bits 8 .. 9 the edge that gave p0; bits 12 .. 13 the edge that gave p1; bits 16 .. 18 side_0 .. side_2;
 *   every other bit zero.
 *   What follows from this definition:
 *     STITCHING.  On a consistently wound mesh the neighbour across an edge runs it the other way, so the p1-edge of one record
 *     is the p0-edge of the neighbour across it: all records of a contour run the same way round (p0 -> p1 turns about n in one
 *     sense on an outward-wound closed mesh), and a caller stitches closed, oriented contours by (triangle, edge) through the
 *     mesh's own adjacency — no floats are compared.
 *     Two triangles compute bit-identical crossings on a shared edge only if their lines give bit-identical vertices: a + e1 can
 *     differ from the stored vertex in the last place, so matching ends by float value is NOT promised.
 *     A vertex exactly on the plane (s_k == 0) counts as the positive side.  It gives a zero-length record (p0 == p1 up to the
 *     rounding of a + e) in triangles that otherwise lie on the negative side, and none in triangles that otherwise lie on the
 *     positive side.
 *   Why the list does not depend on the walk — the argument of lbvh_region_overlaps: every box of the derived tree is the exact
 *   min / max union of what lies below it, fp32 multiplication by a fixed factor and fp32 addition are monotone, so P only grows
 *   towards the root and N only shrinks: every ancestor slot of a candidate's leaf passes the box test.  Rule (2) and the record
 *   are functions of (plane, triangle) only.  Each triangle is one leaf, so each candidate appears exactly once.
 *   How: lbvh_region_overlaps_large's pipeline.  One workgroup per plane opens the four-wide tree breadth first with the box
 *   test until one more round could exceed task_cap entries or only leaves are left (a leaf slot stays iff its box passes; the
 *   expansion reads no triangle); every task is walked by one lane, which reads the triangle's 64-byte line at every leaf slot
 *   that passes — and for a leaf task — and applies rule (2); the per-task counts are scanned into 64-bit task offsets, d_offsets
 *   picks every plane's first, and the fill walk, taking the same decisions from the same values, writes each task's records at
 *   the task's own offset.  No atomic is on the output path and no kernel waits for another workgroup.  task_cap is
 *   lbvh_region_overlaps_large's: the largest power of two not above min(65536, 2^22 / count).
 * Output — lbvh_triangle_intersection_segments' CSR contract, word for word:
 *   d_offsets: count + 1 words of 64 bits.  d_offsets[k] = the number of candidates of planes 0 .. k-1, d_offsets[count] = the
 *   total.  Always written in full, whatever `capacity` is.
 *   d_segments, `capacity` records of 32 bytes: segment k = d_segments[d_offsets[k] .. d_offsets[k+1]) = one record per candidate
 *   of plane k, each triangle exactly once.  THE ORDER INSIDE A SEGMENT IS NOT PART OF THE CONTRACT (sort by `tri` on the host if
 *   an order is needed), but two calls with the same inputs on the same scene write the same bytes.
 *   Overflow: no record at index >= capacity is ever written; every segment with d_offsets[k+1] <= capacity is complete; records
 *   below `capacity` that belong to a segment which does not fit are unspecified.  The call never waits on the host and returns
 *   LBVH_OK in both cases: the caller reads d_offsets[count] (one 8-byte download) to learn what was needed.
 *   Count-only form: capacity == 0 writes the offsets in one walk (d_segments may be NULL); otherwise the tasks are walked twice.
 *   d_segments == NULL with capacity > 0 is LBVH_ERR_INVALID_ARG.
 * Needs the derived traversal scene (lbvh_build_fast_scene; a stale one is LBVH_ERR_INVALID_ARG), is asynchronous on the context's
 * stream with no host wait, and uses the context's ray scratch and lbvh_region_overlaps_large's task scratch: it drops the path
 * tracer's live-path list (see lbvh_path_bounce).  A failed scratch allocation is LBVH_ERR_OUT_OF_MEMORY and leaves the context
 * usable.  count == 0 is a no-op: nothing is enqueued and no buffer is touched, d_offsets[0] included.  Rejected
 * (LBVH_ERR_INVALID_ARG, the message names this entry point): NULL ctx / d_planes / h_scene / d_offsets, d_planes or d_segments
 * not 16-byte aligned, d_offsets not 8-byte aligned, count > LBVH_PLANE_SECTIONS_MAX_COUNT.  lbvh_debug_region_task_cap,
 * lbvh_debug_ray_waves, lbvh_debug_ray_stack_split and lbvh_debug_ray_stack_limit apply to the task walks;
 * lbvh_ray_stats_target: rays counts the tasks that are not empty, node_fetches the node lines of the task walks plus the nodes
 * the expansion opened, triangle_tests the triangle lines read; the full form adds the walks' share twice.
 * Measurements: tools/plane_sections_bench.py (written, not yet recorded).
 * Out of scope: a per-lane form for more than 65 536 planes; an _any form; a device-side sort of 32-byte segments; merging records
 * into polylines on the device (host.stitch_sections does it on the host); coplanar faces.  (Out of scope of THIS call: the
 * device-side sort of these 32-byte segments by `tri` is lbvh_sort_record_segments with LBVH_SORT_RECORDS_BY_TRI, above.) */
#define LBVH_PLANE_SECTIONS_MAX_COUNT 65536
lbvh_status lbvh_plane_sections(lbvh_context* ctx, const lbvh_plane* d_planes, size_t count, const lbvh_scene* h_scene,
                                uint64_t* d_offsets, lbvh_plane_segment* d_segments, uint64_t capacity);

/* Camera rays into path states (origin/dir as Raytracing.compute:108-126, throughput 1, radiance 0, alive). */
lbvh_status lbvh_path_begin(lbvh_context* ctx, const lbvh_camera* h_camera, lbvh_path_state* d_states);

/* One bounce for every live path given its hit record: a miss adds throughput * sky(dir) and ends the path
 * (sky = (1 - s) * (1,1,1) + s * (0.5,0.7,1), s = 0.5 * (dir.y + 1)); a hit multiplies the throughput by
 * `albedo`, moves the origin to the hit point and draws a cosine-weighted direction about the geometric
 * normal (flipped toward the incoming ray): normalize(n + p) with p uniform on the unit sphere by
 * Marsaglia's rejection method, random numbers = PCG hash of (seed, path index, bounce, draw).  `bounce` = 0
 * for the primary hit (it also sets alpha). */
lbvh_status lbvh_path_scatter(lbvh_context* ctx, const lbvh_scene* h_scene, const lbvh_hit* d_hits, size_t count,
                              uint32_t bounce, uint32_t seed, float albedo, lbvh_path_state* d_states);

/* lbvh_path_scatter for bounce `bounce` followed by lbvh_trace_rays for the next segment of the paths that go on,
 * as one call: the scatter kernel itself lists those paths, so no pass over all path states is needed before the
 * trace.  d_hits holds the hit records of the segment just traced on entry and those of the next segment on
 * return.  The record of a path that ends in this call (it ends on a miss) becomes {t = MAX_FLOAT, triangle =
 * 0xFFFFFFFF, 0, 0} — still a miss to every reader; a later lbvh_path_bounce (bounce > 0) on the same buffers recognises
 * it and skips the finished path without reading its 64-byte state.  At bounce 0 every record is the caller's: one that
 * was pre-filled with 0xFFFFFFFF words and never traced is an ordinary miss (sky term, path ends), as in
 * lbvh_path_scatter.  States, radiance and image: the same as the two calls.
 * CROSS-CALL STATE: a call with bounce >= 1 — and the frame's last lbvh_path_scatter — visits only the paths the previous
 * lbvh_path_bounce on the same d_states / d_hits listed as live (a list kept by the context).  Every library call that writes
 * into those buffers drops the list (lbvh_path_begin, lbvh_trace_rays, a primary trace into any part of d_hits,
 * lbvh_buffer_upload / _fill_u32 / _free), and so does lbvh_trace_forget — and so do lbvh_trace_closest,
 * lbvh_trace_occluded, lbvh_closest_point_query, lbvh_within_distance, lbvh_count_hits, lbvh_point_crossings, lbvh_box_overlaps, lbvh_gather_within_distance, lbvh_k_closest_points, lbvh_trace_k_closest, lbvh_gather_hits, lbvh_sphere_cast, lbvh_sphere_cast_any, lbvh_capsule_cast, lbvh_capsule_cast_any, lbvh_box_cast, lbvh_box_cast_any, lbvh_triangle_cast, lbvh_triangle_cast_any, lbvh_triangle_intersections, lbvh_triangle_intersects_any, lbvh_triangle_intersection_segments, lbvh_capsule_overlaps, lbvh_capsule_overlaps_any, lbvh_obb_overlaps, lbvh_obb_overlaps_any, lbvh_capsule_contacts, lbvh_capsule_deepest, lbvh_obb_contacts, lbvh_obb_deepest, lbvh_segment_closest_point, lbvh_segment_within_distance, lbvh_triangle_closest_point, lbvh_triangle_within_distance, lbvh_triangle_gather_within_distance, lbvh_sphere_cast_all, lbvh_capsule_cast_all, lbvh_box_cast_all, lbvh_triangle_cast_all, lbvh_region_overlaps, lbvh_region_overlaps_any, lbvh_region_overlaps_large and lbvh_plane_sections, whatever buffers they are given, since they use the same ray scratch; then every state is scanned again.  The one exception among the query calls:
 * lbvh_sort_hit_segments, lbvh_sort_index_segments and lbvh_sort_record_segments take no context scratch and keep the live-path list (they drop it only when the
 * buffer they sort is d_hits itself).  What the library
 * cannot see is a write of the CALLER's own (a kernel or hipMemcpy that revives or ends paths, Russian roulette): between two
 * consecutive bounces of a frame d_states and d_hits must not be written from outside the library — or lbvh_trace_forget must be
 * called after such a write. */
lbvh_status lbvh_path_bounce(lbvh_context* ctx, const lbvh_scene* h_scene, lbvh_path_state* d_states, lbvh_hit* d_hits,
                             size_t count, uint32_t bounce, uint32_t seed, float albedo, float t_min);

/* lbvh_path_begin + lbvh_path_bounce(bounce = 0) as one call: d_hits holds the primary hit records of the camera's
 * W x H frame (lbvh_trace_primary); every pixel's path state is MADE from the camera on the fly — never stored by one
 * kernel to be loaded by the next (132 MB each way at 1080p) — scattered at its hit, and the first secondary segment is
 * traced.  States, hit records and the image: identical to the two calls. */
lbvh_status lbvh_path_first_bounce(lbvh_context* ctx, const lbvh_camera* h_camera, const lbvh_scene* h_scene, lbvh_path_state* d_states,
                                   lbvh_hit* d_hits, uint32_t seed, float albedo, float t_min);

/* radiance (+ alpha) of the path states as RGBA16F, the reference's render-target format. */
lbvh_status lbvh_path_resolve(lbvh_context* ctx, const lbvh_path_state* d_states, size_t count, uint16_t* d_rgba16f);

/* LBVH_TRACE_FAST dispatches a frame's tiles in the order of their step counts in the PREVIOUS trace of the same frame
 * layout (a scheduling hint kept by the context; any order gives the same hits).  When the camera differs from that
 * trace's, a tile takes the count of the place it came from: the ray through its centre, at the distance of the scene
 * box's centre, projected with the previous camera (exact for a turn of the camera), widened by one tile.  This call
 * drops the history: the next trace runs as a first frame does (row-major).  For measuring cold frames.  It also drops the path
 * tracer's live-path list (lbvh_path_bounce): the next bounce scans every path state. */
lbvh_status lbvh_trace_forget(lbvh_context* ctx);

/* Multi-GPU frames (one context per GPU, each tracing its lbvh_trace_primary_shard share): the dispatch hint above comes
 * from the context's OWN last trace, and under a moving camera the place a tile came from mostly belongs to another
 * rank.  lbvh_trace_costs_export writes this context's per-tile step counts of its last LBVH_TRACE_FAST trace into a
 * full-frame array (one u32 per 8x8-pixel tile, row-major, ceil(W/8) x ceil(H/8); tiles of other shards are left as they
 * are — hand in a zeroed array); the ranks merge their arrays (an all-reduce MAX or SUM of 130 KB at 1080p, e.g. while
 * the next rebuild runs) and give the result back with lbvh_trace_costs_import (copied).  The next trace with a DIFFERENT
 * camera takes its tiles' costs from there — once: a map is a hint for the frame that follows it, not for later ones.  A hint only: hits do
 * not depend on it.  Both calls are asynchronous on the context's stream. */
lbvh_status lbvh_trace_costs_export(lbvh_context* ctx, uint32_t* d_frame_costs, uint32_t tiles_x, uint32_t tiles_y);
lbvh_status lbvh_trace_costs_import(lbvh_context* ctx, const uint32_t* d_frame_costs, uint32_t tiles_x, uint32_t tiles_y);

/* ---- measurement helpers (HIP events on the context's stream) --------------------------------- */

lbvh_status lbvh_event_create(lbvh_context* ctx, void** out_event);
lbvh_status lbvh_event_destroy(lbvh_context* ctx, void* event);
lbvh_status lbvh_event_record(lbvh_context* ctx, void* event);
/* Waits for `stop`, then returns the elapsed milliseconds between the two recorded events. */
lbvh_status lbvh_event_elapsed_ms(lbvh_context* ctx, void* start, void* stop, float* out_ms);

#ifdef __cplusplus
}
#endif
#endif /* LBVH_H */
