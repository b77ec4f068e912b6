// lbvh_driver.cpp — BASELINE config 1 ("plumbing") through the C++ host classes: 4 096 random
// triangles, 256x256 primary rays, the reference's Awake() + Update() call order.  Prints stage
// timings and checksums the parity tests compare with the oracle.  Links only liblbvh.so.
//     lbvh_driver [n] [w] [h] [dynamic]          seeded random triangles (cfg1)
//     lbvh_driver obj <file.obj> [w] [h] [z]     mesh ingest (lbvh_mesh.hpp) -> Awake -> Update, camera at (0, 0, z)
//     lbvh_driver multi <ranks> [n] [w] [h]      one process, <ranks> contexts (MultiGpuDrawer; rank r on device r % device
//                                                count): frames assembled in rank 0's buffer by peer-mapped stores,
//                                                compared word for word with one context's whole frame
//     lbvh_driver sort <ranks> [n] [replicate]   n pairs in uneven blocks over <ranks> contexts sorted by ONE
//                                                lbvh_sort_pairs_sharded call (MultiGpuSorter), compared word for word
//                                                with lbvh_sort_pairs on one context; prints JSON with "equal"
//     lbvh_driver rays [n] [w] [h]               the cfg1 mesh and camera; from every primary hit a shadow ray toward the
//                                                light (0, 250, 150): dir = light - hit point (not normalised), t in
//                                                (1e-4, 1); pixels without a hit give inactive rays.  TraceClosest with
//                                                t_max = 1 and = +inf, TraceOccluded; prints the hit count and t sum of the
//                                                first, the occluded count and whether occluded == (t(+inf) < 1) on every ray
//     lbvh_driver points [n | file.obj] [count] [radius]   the cfg1 mesh of n triangles (or an OBJ asset); `count` points (SplitMix64,
//                                                seed 2) uniform in the box of the vertices grown by a quarter of its extent per
//                                                side, max_dist2 = radius * radius (default: unbounded).  ClosestPoints and
//                                                WithinDistance; prints how many points found a triangle, the sum of all 32-bit
//                                                words of the records (mod 2^64) and the number of set flags
//     lbvh_driver knn <k> [n | file.obj] [count] [radius]   the mesh and the points of `points`; KClosestPoints with k records per
//                                                point; prints the sum of the found counts, how many rows are full, the sum of all
//                                                32-bit words of the count * k records (mod 2^64) and the first rows
//     lbvh_driver khits <k> <n> <count> [t_max]  n random triangles and `count` rays from points around the mesh's box towards
//                                                points inside it (t = 1 at the target, t_max default unbounded); TraceKClosest
//                                                with k records per ray; prints the sum of the found counts, how many rows are
//                                                full, the sum of all 32-bit words of the count * k records (mod 2^64) and the
//                                                first rows
//     lbvh_driver gather <n_rays> [t_max]        the 4 096 triangles and the rays of `khits`; GatherHits twice (count only, one
//                                                8-byte read, fill); every segment sorted by (t, tri) on the host; prints the total,
//                                                how many segments are non-empty, the sum of all 32-bit words of the records (mod
//                                                2^64), the sum of (position + 1) * triangle index over the sorted list (mod 2^64) and
//                                                the first segments
//     lbvh_driver sortedhits <n_rays> [t_max]    `gather` with the segments ordered on the device instead: GatherHits, then
//                                                SortHitSegments, then the download; no host sort; prints the same fields, the
//                                                position-weighted sum now over the device-sorted order
//     lbvh_driver sortedrecords <contacts|boxcontacts|triprox|trisegs|sections> <n> [seed]   a synthetic CSR list of n segments of
//                                                32-byte records (SplitMix64: lengths 0 .. 23, every 97th 300 .. 2 299; word 0 a
//                                                multiple of 0.25, words 1 and 3 distinct inside a segment), SortRecordSegments in
//                                                the order of that list (deepest first / nearest first / by triangle); prints the
//                                                total, the sum of all words and the sum of (position + 1) * (word 1 ^ word 7)
//     lbvh_driver sweep [n | file.obj] [count] [radius]  the mesh of `points` and `count` spheres of the given radius (default 1 %
//                                                of the largest extent) from points around the mesh's box towards points inside
//                                                it (t = 1 at the target, t_max 2); SphereCast and SphereCastAny; prints how
//                                                many casts touch, the sum of all 32-bit words of the records (mod 2^64) and the
//                                                first records
//     lbvh_driver capsule <n_casts> [seed] [radius] [height]  the 4 096 triangles of cfg1 and n_casts capsules (SplitMix64, seed
//                                                default 3; radius default 1.5, height default 4): per axis the origin and the
//                                                target as `sweep` draws them, then the axis component uniform in [-height,
//                                                height]; t_max 2.  CapsuleCast and CapsuleCastAny; prints the fields of `sweep`
//     lbvh_driver boxcast [seed] [half_extent] [t_max] [n_casts]  the 4 096 triangles of cfg1 and n_casts (default 6 000) boxes
//                                                (SplitMix64, seed default 3; half_extent default 1.5, t_max default 2): per
//                                                axis k the centre and the target as `sweep` draws them, then component k of
//                                                ax, ay, az: half_extent on the diagonal, 0 off it, plus uniform in
//                                                [-half_extent / 2, half_extent / 2] (sheared, always solid).  BoxCast and
//                                                BoxCastAny; prints how many casts touch, how many overlap at the start, the
//                                                number of records per axis, the word sum and the first records
//     lbvh_driver castall <sphere|capsule|box|triangle> <n_casts> [seed] [t_max]  the 4 096 triangles of cfg1 and n_casts sweeps (seed default 3,
//                                                t_max default 2): spheres of radius 1.5 drawn as `sweep` draws them, the capsules of
//                                                `capsule` (radius 1.5, height 4), the boxes of `boxcast` (half_extent 1.5) or the
//                                                moving triangles of `tricast` (castall triangle <n> [seed] [t_max]).  The
//                                                shape's CastAll (count only, one 8-byte read, fill), SortHitSegments, then the
//                                                first-contact and the any-contact call on the same casts; prints the total, how many
//                                                segments are non-empty, how many flags are set, for how many casts the first record of
//                                                the sorted segment is the first-contact record word for word (the miss record for an
//                                                empty one), the longest segment, how many records have t = 0, the word sum, the sum
//                                                of (position + 1) * triangle index over the device-sorted list and the first segments
//     lbvh_driver crossings [n | file.obj] [count] the mesh and the points of `points`; PointCrossings along the three default
//                                                directions ((1,1,1)/sqrt 3, (-1,2,3)/sqrt 14, (4,-1,2)/sqrt 21) and CountHits
//                                                on the same rays written out ({p, 0, dir, +inf}); prints the sum of the counts,
//                                                the sum of the parity words, how many points the majority calls inside and
//                                                whether every parity bit equals its ray's count AND 1
//     lbvh_driver tris <n_queries> [seed]        the 4 096 triangles of cfg1 and n_queries query triangles (SplitMix64, seed default 5):
//                                                per axis a centre uniform in the mesh's box, then b's and c's offsets uniform in
//                                                [-3, 3].  TriangleIntersections (count only, one 8-byte read, fill),
//                                                SortIndexSegments, TriangleIntersectsAny; prints the total, how many segments are
//                                                non-empty, how many flags are set, the sum of (position + 1) * triangle index over
//                                                the device-sorted list (mod 2^64) and the first segments
//     lbvh_driver tricast <n> [seed] [t_max]     the 4 096 triangles of cfg1 and n moving triangles (default 6 000; SplitMix64, seed
//                                                default 5; t_max default 2): per axis the vertex a as `sweep` draws an origin, b's and
//                                                c's offsets uniform in [-3, 3], then dir = a target in the mesh's box minus a.
//                                                TriangleCast and TriangleCastAny; prints how many casts touch, how many start in
//                                                overlap, the number of records per feature, the word sum and the first records
//     lbvh_driver trisegs <n_queries> [seed]     the mesh and the queries of `tris`; TriangleIntersectionSegments (count only, one
//                                                8-byte read, fill), every segment sorted by tri on the host; prints the total, how
//                                                many segments are non-empty, how many records have two different ends, the sum of
//                                                (k + 1) * offsets[k] and the sum of (position + 1) * (the record's eight words) over
//                                                the sorted list (both mod 2^64)
//     lbvh_driver shapes <n_shapes> [seed]       the 4 096 triangles of cfg1 and n_shapes capsules and as many boxes (SplitMix64, seed
//                                                default 7): per shape and axis k the capsule's origin uniform in the mesh's box and
//                                                its axis component uniform in [-6, 6] (radius 3), then the box's centre uniform in
//                                                the mesh's box and component k of ax, ay, az: 3 on the diagonal, 0 off it, plus
//                                                uniform in [-1.5, 1.5].  CapsuleOverlaps / ObbOverlaps (count only, one 8-byte read,
//                                                fill), SortIndexSegments, CapsuleOverlapsAny / ObbOverlapsAny; prints per family what
//                                                `tris` prints
//     lbvh_driver contacts <n_shapes> [seed]     the same mesh and n_shapes capsules (SplitMix64, seed default 11): per capsule and
//                                                axis k the origin uniform in the mesh's box and the axis component uniform in [-6, 6]
//                                                (radius 3).  CapsuleContacts (count only, one 8-byte read, fill) and CapsuleDeepest;
//                                                prints the total, how many segments are non-empty, how many capsules touch, the
//                                                order-free sum of the records' words, the same of the deepest records weighted by
//                                                shape, and the first deepest records as words
//     lbvh_driver segclosest <n_segments> [seed] the same mesh and n_segments segments (SplitMix64, seed default 15): per segment and
//                                                axis k the origin uniform in the mesh's box and the axis component uniform in [-6, 6];
//                                                max_dist2 = 9 for the even ones, +inf for the odd ones.  SegmentClosestPoints and
//                                                SegmentWithinDistance; prints how many have a record, how many flags are set, the sum
//                                                of the records' words weighted by word and segment, and the first records as words
//     lbvh_driver triclosest <n_queries> [seed]  the same mesh and n_queries query triangles (SplitMix64, seed default 21) drawn as
//                                                `tris` draws its own; max_dist2 = 4 for the even ones, +inf for the odd ones.
//                                                TriangleClosestPoints and TriangleWithinDistance; prints how many have a record, how
//                                                many flags are set, how many records are pierced, the sum of the records' words
//                                                weighted by word and query, and the first records as words
//     lbvh_driver triprox <n_queries> [seed]     the same mesh and the query triangles of `triclosest` (the same draws, seed default
//                                                21), every max_dist2 = 4: nothing is unbounded.  TriangleGatherWithinDistance (count
//                                                only, one 8-byte read, fill); prints the total, how many segments are non-empty, the
//                                                longest segment, how many records are pierced, and the sum of the records' words
//                                                weighted by word and by the record's position after sorting each segment by tri
//     lbvh_driver boxcontacts <n_shapes> [seed]  the same mesh and n_shapes sheared boxes (SplitMix64, seed default 13): per box and axis
//                                                k the centre uniform in the mesh's box, then component k of ax, ay, az as `shapes`
//                                                draws them.  ObbContacts (count only, one 8-byte read, fill) and ObbDeepest; prints
//                                                what `contacts` prints
//     lbvh_driver regions <n_regions> [seed] [large]  the 4 096 triangles of cfg1 and n_regions sheared boxes (SplitMix64, seed default 6):
//                                                the centre uniform in the mesh's box, then per axis k a normal — the axis' unit
//                                                vector with its two other components uniform in [-0.5, 0.5] — and a half width
//                                                uniform in [1, 12]: the planes {n, h - n . c} and {-n, h + n . c}.  RegionOverlaps
//                                                (count only, one 8-byte read, fill) in both modes, SortIndexSegments,
//                                                RegionOverlapsAny; prints per mode the total, how many segments are non-empty, how
//                                                many flags are set and the sum of (position + 1) * triangle index over the
//                                                device-sorted list (mod 2^64), and the first TOUCHING segments.  With `large` after
//                                                the seed the lists come from RegionOverlapsLarge (n_regions <= 65 536): the same
//                                                numbers, and "large": true in the output
//     lbvh_driver sections <n_planes> [seed]     the 4 096 triangles of cfg1 and n_planes planes (SplitMix64, seed default 7): per plane
//                                                and axis k the normal's component uniform in [-1, 1], then a point's coordinate
//                                                uniform in the mesh's box; d = -((nx * px + ny * py) + nz * pz) in fp32.
//                                                PlaneSections (count only, one 8-byte read, fill), every segment sorted by tri on the
//                                                host; prints the total, how many segments are non-empty, the sum of (k + 1) *
//                                                offsets[k] and the sum of (position + 1) * (the record's eight words) over the sorted
//                                                list (both mod 2^64)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "lbvh_host.hpp"
#include "lbvh_mesh.hpp"

static uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float uniform(uint64_t& s, float lo, float hi) { return lo + (hi - lo) * (float)((splitmix64(s) >> 40) * (1.0 / 16777216.0)); }

// doubled: every second triangle is a copy of the one before it — every hit on one is an exact t tie with the other
static std::vector<lbvh_triangle> random_mesh(uint32_t n, bool doubled = false)
{
    std::vector<lbvh_triangle> mesh(n);
    uint64_t seed = 1;
    for (auto& t : mesh) {
        if (doubled && ((&t - mesh.data()) & 1)) { t = *(&t - 1); continue; }
        std::memset(&t, 0, sizeof t);
        for (int k = 0; k < 3; k++) {
            const float c = uniform(seed, -100.0f, 100.0f);
            t.a[k] = c;
            t.b[k] = c + uniform(seed, -2.0f, 2.0f);
            t.c[k] = c + uniform(seed, -2.0f, 2.0f);
        }
        t.b_uv[0] = 1.0f; t.c_uv[1] = 1.0f;
    }
    return mesh;
}

static lbvh_camera camera_at(int w, int h, float z, float yaw_deg = 0.0f)
{
    lbvh_camera cam;
    cam.screen_width = w; cam.screen_height = h;
    cam.camera_fov = (float)std::tan(60.0 * 3.14159265358979323846 / 180.0 / 2.0);   // Mathf.Tan(fov * Deg2Rad / 2)
    cam.near_plane = 0.3f;
    const float c = (float)std::cos(yaw_deg * 3.14159265358979323846 / 180.0), s = (float)std::sin(yaw_deg * 3.14159265358979323846 / 180.0);
    const float m[16] = {-c, 0, s, 0, 0, 1, 0, 0, s, 0, c, z, 0, 0, 0, 1};
    std::memcpy(cam.camera_to_world, m, sizeof m);
    return cam;
}

// the mesh argument of the query sub-commands: a triangle count (the cfg1 mesh) or an OBJ asset (MeshBufferContainer.cs:117-146)
static std::vector<lbvh_triangle> load_mesh(const char* what)
{
    const size_t len = std::strlen(what);
    const bool from_obj = len > 4 && std::strcmp(what + len - 4, ".obj") == 0;
    return from_obj ? lbvh::MeshTriangles(lbvh::LoadObj(what)) : random_mesh((uint32_t)atoi(what));
}

// the box of the vertices
static void mesh_box(const std::vector<lbvh_triangle>& mesh, float lo[3], float hi[3])
{
    for (int k = 0; k < 3; k++) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (const auto& t : mesh)
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(lo[k], std::fmin(t.a[k], std::fmin(t.b[k], t.c[k])));
            hi[k] = std::fmax(hi[k], std::fmax(t.a[k], std::fmax(t.b[k], t.c[k])));
        }
}

// points uniform in the box grown by a quarter of its extent per side, every one with the same max_dist2; draws axis by axis
static void points_around(const float lo[3], const float hi[3], uint64_t seed, float max_dist2, std::vector<lbvh_point_query>& points)
{
    for (auto& q : points) {
        for (int k = 0; k < 3; k++) {
            const float grow = 0.25f * (hi[k] - lo[k]);
            q.p[k] = uniform(seed, lo[k] - grow, hi[k] + grow);
        }
        q.max_dist2 = max_dist2;
    }
}

// origin and dir of lbvh_ray or lbvh_sphere_ray records: from points around the box (as points_around) towards points inside it,
// t = 1 at the target; per axis the origin is drawn before the target.  The fourth float of each half is the caller's
template <class Ray>
static void rays_into(const float lo[3], const float hi[3], uint64_t seed, std::vector<Ray>& rays)
{
    for (auto& r : rays)
        for (int k = 0; k < 3; k++) {
            const float grow = 0.25f * (hi[k] - lo[k]);
            r.origin[k] = uniform(seed, lo[k] - grow, hi[k] + grow);
            r.dir[k] = uniform(seed, lo[k], hi[k]) - r.origin[k];
        }
}

// the sum of the four 32-bit words of a 16-byte record (lbvh_hit, lbvh_closest_point)
template <class Record>
static uint64_t word_sum(const Record& record)
{
    static_assert(sizeof(Record) == 16, "four words");
    uint32_t w[4];
    std::memcpy(w, &record, sizeof w);
    return (uint64_t)w[0] + w[1] + w[2] + w[3];
}

// BASELINE configs[2] through the one-process host: every frame of every camera / mode assembled from <ranks> shares must
// equal the frame one context traces alone, the assembled buffer poisoned before each frame
static int multi_main(int argc, char** argv)
{
    const int ranks = argc > 2 ? atoi(argv[2]) : 2;
    const uint32_t n = argc > 3 ? (uint32_t)atoi(argv[3]) : 4096;
    const int w = argc > 4 ? atoi(argv[4]) : 256, h = argc > 5 ? atoi(argv[5]) : 256;
    // "doubled": a scene full of exact t ties — LBVH_TRACE_FAST_EXACT's tie resolution then runs on EVERY rank against the owner's
    // frame (system-scope loads and compare-and-swaps on peer memory): ADVICE r4
    const bool doubled = argc > 6 && std::strcmp(argv[6], "doubled") == 0;
    const std::vector<lbvh_triangle> mesh = random_mesh(n, doubled);
    const int n_dev = lbvh::Context::device_count();
    if (n_dev <= 0) { std::fprintf(stderr, "no HIP device visible\n"); return 1; }
    std::vector<int> devices;
    for (int r = 0; r < ranks; r++) devices.push_back(r % n_dev);
    lbvh::MultiGpuDrawer multi(devices, mesh);
    multi.Awake();
    lbvh::Context one(0);
    lbvh::RaytracingMeshDrawer single(one, mesh);
    single.Awake();
    int frames = 0, equal = 0;
    size_t hits = 0;
    for (int mode : {LBVH_TRACE_FAST, LBVH_TRACE_REFERENCE, LBVH_TRACE_FAST_EXACT})
        for (int f = 0; f < 4; f++) {
            // two frames from one camera (the second is dispatched by the first one's costs), then a turned one, then a
            // rebuilt scene
            const lbvh_camera cam = camera_at(w, h, 300.0f, f < 2 ? 0.0f : 2.0f * f);
            if (f == 3) { multi.Rebuild(); single.Rebuild(); }
            if (frames) multi.Hits().Fill(0x7FC00000u, false);            // poison: a missing tile cannot pass on old values
            multi.Update(cam, mode);
            single.Update(cam, mode);
            multi.Hits().GetData();                                      // on the owner's stream: behind the device-side gather
            single.Hits().GetData();
            const bool same = std::memcmp(multi.Hits().LocalBuffer().data(), single.Hits().LocalBuffer().data(),
                                          (size_t)w * h * sizeof(lbvh_hit)) == 0;
            frames++;
            equal += same ? 1 : 0;
            if (mode == LBVH_TRACE_FAST_EXACT) {      // ... and the exact mode's frame is the reference mode's, word for word
                // (include/lbvh.h: except at a pixel whose reference winner lies in front of its own triangle's box — this
                // scene and these cameras have none; the general case is checked against the oracle by the Python suite)
                single.Update(cam, LBVH_TRACE_REFERENCE);
                single.Hits().GetData();
                if (std::memcmp(multi.Hits().LocalBuffer().data(), single.Hits().LocalBuffer().data(), (size_t)w * h * sizeof(lbvh_hit)) != 0)
                    equal--;
            }
            if (mode == LBVH_TRACE_REFERENCE && f == 0)
                for (size_t i = 0; i < (size_t)w * h; i++) hits += multi.Hits().LocalBuffer()[i].t < LBVH_MAX_FLOAT ? 1 : 0;
        }
    multi.Sync();
    std::printf("{\"ranks\": %d, \"devices\": %d, \"triangles\": %u, \"rays\": %d, \"frames\": %d, \"frames_equal\": %d, \"hits\": %zu}\n",
                ranks, n_dev, n, w * h, frames, equal, hits);
    return equal == frames ? 0 : 2;
}

// `sort <ranks> <n> [replicate]`: n (key, value) pairs in uneven blocks over `ranks` contexts (devices dealt round-robin; one
// block empty when ranks > 2), sorted by MultiGpuSorter (lbvh_sort_pairs_sharded), compared word for word with lbvh_sort_pairs
// of the whole sequence on one context.  Keys: half uniform, half from eight values (ties across blocks); values: global index.
static int sort_main(int argc, char** argv)
{
    const int ranks = argc > 2 ? atoi(argv[2]) : 2;
    const uint32_t n = argc > 3 ? (uint32_t)strtoul(argv[3], nullptr, 10) : 1000000u;
    const bool replicate = argc > 4 && std::strcmp(argv[4], "replicate") == 0;
    if (ranks < 1 || ranks > LBVH_SORT_SHARDED_MAX_CONTEXTS) { std::fprintf(stderr, "ranks: 1 .. 16\n"); return 1; }
    uint64_t seed = 7;
    std::vector<uint32_t> keys(n), values(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t r = splitmix64(seed);
        keys[i] = (i & 1) ? (uint32_t)(r >> 32) : (uint32_t)(r % 8u) * 0x1F00A5u;
        values[i] = i;
    }
    // uneven blocks: weight r + 1, block 1 empty when ranks > 2
    std::vector<uint64_t> weight(ranks);
    uint64_t wsum = 0;
    for (int r = 0; r < ranks; r++) wsum += weight[r] = (ranks > 2 && r == 1) ? 0 : (uint64_t)r + 1;
    std::vector<std::vector<uint32_t>> bk(ranks), bv(ranks);
    uint64_t lo = 0, acc = 0;
    for (int r = 0; r < ranks; r++) {
        acc += weight[r];
        const uint64_t hi = r == ranks - 1 ? n : n * acc / wsum;
        bk[r].assign(keys.begin() + lo, keys.begin() + hi);
        bv[r].assign(values.begin() + lo, values.begin() + hi);
        lo = hi;
    }
    const int n_dev = lbvh::Context::device_count();
    if (n_dev <= 0) { std::fprintf(stderr, "no HIP device visible\n"); return 1; }
    std::vector<int> devices;
    for (int r = 0; r < ranks; r++) devices.push_back(r % n_dev);
    lbvh::MultiGpuSorter sorter(devices);
    sorter.SetBlocks(bk, bv);
    auto t0 = std::chrono::steady_clock::now();
    const std::vector<uint32_t> counts = sorter.Sort(replicate);
    sorter.Sync();
    const double sharded_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // the one-context sort of the whole sequence
    lbvh::Context one(0);
    lbvh::DataBuffer<uint32_t> k1(one, n ? n : 1), v1(one, n ? n : 1);
    std::copy(keys.begin(), keys.end(), k1.LocalBuffer().begin());
    std::copy(values.begin(), values.end(), v1.LocalBuffer().begin());
    k1.Sync(); v1.Sync();
    lbvh::check(one.get(), lbvh_sort_pairs(one.get(), (uint32_t*)k1.DeviceBuffer(), (uint32_t*)v1.DeviceBuffer(), n));
    k1.GetData(); v1.GetData();
    bool equal = true;
    uint64_t at = 0;
    for (int q = 0; q < ranks; q++) {
        sorter.OutKeys(q).GetData();
        sorter.OutValues(q).GetData();
        const uint64_t from = replicate ? 0 : at, len = replicate ? n : counts[q];
        equal = equal && std::memcmp(sorter.OutKeys(q).LocalBuffer().data(), k1.LocalBuffer().data() + from, len * 4) == 0 &&
                std::memcmp(sorter.OutValues(q).LocalBuffer().data(), v1.LocalBuffer().data() + from, len * 4) == 0;
        at += counts[q];
    }
    equal = equal && at == n;
    std::printf("{\"ranks\": %d, \"devices\": %d, \"pairs\": %u, \"replicate\": %s, \"slice_counts\": [", ranks, n_dev, n,
                replicate ? "true" : "false");
    for (int q = 0; q < ranks; q++) std::printf("%s%u", q ? ", " : "", counts[q]);
    std::printf("], \"host_ms\": %.3f, \"equal\": %s}\n", sharded_ms, equal ? "true" : "false");
    return equal ? 0 : 2;
}

static int rays_main(int argc, char** argv)
{
    const uint32_t n = argc > 2 ? (uint32_t)atoi(argv[2]) : 4096;
    const int w = argc > 3 ? atoi(argv[3]) : 256, h = argc > 4 ? atoi(argv[4]) : 256;
    const size_t count = (size_t)w * h;
    const float light[3] = {0.0f, 250.0f, 150.0f};
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, random_mesh(n));
    drawer.Awake();
    const lbvh_camera cam = camera_at(w, h, 300.0f);
    drawer.Update(cam, LBVH_TRACE_FAST);
    lbvh::DataBuffer<lbvh_path_state> primary(ctx, count);          // the camera rays, as the primary trace made them
    lbvh::check(ctx.get(), lbvh_path_begin(ctx.get(), &cam, (lbvh_path_state*)primary.DeviceBuffer()));
    primary.GetData();
    drawer.Hits().GetData();
    lbvh::DataBuffer<lbvh_ray> rays(ctx, count);
    for (size_t i = 0; i < count; i++) {
        const lbvh_path_state& p = primary.LocalBuffer()[i];
        const float t = drawer.Hits().LocalBuffer()[i].t;
        lbvh_ray& r = rays.LocalBuffer()[i];
        std::memset(&r, 0, sizeof r);                                 // t_min = t_max = 0: inactive
        if (!(t < LBVH_MAX_FLOAT)) continue;
        for (int k = 0; k < 3; k++) {
            r.origin[k] = p.origin[k] + p.dir[k] * t;
            r.dir[k] = light[k] - r.origin[k];
        }
        r.t_min = 1e-4f;
        r.t_max = 1.0f;
    }
    rays.Sync();
    lbvh::DataBuffer<lbvh_hit> closest(ctx, count), unbounded(ctx, count);
    lbvh::DataBuffer<uint32_t> occluded(ctx, count);
    drawer.TraceClosest(rays, closest);
    drawer.TraceOccluded(rays, occluded);
    for (auto& r : rays.LocalBuffer())
        if (r.t_max > 0.0f) r.t_max = INFINITY;
    rays.Sync();
    drawer.TraceClosest(rays, unbounded);
    closest.GetData();
    unbounded.GetData();
    occluded.GetData();
    size_t hits = 0, n_occluded = 0;
    double tsum = 0;
    bool e3 = true;
    for (size_t i = 0; i < count; i++) {
        const lbvh_hit& c = closest.LocalBuffer()[i];
        if (c.t < LBVH_MAX_FLOAT) { hits++; tsum += c.t; }
        const uint32_t o = occluded.LocalBuffer()[i];
        n_occluded += o;
        const bool active = rays.LocalBuffer()[i].t_max > 0.0f;
        e3 = e3 && o == (uint32_t)(active && unbounded.LocalBuffer()[i].t < 1.0f);
    }
    std::printf("{\"triangles\": %u, \"rays\": %zu, \"hits\": %zu, \"t_sum\": %.6f, \"occluded\": %zu, \"e3_holds\": %s}\n", n, count,
                hits, tsum, n_occluded, e3 ? "true" : "false");
    return 0;
}

static int points_main(int argc, char** argv)
{
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 65536;
    const float radius = argc > 4 ? (float)atof(argv[4]) : INFINITY;
    const std::vector<lbvh_triangle> mesh = load_mesh(argc > 2 ? argv[2] : "4096");
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_point_query> queries(ctx, count);
    points_around(lo, hi, 2, radius * radius, queries.LocalBuffer());
    queries.Sync();
    lbvh::DataBuffer<lbvh_closest_point> closest(ctx, count);
    lbvh::DataBuffer<uint32_t> within(ctx, count);
    drawer.ClosestPoints(queries, closest);
    drawer.WithinDistance(queries, within);
    closest.GetData();
    within.GetData();
    size_t found = 0, n_within = 0;
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        const lbvh_closest_point& c = closest.LocalBuffer()[i];
        if (c.dist2 < LBVH_MAX_FLOAT) found++;
        words += word_sum(c);
        n_within += within.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"points\": %zu, \"found\": %zu, \"word_sum\": %llu, \"within\": %zu}\n", mesh.size(), count, found,
                (unsigned long long)words, n_within);
    return 0;
}

static float first_of(const lbvh_closest_point& c) { return c.dist2; }
static float first_of(const lbvh_hit& h) { return h.t; }

// what knn and khits print of their count * k records: the sum of the found counts, how many rows are full, the word sum and the
// first rows as [dist2 or t, tri] pairs.  Record: lbvh_closest_point or lbvh_hit (the same 16-byte shape)
template <class Record>
static void print_rows(const char* queries, size_t triangles, size_t count, uint32_t k, const std::vector<Record>& rows,
                       const std::vector<uint32_t>& found)
{
    size_t found_sum = 0, full = 0;
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        found_sum += found[i];
        full += found[i] == k;
    }
    for (const Record& c : rows) words += word_sum(c);
    std::printf("{\"triangles\": %zu, \"%s\": %zu, \"k\": %u, \"found_sum\": %zu, \"full_rows\": %zu, \"word_sum\": %llu, \"rows\": [",
                triangles, queries, count, k, found_sum, full, (unsigned long long)words);
    for (size_t i = 0; i < std::min<size_t>(count, 3); i++) {
        std::printf("%s[", i ? ", " : "");
        for (uint32_t j = 0; j < found[i]; j++) std::printf("%s[%.9g, %u]", j ? ", " : "", first_of(rows[i * k + j]), rows[i * k + j].tri);
        std::printf("]");
    }
    std::printf("]}\n");
}

static int knn_main(int argc, char** argv)
{
    const uint32_t k = argc > 2 ? (uint32_t)atoi(argv[2]) : 8;
    const size_t count = argc > 4 ? (size_t)strtoull(argv[4], nullptr, 10) : 65536;
    const float radius = argc > 5 ? (float)atof(argv[5]) : INFINITY;
    const std::vector<lbvh_triangle> mesh = load_mesh(argc > 3 ? argv[3] : "4096");
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_point_query> queries(ctx, count);
    points_around(lo, hi, 2, radius * radius, queries.LocalBuffer());
    queries.Sync();
    lbvh::DataBuffer<lbvh_closest_point> rows(ctx, count * (size_t)k);
    lbvh::DataBuffer<uint32_t> found(ctx, count);
    drawer.KClosestPoints(queries, k, rows, &found);
    rows.GetData();
    found.GetData();
    print_rows("points", mesh.size(), count, k, rows.LocalBuffer(), found.LocalBuffer());
    return 0;
}

static int khits_main(int argc, char** argv)
{
    const uint32_t k = argc > 2 ? (uint32_t)atoi(argv[2]) : 8;
    const uint32_t n = argc > 3 ? (uint32_t)atoi(argv[3]) : 4096;
    const size_t count = argc > 4 ? (size_t)strtoull(argv[4], nullptr, 10) : 65536;
    const float t_max = argc > 5 ? (float)atof(argv[5]) : INFINITY;
    const std::vector<lbvh_triangle> mesh = random_mesh(n);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_ray> rays(ctx, count);
    rays_into(lo, hi, 3, rays.LocalBuffer());
    for (auto& r : rays.LocalBuffer()) { r.t_min = 0.0f; r.t_max = t_max; }
    rays.Sync();
    lbvh::DataBuffer<lbvh_hit> rows(ctx, count * (size_t)k);
    lbvh::DataBuffer<uint32_t> found(ctx, count);
    drawer.TraceKClosest(rays, k, rows, &found);
    rows.GetData();
    found.GetData();
    print_rows("rays", mesh.size(), count, k, rows.LocalBuffer(), found.LocalBuffer());
    return 0;
}

// `gather` and `sortedhits`: the same list, ordered by (t, tri) on the host / by lbvh_sort_hit_segments on the device
static int gather_run(int argc, char** argv, bool device_sort)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    const float t_max = argc > 3 ? (float)atof(argv[3]) : INFINITY;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_ray> rays(ctx, count);
    rays_into(lo, hi, 3, rays.LocalBuffer());
    for (auto& r : rays.LocalBuffer()) { r.t_min = 0.0f; r.t_max = t_max; }
    rays.Sync();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    drawer.GatherHits(rays, offsets);                       // count only
    offsets.GetData();
    const uint64_t total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<lbvh_hit> hits(ctx, std::max<size_t>((size_t)total, 1));
    drawer.GatherHits(rays, offsets, &hits);
    if (device_sort) drawer.SortHitSegments(offsets, hits, count);
    offsets.GetData();
    hits.GetData();
    const std::vector<uint64_t>& off = offsets.LocalBuffer();
    std::vector<lbvh_hit>& rec = hits.LocalBuffer();
    size_t nonempty = 0;
    for (size_t q = 0; q < count; q++) {                    // the gather promises no order inside a segment: (t, tri) here
        if (!device_sort)
            std::sort(rec.begin() + off[q], rec.begin() + off[q + 1],
                      [](const lbvh_hit& x, const lbvh_hit& y) { return x.t < y.t || (x.t == y.t && x.tri < y.tri); });
        nonempty += off[q + 1] > off[q];
    }
    uint64_t words = 0, weighted_sum = 0;
    for (uint64_t i = 0; i < total; i++) {
        words += word_sum(rec[i]);
        weighted_sum += (i + 1) * (uint64_t)rec[i].tri;
    }
    std::printf("{\"triangles\": %zu, \"rays\": %zu, \"total\": %llu, \"nonempty\": %zu, \"word_sum\": %llu, \"weighted_sum\": %llu, \"rows\": [",
                mesh.size(), count, (unsigned long long)off[count], nonempty, (unsigned long long)words, (unsigned long long)weighted_sum);
    for (size_t q = 0; q < std::min<size_t>(count, 3); q++) {
        std::printf("%s[", q ? ", " : "");
        for (uint64_t j = off[q]; j < off[q + 1]; j++) std::printf("%s[%.9g, %u]", j != off[q] ? ", " : "", rec[j].t, rec[j].tri);
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

static int gather_main(int argc, char** argv) { return gather_run(argc, argv, false); }
static int sortedhits_main(int argc, char** argv) { return gather_run(argc, argv, true); }

// `sortedrecords`: a synthetic CSR list of 32-byte records, ordered by lbvh_sort_record_segments in the order of the named list
static int sortedrecords_main(int argc, char** argv)
{
    static const struct { const char* kind; uint32_t order; } kinds[] = {
        {"contacts", LBVH_SORT_RECORDS_DESCENDING}, {"boxcontacts", LBVH_SORT_RECORDS_DESCENDING}, {"triprox", LBVH_SORT_RECORDS_ASCENDING},
        {"trisegs", LBVH_SORT_RECORDS_BY_TRI},      {"sections", LBVH_SORT_RECORDS_BY_TRI}};
    uint32_t order = 3;
    for (const auto& k : kinds)
        if (argc > 2 && std::strcmp(argv[2], k.kind) == 0) order = k.order;
    if (order > LBVH_SORT_RECORDS_BY_TRI) throw std::runtime_error("sortedrecords <contacts|boxcontacts|triprox|trisegs|sections> <n> [seed]");
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 4096;
    uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 5;
    // segment q: every 97th has 300 .. 2 299 records, the others 0 .. 23
    std::vector<uint64_t> off(count + 1, 0);
    for (size_t q = 0; q < count; q++)
        off[q + 1] = off[q] + (q % 97 == 5 ? 300u + (uint32_t)uniform(seed, 0.0f, 2000.0f) : (uint32_t)uniform(seed, 0.0f, 24.0f));
    const uint64_t total = off[count];
    lbvh::Context ctx(0);
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    offsets.LocalBuffer() = off;
    offsets.Sync();
    lbvh::DataBuffer<lbvh_contact> records(ctx, std::max<size_t>((size_t)total, 1));
    // record j of segment q, i its position in the list: word 0 a multiple of 0.25 in [-2, 2) (many ties), words 1 and 3 distinct
    // inside the segment (j times an odd number), the other words a fingerprint of i
    for (size_t q = 0; q < count; q++)
        for (uint64_t i = off[q]; i < off[q + 1]; i++) {
            const uint32_t j = (uint32_t)(i - off[q]);
            const float v = floorf(uniform(seed, 0.0f, 16.0f)) * 0.25f - 2.0f;
            uint32_t w[8];
            for (uint32_t k = 0; k < 8; k++) w[k] = ((uint32_t)i * 8u + k) * 2654435761u;
            std::memcpy(&w[0], &v, 4);
            w[1] = j * 2654435761u + (uint32_t)q;
            w[3] = j * 2246822519u + 7u * (uint32_t)q;
            std::memcpy(&records.LocalBuffer()[i], w, 32);
        }
    records.Sync();
    lbvh::RaytracingMeshDrawer drawer(ctx, random_mesh(64));       // the sort needs no scene: the wrapper is the drawer's
    drawer.SortRecordSegments(offsets, records, count, order);
    records.GetData();
    uint64_t words = 0, weighted_sum = 0;
    size_t nonempty = 0;
    for (size_t q = 0; q < count; q++) nonempty += off[q + 1] > off[q];
    for (uint64_t i = 0; i < total; i++) {
        uint32_t w[8];
        std::memcpy(w, &records.LocalBuffer()[i], 32);
        for (uint32_t k = 0; k < 8; k++) words += w[k];
        weighted_sum += (i + 1) * (uint64_t)(w[1] ^ w[7]);
    }
    std::printf("{\"kind\": \"%s\", \"order\": %u, \"segments\": %zu, \"total\": %llu, \"nonempty\": %zu, \"word_sum\": %llu, \"weighted_sum\": %llu}\n",
                argv[2], order, count, (unsigned long long)total, nonempty, (unsigned long long)words, (unsigned long long)weighted_sum);
    return 0;
}

static int sweep_main(int argc, char** argv)
{
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 65536;
    const std::vector<lbvh_triangle> mesh = load_mesh(argc > 2 ? argv[2] : "4096");
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    const float extent = std::fmax(hi[0] - lo[0], std::fmax(hi[1] - lo[1], hi[2] - lo[2]));
    const float radius = argc > 4 ? (float)atof(argv[4]) : 0.01f * extent;
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_sphere_ray> casts(ctx, count);
    rays_into(lo, hi, 3, casts.LocalBuffer());
    for (auto& c : casts.LocalBuffer()) { c.radius = radius; c.t_max = 2.0f; }
    casts.Sync();
    lbvh::DataBuffer<lbvh_hit> hits(ctx, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    drawer.SphereCast(casts, hits);
    drawer.SphereCastAny(casts, flags);
    hits.GetData();
    flags.GetData();
    size_t touching = 0, flagged = 0, at_start = 0;
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        const lbvh_hit& h = hits.LocalBuffer()[i];
        words += word_sum(h);
        touching += h.t < LBVH_MAX_FLOAT;
        at_start += h.t == 0.0f;
        flagged += flags.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"casts\": %zu, \"radius\": %.9g, \"touching\": %zu, \"flagged\": %zu, \"at_start\": %zu, "
                "\"word_sum\": %llu, \"records\": [",
                mesh.size(), count, radius, touching, flagged, at_start, (unsigned long long)words);
    for (size_t i = 0; i < std::min<size_t>(count, 3); i++) {
        const lbvh_hit& h = hits.LocalBuffer()[i];
        std::printf("%s[%.9g, %u, %.9g, %.9g]", i ? ", " : "", h.t, h.tri, h.u, h.v);
    }
    std::printf("]}\n");
    return 0;
}

// lbvh_driver overlaps [n | file.obj] [count] [size]: `count` boxes with centres in the mesh's box and half-extents up to `size` x its
// extent, and the balls of the same centres with radius up to `size` x the largest extent; count -> one 8-byte read -> fill
static int overlaps_main(int argc, char** argv)
{
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 65536;
    const float size = argc > 4 ? (float)atof(argv[4]) : 0.1f;
    const std::vector<lbvh_triangle> mesh = load_mesh(argc > 2 ? argv[2] : "4096");
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    const float widest = std::fmax(hi[0] - lo[0], std::fmax(hi[1] - lo[1], hi[2] - lo[2]));
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_aabb> boxes(ctx, count);
    lbvh::DataBuffer<lbvh_point_query> balls(ctx, count);
    uint64_t seed = 3;
    for (size_t i = 0; i < count; i++) {
        lbvh_aabb& b = boxes.LocalBuffer()[i];
        lbvh_point_query& q = balls.LocalBuffer()[i];
        std::memset(&b, 0, sizeof b);
        for (int k = 0; k < 3; k++) {
            const float c = uniform(seed, lo[k], hi[k]), h = uniform(seed, 0.0f, size * (hi[k] - lo[k]));
            b.min[k] = c - h;
            b.max[k] = c + h;
            q.p[k] = c;
        }
        const float r = uniform(seed, 0.0f, size * widest);
        q.max_dist2 = r * r;
    }
    boxes.Sync();
    balls.Sync();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    unsigned long long total[2] = {0, 0}, index_sum[2] = {0, 0};
    for (int form = 0; form < 2; form++) {
        if (form == 0) drawer.BoxOverlaps(boxes, offsets);
        else drawer.GatherWithinDistance(balls, offsets);
        offsets.GetData();
        total[form] = offsets.LocalBuffer()[count];
        lbvh::DataBuffer<uint32_t> tris(ctx, total[form] ? (size_t)total[form] : 1);
        if (form == 0) drawer.BoxOverlaps(boxes, offsets, &tris);
        else drawer.GatherWithinDistance(balls, offsets, &tris);
        tris.GetData();
        for (size_t i = 0; i < (size_t)total[form]; i++) index_sum[form] += tris.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"queries\": %zu, \"box_total\": %llu, \"box_index_sum\": %llu, \"ball_total\": %llu, \"ball_index_sum\": %llu}\n",
                mesh.size(), count, total[0], index_sum[0], total[1], index_sum[1]);
    return 0;
}

// the query triangles of `tris` and `trisegs`: per axis a centre uniform in the box, then b's and c's offsets uniform in [-3, 3]
static void triangles_in(lbvh::DataBuffer<lbvh_tri_query>& queries, uint64_t& seed, const float lo[3], const float hi[3])
{
    for (size_t i = 0; i < queries.Size(); i++) {
        lbvh_tri_query& q = queries.LocalBuffer()[i];
        std::memset(&q, 0, sizeof q);
        q.skip = LBVH_NULL;
        for (int k = 0; k < 3; k++) {
            const float centre = uniform(seed, lo[k], hi[k]);
            q.a[k] = centre;
            q.b[k] = centre + uniform(seed, -3.0f, 3.0f);
            q.c[k] = centre + uniform(seed, -3.0f, 3.0f);
        }
    }
    queries.Sync();
}

static int tris_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 5;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_tri_query> queries(ctx, count);
    triangles_in(queries, seed, lo, hi);
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    drawer.TriangleIntersections(queries, offsets);
    offsets.GetData();
    const unsigned long long total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<uint32_t> tris(ctx, total ? (size_t)total : 1);
    drawer.TriangleIntersections(queries, offsets, &tris);
    drawer.SortIndexSegments(offsets, tris, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    drawer.TriangleIntersectsAny(queries, flags);
    offsets.GetData();
    tris.GetData();
    flags.GetData();
    size_t non_empty = 0, flagged = 0;
    unsigned long long weighted = 0;
    for (size_t i = 0; i < count; i++) {
        non_empty += offsets.LocalBuffer()[i + 1] > offsets.LocalBuffer()[i];
        flagged += flags.LocalBuffer()[i];
    }
    for (size_t i = 0; i < (size_t)total; i++) weighted += (unsigned long long)(i + 1) * tris.LocalBuffer()[i];
    std::printf("{\"triangles\": %zu, \"queries\": %zu, \"total\": %llu, \"non_empty\": %zu, \"flagged\": %zu, \"weighted_index_sum\": %llu, \"segments\": [",
                mesh.size(), count, total, non_empty, flagged, weighted);
    size_t shown = 0;
    for (size_t i = 0; i < count && shown < 3; i++) {
        const uint64_t first = offsets.LocalBuffer()[i], last = offsets.LocalBuffer()[i + 1];
        if (first == last) continue;
        std::printf("%s[%zu", shown++ ? ", " : "", i);
        for (uint64_t j = first; j < last; j++) std::printf(", %u", tris.LocalBuffer()[j]);
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

// moving triangles against the mesh of `tris`: per cast and axis k the vertex a around the mesh's box (as `sweep` draws an origin),
// b's and c's offsets uniform in [-3, 3], then dir = a target uniform in the box minus a (the casts of `tricast` and of
// `castall triangle`)
static void triangle_casts(const float lo[3], const float hi[3], uint64_t seed, float t_max, std::vector<lbvh_tri_ray>& casts)
{
    for (auto& c : casts) {
        std::memset(&c, 0, sizeof c);
        c.skip = LBVH_NULL;
        c.t_max = t_max;
        for (int k = 0; k < 3; k++) {
            const float grow = 0.25f * (hi[k] - lo[k]);
            c.a[k] = uniform(seed, lo[k] - grow, hi[k] + grow);
            c.b[k] = c.a[k] + uniform(seed, -3.0f, 3.0f);
            c.c[k] = c.a[k] + uniform(seed, -3.0f, 3.0f);
            c.dir[k] = uniform(seed, lo[k], hi[k]) - c.a[k];
        }
    }
}

// TriangleCast and TriangleCastAny.
static int tricast_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 6000;
    const uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 5;
    const float t_max = argc > 4 ? (float)atof(argv[4]) : 2.0f;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_tri_ray> casts(ctx, count);
    triangle_casts(lo, hi, seed, t_max, casts.LocalBuffer());
    casts.Sync();
    lbvh::DataBuffer<lbvh_tri_cast_hit> hits(ctx, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    drawer.TriangleCast(casts, hits);
    drawer.TriangleCastAny(casts, flags);
    hits.GetData();
    flags.GetData();
    size_t touching = 0, flagged = 0, at_start = 0, by_feature[22] = {};
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        const lbvh_tri_cast_hit& h = hits.LocalBuffer()[i];
        words += word_sum(h);
        touching += h.t < LBVH_MAX_FLOAT;
        at_start += h.t < LBVH_MAX_FLOAT && (h.feature & LBVH_TRI_CAST_START) != 0;
        if (h.t < LBVH_MAX_FLOAT && h.feature < 22) by_feature[h.feature]++;
        flagged += flags.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"casts\": %zu, \"t_max\": %.9g, \"touching\": %zu, \"flagged\": %zu, \"at_start\": %zu, "
                "\"word_sum\": %llu, \"by_feature\": [",
                mesh.size(), count, t_max, touching, flagged, at_start, (unsigned long long)words);
    for (int j = 0; j < 22; j++) std::printf("%s%zu", j ? ", " : "", by_feature[j]);
    std::printf("], \"records\": [");
    for (size_t i = 0; i < std::min<size_t>(count, 3); i++) {
        const lbvh_tri_cast_hit& h = hits.LocalBuffer()[i];
        std::printf("%s[%.9g, %u, %u, %.9g]", i ? ", " : "", h.t, h.tri, h.feature, h.w);
    }
    std::printf("]}\n");
    return 0;
}

// `tris` with a record in place of an index: TriangleIntersectionSegments (count only, one 8-byte read, fill), every segment sorted
// by tri on the host.  offset_sum = the sum of (k + 1) * offsets[k], record_sum = the sum of (position + 1) * (the sum of the
// record's eight words) over the sorted list, both mod 2^64.
static int trisegs_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 5;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_tri_query> queries(ctx, count);
    triangles_in(queries, seed, lo, hi);
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    drawer.TriangleIntersectionSegments(queries, offsets);
    offsets.GetData();
    const unsigned long long total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<lbvh_tri_segment> segments(ctx, total ? (size_t)total : 1);
    drawer.TriangleIntersectionSegments(queries, offsets, &segments);
    offsets.GetData();
    segments.GetData();
    std::vector<lbvh_tri_segment>& rec = segments.LocalBuffer();
    size_t non_empty = 0, two_ends = 0;
    unsigned long long offset_sum = 0, record_sum = 0;
    for (size_t k = 0; k <= count; k++) offset_sum += (unsigned long long)(k + 1) * offsets.LocalBuffer()[k];
    for (size_t k = 0; k < count; k++) {
        const uint64_t first = offsets.LocalBuffer()[k], last = offsets.LocalBuffer()[k + 1];
        non_empty += last > first;
        std::sort(rec.begin() + (ptrdiff_t)first, rec.begin() + (ptrdiff_t)last,
                  [](const lbvh_tri_segment& x, const lbvh_tri_segment& y) { return x.tri < y.tri; });
    }
    for (size_t i = 0; i < (size_t)total; i++) {
        uint32_t w[8];
        std::memcpy(w, &rec[i], sizeof w);
        unsigned long long words = 0;
        for (uint32_t x : w) words += x;
        record_sum += (unsigned long long)(i + 1) * words;
        two_ends += ((rec[i].edges >> 8) & 7u) != ((rec[i].edges >> 12) & 7u);
    }
    std::printf("{\"triangles\": %zu, \"queries\": %zu, \"total\": %llu, \"non_empty\": %zu, \"two_ends\": %zu, \"offset_sum\": %llu, "
                "\"record_sum\": %llu}\n", mesh.size(), count, total, non_empty, two_ends, offset_sum, record_sum);
    return 0;
}

// `sections`: PlaneSections (count only, one 8-byte read, fill), every segment sorted by tri on the host; the sums of `trisegs`
static int sections_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 64;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 7;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_plane> planes(ctx, count);
    for (size_t i = 0; i < count; i++) {
        lbvh_plane& q = planes.LocalBuffer()[i];
        float p[3];
        for (int k = 0; k < 3; k++) {
            q.n[k] = uniform(seed, -1.0f, 1.0f);
            p[k] = uniform(seed, lo[k], hi[k]);
        }
        const float xy = q.n[0] * p[0] + q.n[1] * p[1];
        const float xyz = xy + q.n[2] * p[2];
        q.d = -xyz;
    }
    planes.Sync();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    drawer.PlaneSections(planes, offsets);
    offsets.GetData();
    const unsigned long long total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<lbvh_plane_segment> segments(ctx, total ? (size_t)total : 1);
    drawer.PlaneSections(planes, offsets, &segments);
    offsets.GetData();
    segments.GetData();
    std::vector<lbvh_plane_segment>& rec = segments.LocalBuffer();
    size_t non_empty = 0;
    unsigned long long offset_sum = 0, record_sum = 0;
    for (size_t k = 0; k <= count; k++) offset_sum += (unsigned long long)(k + 1) * offsets.LocalBuffer()[k];
    for (size_t k = 0; k < count; k++) {
        const uint64_t first = offsets.LocalBuffer()[k], last = offsets.LocalBuffer()[k + 1];
        non_empty += last > first;
        std::sort(rec.begin() + (ptrdiff_t)first, rec.begin() + (ptrdiff_t)last,
                  [](const lbvh_plane_segment& x, const lbvh_plane_segment& y) { return x.tri < y.tri; });
    }
    for (size_t i = 0; i < (size_t)total; i++) {
        uint32_t w[8];
        std::memcpy(w, &rec[i], sizeof w);
        unsigned long long words = 0;
        for (uint32_t x : w) words += x;
        record_sum += (unsigned long long)(i + 1) * words;
    }
    std::printf("{\"triangles\": %zu, \"planes\": %zu, \"total\": %llu, \"non_empty\": %zu, \"offset_sum\": %llu, \"record_sum\": %llu}\n",
                mesh.size(), count, total, non_empty, offset_sum, record_sum);
    return 0;
}

// one shape family of `shapes`: the CSR list (count only, one 8-byte read, fill), the device sort and the flags, printed as fields
// of the line `shapes_main` opens
template <class SHAPE, class LIST, class ANY>
static void shape_lists(lbvh::Context& ctx, lbvh::RaytracingMeshDrawer& drawer, const lbvh::DataBuffer<SHAPE>& shapes, const char* name, LIST list, ANY any)
{
    const size_t count = shapes.Size();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    list(shapes, offsets, nullptr);
    offsets.GetData();
    const unsigned long long total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<uint32_t> tris(ctx, total ? (size_t)total : 1);
    list(shapes, offsets, &tris);
    drawer.SortIndexSegments(offsets, tris, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    any(shapes, flags);
    offsets.GetData();
    tris.GetData();
    flags.GetData();
    size_t non_empty = 0, flagged = 0;
    unsigned long long weighted = 0;
    for (size_t i = 0; i < count; i++) {
        non_empty += offsets.LocalBuffer()[i + 1] > offsets.LocalBuffer()[i];
        flagged += flags.LocalBuffer()[i];
    }
    for (size_t i = 0; i < (size_t)total; i++) weighted += (unsigned long long)(i + 1) * tris.LocalBuffer()[i];
    std::printf(", \"%s\": {\"total\": %llu, \"non_empty\": %zu, \"flagged\": %zu, \"weighted_index_sum\": %llu, \"segments\": [", name, total,
                non_empty, flagged, weighted);
    size_t shown = 0;
    for (size_t i = 0; i < count && shown < 3; i++) {
        const uint64_t first = offsets.LocalBuffer()[i], last = offsets.LocalBuffer()[i + 1];
        if (first == last) continue;
        std::printf("%s[%zu", shown++ ? ", " : "", i);
        for (uint64_t j = first; j < last; j++) std::printf(", %u", tris.LocalBuffer()[j]);
        std::printf("]");
    }
    std::printf("]}");
}

static int shapes_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 7;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_capsule> capsules(ctx, count);
    lbvh::DataBuffer<lbvh_obb> boxes(ctx, count);
    const float half = 3.0f;
    for (size_t i = 0; i < count; i++) {
        lbvh_capsule& c = capsules.LocalBuffer()[i];
        lbvh_obb& b = boxes.LocalBuffer()[i];
        std::memset(&c, 0, sizeof c);
        std::memset(&b, 0, sizeof b);
        c.radius = 3.0f;
        for (int k = 0; k < 3; k++) {
            c.origin[k] = uniform(seed, lo[k], hi[k]);
            c.axis[k] = uniform(seed, -6.0f, 6.0f);
            b.centre[k] = uniform(seed, lo[k], hi[k]);
            b.ax[k] = (k == 0 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            b.ay[k] = (k == 1 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            b.az[k] = (k == 2 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
        }
    }
    capsules.Sync();
    boxes.Sync();
    std::printf("{\"triangles\": %zu, \"shapes\": %zu", mesh.size(), count);
    shape_lists(ctx, drawer, capsules, "capsule",
                [&](const lbvh::DataBuffer<lbvh_capsule>& s, lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<uint32_t>* t) { drawer.CapsuleOverlaps(s, o, t); },
                [&](const lbvh::DataBuffer<lbvh_capsule>& s, lbvh::DataBuffer<uint32_t>& f) { drawer.CapsuleOverlapsAny(s, f); });
    shape_lists(ctx, drawer, boxes, "obb",
                [&](const lbvh::DataBuffer<lbvh_obb>& s, lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<uint32_t>* t) { drawer.ObbOverlaps(s, o, t); },
                [&](const lbvh::DataBuffer<lbvh_obb>& s, lbvh::DataBuffer<uint32_t>& f) { drawer.ObbOverlapsAny(s, f); });
    std::printf("}\n");
    return 0;
}

// `contacts` / `boxcontacts`: the list form (count only, one 8-byte read, fill) and the deepest form on one set of shapes; REC is the
// 32-byte record.  The order inside a segment is the walk's, so the list is summed: word_sum = the sum over all records of
// sum_k (k + 1) * word k of the record (64-bit, wrapping); deepest_sum weights shape i's record by i + 1 as well.
template <class REC, class SHAPE, class LIST, class DEEPEST>
static void contact_report(lbvh::Context& ctx, const lbvh::DataBuffer<SHAPE>& shapes, size_t triangles, LIST list, DEEPEST deepest_of)
{
    static_assert(sizeof(REC) == 32, "a contact record is eight words");
    const size_t count = shapes.Size();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    list(shapes, offsets, nullptr);
    offsets.GetData();
    const unsigned long long total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<REC> contacts(ctx, total ? (size_t)total : 1);
    list(shapes, offsets, &contacts);
    lbvh::DataBuffer<REC> deepest(ctx, count);
    deepest_of(shapes, deepest);
    offsets.GetData();
    contacts.GetData();
    deepest.GetData();
    auto weigh = [](const REC& c) {
        uint32_t w[8];
        std::memcpy(w, &c, sizeof w);
        unsigned long long sum = 0;
        for (int k = 0; k < 8; k++) sum += (unsigned long long)(k + 1) * w[k];
        return sum;
    };
    size_t non_empty = 0, touching = 0;
    unsigned long long word_sum = 0, deepest_sum = 0;
    for (size_t i = 0; i < count; i++) {
        non_empty += offsets.LocalBuffer()[i + 1] > offsets.LocalBuffer()[i];
        touching += deepest.LocalBuffer()[i].tri != LBVH_NULL;
        deepest_sum += (unsigned long long)(i + 1) * weigh(deepest.LocalBuffer()[i]);
    }
    for (size_t i = 0; i < (size_t)total; i++) word_sum += weigh(contacts.LocalBuffer()[i]);
    std::printf("{\"triangles\": %zu, \"shapes\": %zu, \"total\": %llu, \"non_empty\": %zu, \"touching\": %zu, \"word_sum\": %llu, \"deepest_sum\": %llu, "
                "\"deepest\": [", triangles, count, total, non_empty, touching, word_sum, deepest_sum);
    size_t shown = 0;
    for (size_t i = 0; i < count && shown < 3; i++) {
        if (deepest.LocalBuffer()[i].tri == LBVH_NULL) continue;
        uint32_t w[8];
        std::memcpy(w, &deepest.LocalBuffer()[i], sizeof w);
        std::printf("%s[%zu", shown++ ? ", " : "", i);
        for (int k = 0; k < 8; k++) std::printf(", %u", w[k]);
        std::printf("]");
    }
    std::printf("]}\n");
}

static int contacts_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 11;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_capsule> capsules(ctx, count);
    for (size_t i = 0; i < count; i++) {
        lbvh_capsule& c = capsules.LocalBuffer()[i];
        std::memset(&c, 0, sizeof c);
        c.radius = 3.0f;
        for (int k = 0; k < 3; k++) {
            c.origin[k] = uniform(seed, lo[k], hi[k]);
            c.axis[k] = uniform(seed, -6.0f, 6.0f);
        }
    }
    capsules.Sync();
    contact_report<lbvh_contact>(
        ctx, capsules, mesh.size(),
        [&](const lbvh::DataBuffer<lbvh_capsule>& s, lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_contact>* c) { drawer.CapsuleContacts(s, o, c); },
        [&](const lbvh::DataBuffer<lbvh_capsule>& s, lbvh::DataBuffer<lbvh_contact>& d) { drawer.CapsuleDeepest(s, d); });
    return 0;
}

static int segclosest_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 15;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_segment_query> queries(ctx, count);
    for (size_t i = 0; i < count; i++) {
        lbvh_segment_query& q = queries.LocalBuffer()[i];
        std::memset(&q, 0, sizeof q);
        q.max_dist2 = (i & 1) ? INFINITY : 9.0f;
        for (int k = 0; k < 3; k++) {
            q.origin[k] = uniform(seed, lo[k], hi[k]);
            q.axis[k] = uniform(seed, -6.0f, 6.0f);
        }
    }
    queries.Sync();
    lbvh::DataBuffer<lbvh_segment_closest> closest(ctx, count);
    lbvh::DataBuffer<uint32_t> within(ctx, count);
    drawer.SegmentClosestPoints(queries, closest);
    drawer.SegmentWithinDistance(queries, within);
    closest.GetData();
    within.GetData();
    size_t found = 0, n_within = 0;
    unsigned long long words = 0;
    for (size_t i = 0; i < count; i++) {
        uint32_t w[8];
        std::memcpy(w, &closest.LocalBuffer()[i], sizeof w);
        unsigned long long sum = 0;
        for (int k = 0; k < 8; k++) sum += (unsigned long long)(k + 1) * w[k];
        words += (unsigned long long)(i + 1) * sum;
        found += closest.LocalBuffer()[i].dist2 != LBVH_MAX_FLOAT;
        n_within += within.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"segments\": %zu, \"found\": %zu, \"within\": %zu, \"word_sum\": %llu, \"closest\": [", mesh.size(), count,
                found, n_within, words);
    size_t shown = 0;
    for (size_t i = 0; i < count && shown < 3; i++) {
        if (closest.LocalBuffer()[i].dist2 == LBVH_MAX_FLOAT) continue;
        uint32_t w[8];
        std::memcpy(w, &closest.LocalBuffer()[i], sizeof w);
        std::printf("%s[%zu", shown++ ? ", " : "", i);
        for (int k = 0; k < 8; k++) std::printf(", %u", w[k]);
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

static int triclosest_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 21;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_tri_distance_query> queries(ctx, count);
    for (size_t i = 0; i < count; i++) {               // the draws of triangles_in
        lbvh_tri_distance_query& q = queries.LocalBuffer()[i];
        std::memset(&q, 0, sizeof q);
        q.skip = LBVH_NULL;
        q.max_dist2 = (i & 1) ? INFINITY : 4.0f;
        for (int k = 0; k < 3; k++) {
            const float centre = uniform(seed, lo[k], hi[k]);
            q.a[k] = centre;
            q.b[k] = centre + uniform(seed, -3.0f, 3.0f);
            q.c[k] = centre + uniform(seed, -3.0f, 3.0f);
        }
    }
    queries.Sync();
    lbvh::DataBuffer<lbvh_tri_closest> closest(ctx, count);
    lbvh::DataBuffer<uint32_t> within(ctx, count);
    drawer.TriangleClosestPoints(queries, closest);
    drawer.TriangleWithinDistance(queries, within);
    closest.GetData();
    within.GetData();
    size_t found = 0, n_within = 0, pierced = 0;
    unsigned long long words = 0;
    for (size_t i = 0; i < count; i++) {
        uint32_t w[8];
        std::memcpy(w, &closest.LocalBuffer()[i], sizeof w);
        unsigned long long sum = 0;
        for (int k = 0; k < 8; k++) sum += (unsigned long long)(k + 1) * w[k];
        words += (unsigned long long)(i + 1) * sum;
        found += closest.LocalBuffer()[i].dist2 != LBVH_MAX_FLOAT;
        pierced += (closest.LocalBuffer()[i].edge & 8u) != 0;
        n_within += within.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"queries\": %zu, \"found\": %zu, \"within\": %zu, \"pierced\": %zu, \"word_sum\": %llu, \"closest\": [",
                mesh.size(), count, found, n_within, pierced, words);
    size_t shown = 0;
    for (size_t i = 0; i < count && shown < 3; i++) {
        if (closest.LocalBuffer()[i].dist2 == LBVH_MAX_FLOAT) continue;
        uint32_t w[8];
        std::memcpy(w, &closest.LocalBuffer()[i], sizeof w);
        std::printf("%s[%zu", shown++ ? ", " : "", i);
        for (int k = 0; k < 8; k++) std::printf(", %u", w[k]);
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

static int triprox_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 21;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_tri_distance_query> queries(ctx, count);
    for (size_t i = 0; i < count; i++) {               // the draws of triclosest
        lbvh_tri_distance_query& q = queries.LocalBuffer()[i];
        std::memset(&q, 0, sizeof q);
        q.skip = LBVH_NULL;
        q.max_dist2 = 4.0f;
        for (int k = 0; k < 3; k++) {
            const float centre = uniform(seed, lo[k], hi[k]);
            q.a[k] = centre;
            q.b[k] = centre + uniform(seed, -3.0f, 3.0f);
            q.c[k] = centre + uniform(seed, -3.0f, 3.0f);
        }
    }
    queries.Sync();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    drawer.TriangleGatherWithinDistance(queries, offsets);              // count only
    offsets.GetData();
    const size_t total = (size_t)offsets.LocalBuffer()[count];
    lbvh::DataBuffer<lbvh_tri_closest> records(ctx, total ? total : 1);
    drawer.TriangleGatherWithinDistance(queries, offsets, &records);
    offsets.GetData();
    records.GetData();
    size_t nonempty = 0, longest = 0, pierced = 0;
    unsigned long long words = 0;
    lbvh_tri_closest* rec = records.LocalBuffer().data();
    for (size_t i = 0; i < count; i++) {
        const size_t from = (size_t)offsets.LocalBuffer()[i], to = (size_t)offsets.LocalBuffer()[i + 1];
        nonempty += to > from;
        longest = std::max(longest, to - from);
        std::sort(rec + from, rec + to, [](const lbvh_tri_closest& x, const lbvh_tri_closest& y) { return x.tri < y.tri; });
        for (size_t p = from; p < to; p++) {
            uint32_t w[8];
            std::memcpy(w, &rec[p], sizeof w);
            unsigned long long sum = 0;
            for (int k = 0; k < 8; k++) sum += (unsigned long long)(k + 1) * w[k];
            words += (unsigned long long)(p + 1) * sum;
            pierced += (rec[p].edge & 8u) != 0;
        }
    }
    std::printf("{\"triangles\": %zu, \"queries\": %zu, \"total\": %zu, \"nonempty\": %zu, \"longest\": %zu, \"pierced\": %zu, \"word_sum\": %llu}\n",
                mesh.size(), count, total, nonempty, longest, pierced, words);
    return 0;
}

static int boxcontacts_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 13;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_obb> boxes(ctx, count);
    const float half = 3.0f;
    for (size_t i = 0; i < count; i++) {
        lbvh_obb& b = boxes.LocalBuffer()[i];
        std::memset(&b, 0, sizeof b);
        for (int k = 0; k < 3; k++) {
            b.centre[k] = uniform(seed, lo[k], hi[k]);
            b.ax[k] = (k == 0 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            b.ay[k] = (k == 1 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            b.az[k] = (k == 2 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
        }
    }
    boxes.Sync();
    contact_report<lbvh_box_contact>(
        ctx, boxes, mesh.size(),
        [&](const lbvh::DataBuffer<lbvh_obb>& s, lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_box_contact>* c) { drawer.ObbContacts(s, o, c); },
        [&](const lbvh::DataBuffer<lbvh_obb>& s, lbvh::DataBuffer<lbvh_box_contact>& d) { drawer.ObbDeepest(s, d); });
    return 0;
}

static int regions_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 6;
    const bool large = argc > 4 && std::string(argv[4]) == "large";
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_region> regions(ctx, count);
    for (size_t i = 0; i < count; i++) {
        lbvh_region& r = regions.LocalBuffer()[i];
        float c[3];
        for (int k = 0; k < 3; k++) c[k] = uniform(seed, lo[k], hi[k]);
        for (int k = 0; k < 3; k++) {
            float n[3] = {0.0f, 0.0f, 0.0f};
            n[k] = 1.0f;
            for (int j = 0; j < 3; j++)
                if (j != k) n[j] = uniform(seed, -0.5f, 0.5f);
            const float h = uniform(seed, 1.0f, 12.0f);
            const float p0 = n[0] * c[0], p1 = n[1] * c[1], p2 = n[2] * c[2];         // every operation rounded on its own, as the mirror has it
            const float s01 = p0 + p1;
            const float s = s01 + p2;
            for (int j = 0; j < 3; j++) { r.plane[2 * k][j] = n[j]; r.plane[2 * k + 1][j] = -n[j]; }
            r.plane[2 * k][3] = h - s;
            r.plane[2 * k + 1][3] = h + s;
        }
    }
    regions.Sync();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    std::printf("{\"triangles\": %zu, \"regions\": %zu%s", mesh.size(), count, large ? ", \"large\": true" : "");
    auto lists = [&](uint32_t mode, lbvh::DataBuffer<uint32_t>* tris) {
        if (large) drawer.RegionOverlapsLarge(regions, mode, offsets, tris);
        else drawer.RegionOverlaps(regions, mode, offsets, tris);
    };
    for (uint32_t mode : {LBVH_REGION_CONTAINED, LBVH_REGION_TOUCHING}) {
        lists(mode, nullptr);
        offsets.GetData();
        const unsigned long long total = offsets.LocalBuffer()[count];
        lbvh::DataBuffer<uint32_t> tris(ctx, total ? (size_t)total : 1);
        lists(mode, &tris);
        drawer.SortIndexSegments(offsets, tris, count);
        drawer.RegionOverlapsAny(regions, mode, flags);
        offsets.GetData();
        tris.GetData();
        flags.GetData();
        size_t non_empty = 0, flagged = 0;
        unsigned long long weighted = 0;
        for (size_t i = 0; i < count; i++) {
            non_empty += offsets.LocalBuffer()[i + 1] > offsets.LocalBuffer()[i];
            flagged += flags.LocalBuffer()[i];
        }
        for (size_t i = 0; i < (size_t)total; i++) weighted += (unsigned long long)(i + 1) * tris.LocalBuffer()[i];
        std::printf(", \"%s\": {\"total\": %llu, \"non_empty\": %zu, \"flagged\": %zu, \"weighted_index_sum\": %llu}",
                    mode == LBVH_REGION_TOUCHING ? "touching" : "contained", total, non_empty, flagged, weighted);
        if (mode != LBVH_REGION_TOUCHING) continue;
        std::printf(", \"segments\": [");
        size_t shown = 0;
        for (size_t i = 0; i < count && shown < 3; i++) {
            const uint64_t first = offsets.LocalBuffer()[i], last = offsets.LocalBuffer()[i + 1];
            if (first == last) continue;
            std::printf("%s[%zu", shown++ ? ", " : "", i);
            for (uint64_t j = first; j < last; j++) std::printf(", %u", tris.LocalBuffer()[j]);
            std::printf("]");
        }
        std::printf("]");
    }
    std::printf("}\n");
    return 0;
}

// the casts of `capsule` and of `castall capsule`: per axis the origin and the target as rays_into draws them, then the axis component
static void capsule_casts(const float lo[3], const float hi[3], uint64_t seed, float radius, float height, float t_max,
                          std::vector<lbvh_capsule_ray>& casts)
{
    for (auto& c : casts) {
        std::memset(&c, 0, sizeof c);
        for (int k = 0; k < 3; k++) {
            const float grow = 0.25f * (hi[k] - lo[k]);
            c.origin[k] = uniform(seed, lo[k] - grow, hi[k] + grow);
            c.dir[k] = uniform(seed, lo[k], hi[k]) - c.origin[k];
            c.axis[k] = uniform(seed, -height, height);
        }
        c.radius = radius;
        c.t_max = t_max;
    }
}

// the casts of `boxcast` and of `castall box`: per axis k the centre and the target, then component k of ax, ay, az
static void box_casts(const float lo[3], const float hi[3], uint64_t seed, float half, float t_max, std::vector<lbvh_box_ray>& casts)
{
    for (auto& c : casts) {
        std::memset(&c, 0, sizeof c);
        for (int k = 0; k < 3; k++) {
            const float grow = 0.25f * (hi[k] - lo[k]);
            c.centre[k] = uniform(seed, lo[k] - grow, hi[k] + grow);
            c.dir[k] = uniform(seed, lo[k], hi[k]) - c.centre[k];
            c.ax[k] = (k == 0 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            c.ay[k] = (k == 1 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
            c.az[k] = (k == 2 ? half : 0.0f) + uniform(seed, -0.5f * half, 0.5f * half);
        }
        c.t_max = t_max;
    }
}

static int capsule_main(int argc, char** argv)
{
    const size_t count = argc > 2 ? (size_t)strtoull(argv[2], nullptr, 10) : 65536;
    uint64_t seed = argc > 3 ? strtoull(argv[3], nullptr, 10) : 3;
    const float radius = argc > 4 ? (float)atof(argv[4]) : 1.5f;
    const float height = argc > 5 ? (float)atof(argv[5]) : 4.0f;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_capsule_ray> casts(ctx, count);
    capsule_casts(lo, hi, seed, radius, height, 2.0f, casts.LocalBuffer());
    casts.Sync();
    lbvh::DataBuffer<lbvh_hit> hits(ctx, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    drawer.CapsuleCast(casts, hits);
    drawer.CapsuleCastAny(casts, flags);
    hits.GetData();
    flags.GetData();
    size_t touching = 0, flagged = 0, at_start = 0;
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        const lbvh_hit& h = hits.LocalBuffer()[i];
        words += word_sum(h);
        touching += h.t < LBVH_MAX_FLOAT;
        at_start += h.t == 0.0f;
        flagged += flags.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"casts\": %zu, \"radius\": %.9g, \"height\": %.9g, \"touching\": %zu, \"flagged\": %zu, "
                "\"at_start\": %zu, \"word_sum\": %llu, \"records\": [",
                mesh.size(), count, radius, height, touching, flagged, at_start, (unsigned long long)words);
    for (size_t i = 0; i < std::min<size_t>(count, 3); i++) {
        const lbvh_hit& h = hits.LocalBuffer()[i];
        std::printf("%s[%.9g, %u, %.9g, %.9g]", i ? ", " : "", h.t, h.tri, h.u, h.v);
    }
    std::printf("]}\n");
    return 0;
}

static int boxcast_main(int argc, char** argv)
{
    uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 10) : 3;
    const float half = argc > 3 ? (float)atof(argv[3]) : 1.5f;
    const float t_max = argc > 4 ? (float)atof(argv[4]) : 2.0f;
    const size_t count = argc > 5 ? (size_t)strtoull(argv[5], nullptr, 10) : 6000;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_box_ray> casts(ctx, count);
    box_casts(lo, hi, seed, half, t_max, casts.LocalBuffer());
    casts.Sync();
    lbvh::DataBuffer<lbvh_box_hit> hits(ctx, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    drawer.BoxCast(casts, hits);
    drawer.BoxCastAny(casts, flags);
    hits.GetData();
    flags.GetData();
    size_t touching = 0, flagged = 0, at_start = 0, by_axis[14] = {};
    uint64_t words = 0;
    for (size_t i = 0; i < count; i++) {
        const lbvh_box_hit& h = hits.LocalBuffer()[i];
        words += word_sum(h);
        touching += h.t < LBVH_MAX_FLOAT;
        at_start += h.t == 0.0f;
        if (h.t < LBVH_MAX_FLOAT && h.axis < 14) by_axis[h.axis]++;
        flagged += flags.LocalBuffer()[i];
    }
    std::printf("{\"triangles\": %zu, \"casts\": %zu, \"half_extent\": %.9g, \"t_max\": %.9g, \"touching\": %zu, \"flagged\": %zu, "
                "\"at_start\": %zu, \"word_sum\": %llu, \"by_axis\": [",
                mesh.size(), count, half, t_max, touching, flagged, at_start, (unsigned long long)words);
    for (int j = 0; j < 14; j++) std::printf("%s%zu", j ? ", " : "", by_axis[j]);
    std::printf("], \"records\": [");
    for (size_t i = 0; i < std::min<size_t>(count, 3); i++) {
        const lbvh_box_hit& h = hits.LocalBuffer()[i];
        std::printf("%s[%.9g, %u, %u]", i ? ", " : "", h.t, h.tri, h.axis);
    }
    std::printf("]}\n");
    return 0;
}

// `castall`: CAST_ALL (count only, one 8-byte read, fill), SortHitSegments on the device, then what the first-contact call and the
// any-contact call give on the same casts
template <class CAST, class HIT, class ALL, class FIRST, class ANY>
static int castall_report(lbvh::Context& ctx, lbvh::RaytracingMeshDrawer& drawer, const char* shape, size_t triangles, const lbvh::DataBuffer<CAST>& casts, float t_max, ALL all, FIRST first,
                          ANY any)
{
    const size_t count = casts.Size();
    lbvh::DataBuffer<uint64_t> offsets(ctx, count + 1);
    all(offsets, (lbvh::DataBuffer<HIT>*)nullptr);          // count only
    offsets.GetData();
    const uint64_t total = offsets.LocalBuffer()[count];
    lbvh::DataBuffer<HIT> hits(ctx, std::max<size_t>((size_t)total, 1));
    all(offsets, &hits);
    drawer.SortHitSegments(offsets, hits, count);
    lbvh::DataBuffer<HIT> nearest(ctx, count);
    lbvh::DataBuffer<uint32_t> flags(ctx, count);
    first(nearest);
    any(flags);
    offsets.GetData();
    hits.GetData();
    nearest.GetData();
    flags.GetData();
    const std::vector<uint64_t>& off = offsets.LocalBuffer();
    const std::vector<HIT>& rec = hits.LocalBuffer();
    size_t nonempty = 0, at_start = 0, flagged = 0, first_equal = 0;
    uint64_t longest = 0, words = 0, weighted_sum = 0;
    for (size_t q = 0; q < count; q++) {
        const uint64_t m = off[q + 1] - off[q];
        nonempty += m != 0;
        longest = std::max(longest, m);
        flagged += flags.LocalBuffer()[q];
        const HIT& n = nearest.LocalBuffer()[q];            // the least of a device-sorted segment is the first-contact record
        first_equal += m != 0 ? std::memcmp(&rec[off[q]], &n, sizeof n) == 0 : n.t == LBVH_MAX_FLOAT;
    }
    for (uint64_t i = 0; i < total; i++) {
        words += word_sum(rec[i]);
        weighted_sum += (i + 1) * (uint64_t)rec[i].tri;
        at_start += rec[i].t == 0.0f;
    }
    std::printf("{\"shape\": \"%s\", \"triangles\": %zu, \"casts\": %zu, \"t_max\": %.9g, \"total\": %llu, \"nonempty\": %zu, \"flagged\": %zu, "
                "\"first_equal\": %zu, \"longest\": %llu, \"at_start\": %zu, \"word_sum\": %llu, \"weighted_sum\": %llu, \"rows\": [",
                shape, triangles, count, t_max, (unsigned long long)total, nonempty, flagged, first_equal, (unsigned long long)longest, at_start,
                (unsigned long long)words, (unsigned long long)weighted_sum);
    for (size_t q = 0; q < std::min<size_t>(count, 3); q++) {
        std::printf("%s[", q ? ", " : "");
        for (uint64_t j = off[q]; j < off[q + 1]; j++) std::printf("%s[%.9g, %u]", j != off[q] ? ", " : "", rec[j].t, rec[j].tri);
        std::printf("]");
    }
    std::printf("]}\n");
    return 0;
}

static int castall_main(int argc, char** argv)
{
    const char* shape = argc > 2 ? argv[2] : "sphere";
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 4096;
    const uint64_t seed = argc > 4 ? strtoull(argv[4], nullptr, 10) : 3;
    const float t_max = argc > 5 ? (float)atof(argv[5]) : 2.0f;
    const std::vector<lbvh_triangle> mesh = random_mesh(4096);
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    if (std::strcmp(shape, "sphere") == 0) {
        lbvh::DataBuffer<lbvh_sphere_ray> casts(ctx, count);
        rays_into(lo, hi, seed, casts.LocalBuffer());
        for (auto& c : casts.LocalBuffer()) { c.radius = 1.5f; c.t_max = t_max; }
        casts.Sync();
        return castall_report<lbvh_sphere_ray, lbvh_hit>(
            ctx, drawer, shape, mesh.size(), casts, t_max, [&](lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_hit>* h) { drawer.SphereCastAll(casts, o, h); },
            [&](lbvh::DataBuffer<lbvh_hit>& h) { drawer.SphereCast(casts, h); }, [&](lbvh::DataBuffer<uint32_t>& f) { drawer.SphereCastAny(casts, f); });
    }
    if (std::strcmp(shape, "capsule") == 0) {
        lbvh::DataBuffer<lbvh_capsule_ray> casts(ctx, count);
        capsule_casts(lo, hi, seed, 1.5f, 4.0f, t_max, casts.LocalBuffer());
        casts.Sync();
        return castall_report<lbvh_capsule_ray, lbvh_hit>(
            ctx, drawer, shape, mesh.size(), casts, t_max, [&](lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_hit>* h) { drawer.CapsuleCastAll(casts, o, h); },
            [&](lbvh::DataBuffer<lbvh_hit>& h) { drawer.CapsuleCast(casts, h); }, [&](lbvh::DataBuffer<uint32_t>& f) { drawer.CapsuleCastAny(casts, f); });
    }
    if (std::strcmp(shape, "box") == 0) {
        lbvh::DataBuffer<lbvh_box_ray> casts(ctx, count);
        box_casts(lo, hi, seed, 1.5f, t_max, casts.LocalBuffer());
        casts.Sync();
        return castall_report<lbvh_box_ray, lbvh_box_hit>(
            ctx, drawer, shape, mesh.size(), casts, t_max, [&](lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_box_hit>* h) { drawer.BoxCastAll(casts, o, h); },
            [&](lbvh::DataBuffer<lbvh_box_hit>& h) { drawer.BoxCast(casts, h); }, [&](lbvh::DataBuffer<uint32_t>& f) { drawer.BoxCastAny(casts, f); });
    }
    if (std::strcmp(shape, "triangle") == 0) {              // `castall triangle <n> [seed] [t_max]`: the casts of `tricast`
        lbvh::DataBuffer<lbvh_tri_ray> casts(ctx, count);
        triangle_casts(lo, hi, seed, t_max, casts.LocalBuffer());
        casts.Sync();
        return castall_report<lbvh_tri_ray, lbvh_tri_cast_hit>(
            ctx, drawer, shape, mesh.size(), casts, t_max,
            [&](lbvh::DataBuffer<uint64_t>& o, lbvh::DataBuffer<lbvh_tri_cast_hit>* h) { drawer.TriangleCastAll(casts, o, h); },
            [&](lbvh::DataBuffer<lbvh_tri_cast_hit>& h) { drawer.TriangleCast(casts, h); },
            [&](lbvh::DataBuffer<uint32_t>& f) { drawer.TriangleCastAny(casts, f); });
    }
    std::fprintf(stderr, "castall: the shape is sphere, capsule, box or triangle\n");
    return 2;
}

static int crossings_main(int argc, char** argv)
{
    const size_t count = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : 65536;
    const std::vector<float> dirs = {(float)(1.0 / std::sqrt(3.0)),  (float)(1.0 / std::sqrt(3.0)),  (float)(1.0 / std::sqrt(3.0)),
                                     (float)(-1.0 / std::sqrt(14.0)), (float)(2.0 / std::sqrt(14.0)), (float)(3.0 / std::sqrt(14.0)),
                                     (float)(4.0 / std::sqrt(21.0)),  (float)(-1.0 / std::sqrt(21.0)), (float)(2.0 / std::sqrt(21.0))};
    const std::vector<lbvh_triangle> mesh = load_mesh(argc > 2 ? argv[2] : "4096");
    float lo[3], hi[3];
    mesh_box(mesh, lo, hi);
    lbvh::Context ctx(0);
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    drawer.Awake();
    lbvh::DataBuffer<lbvh_point_query> points(ctx, count);
    lbvh::DataBuffer<lbvh_ray> rays(ctx, 3 * count);
    points_around(lo, hi, 2, INFINITY, points.LocalBuffer());
    for (size_t i = 0; i < count; i++) {
        const lbvh_point_query& q = points.LocalBuffer()[i];
        for (int j = 0; j < 3; j++) {
            lbvh_ray& r = rays.LocalBuffer()[3 * i + j];
            for (int k = 0; k < 3; k++) { r.origin[k] = q.p[k]; r.dir[k] = dirs[3 * j + k]; }
            r.t_min = 0.0f;
            r.t_max = INFINITY;
        }
    }
    points.Sync();
    rays.Sync();
    lbvh::DataBuffer<uint32_t> parity(ctx, count);
    lbvh::DataBuffer<uint32_t> counts(ctx, 3 * count);
    drawer.PointCrossings(points, dirs, parity);
    drawer.CountHits(rays, counts);
    parity.GetData();
    counts.GetData();
    uint64_t count_sum = 0, parity_sum = 0;
    size_t n_inside = 0;
    bool consistent = true;
    for (size_t i = 0; i < count; i++) {
        const uint32_t p = parity.LocalBuffer()[i];
        parity_sum += p;
        n_inside += __builtin_popcount(p) >= 2;
        consistent = consistent && (p >> 3) == 0u;
        for (int j = 0; j < 3; j++) {
            const uint32_t c = counts.LocalBuffer()[3 * i + j];
            count_sum += c;
            consistent = consistent && ((p >> j) & 1u) == (c & 1u);
        }
    }
    std::printf("{\"triangles\": %zu, \"points\": %zu, \"count_sum\": %llu, \"parity_sum\": %llu, \"inside\": %zu, \"consistent\": %s}\n",
                mesh.size(), count, (unsigned long long)count_sum, (unsigned long long)parity_sum, n_inside, consistent ? "true" : "false");
    return 0;
}

// the default command: `[n] [w] [h] [dynamic]` or `obj <file.obj> [w] [h] [z]`
static int frame_main(int argc, char** argv)
{
    const bool from_obj = argc > 2 && std::strcmp(argv[1], "obj") == 0;
    const int w = from_obj ? (argc > 3 ? atoi(argv[3]) : 256) : (argc > 2 ? atoi(argv[2]) : 256);
    const int h = from_obj ? (argc > 4 ? atoi(argv[4]) : 256) : (argc > 3 ? atoi(argv[3]) : 256);
    const float cam_z = from_obj && argc > 5 ? (float)atof(argv[5]) : 300.0f;
    const std::vector<lbvh_triangle> mesh = from_obj ? lbvh::MeshTriangles(lbvh::LoadObj(argv[2]))       // MeshBufferContainer.cs:117-146
                                                     : random_mesh(argc > 1 ? (uint32_t)atoi(argv[1]) : 4096);
    const uint32_t n = (uint32_t)mesh.size();
    const bool dynamic = !from_obj && argc > 4 && std::strcmp(argv[4], "dynamic") == 0;
    lbvh::Context ctx(0);
    if (dynamic) {
        // BASELINE configs[4] in miniature: 8 rigid bodies (triangle i belongs to body i % 8), one animated frame,
        // primary rays + 2 bounces; prints a checksum of the RGBA16F image
        std::vector<uint32_t> body(n);
        for (uint32_t i = 0; i < n; i++) body[i] = i % 8;
        std::vector<float> centres(8 * 4, 0.0f);
        for (int bdy = 0; bdy < 8; bdy++) {
            centres[bdy * 4 + 0] = (bdy & 1) ? 40.0f : -40.0f;
            centres[bdy * 4 + 1] = (bdy & 2) ? 40.0f : -40.0f;
            centres[bdy * 4 + 2] = (bdy & 4) ? 40.0f : -40.0f;
        }
        lbvh::DynamicPathTracer pt(ctx, mesh, body, centres, 1e-3f, 0.7f, 3);
        pt.Animate(0.1f);
        pt.Render(camera_at(w, h, 300.0f), 2);
        pt.Image().GetData();
        uint64_t image_sum = 0;
        for (size_t i = 0; i < (size_t)w * h; i++) {
            const uint64_t px = pt.Image().LocalBuffer()[i];
            image_sum += (px & 0xFFFF) + ((px >> 16) & 0xFFFF) * 3 + ((px >> 32) & 0xFFFF) * 5 + ((px >> 48) & 0xFFFF) * 7;
        }
        std::printf("{\"triangles\": %u, \"rays\": %d, \"image_sum\": %llu}\n", n, w * h, (unsigned long long)image_sum);
        return 0;
    }
    lbvh::RaytracingMeshDrawer drawer(ctx, mesh);
    auto t0 = std::chrono::steady_clock::now();
    drawer.Awake();
    ctx.sync();
    auto t1 = std::chrono::steady_clock::now();
    const lbvh_camera cam = camera_at(w, h, cam_z);
    lbvh::Event e0(ctx), e1(ctx);
    e0.record();
    drawer.Update(cam, LBVH_TRACE_FAST);
    e1.record();
    ctx.sync();
    auto t2 = std::chrono::steady_clock::now();
    const float update_device_ms = lbvh::Event::elapsed_ms(e0, e1);
    // the same frame as three shards traced one after the other into the one buffer: must reproduce it exactly
    drawer.Hits().GetData();
    const std::vector<lbvh_hit> whole = drawer.Hits().LocalBuffer();
    drawer.Hits().Fill(0xFFFFFFFFu);
    for (uint32_t r = 0; r < 3; r++) drawer.UpdateShard(cam, r, 3, LBVH_TRACE_FAST);
    drawer.Hits().GetData();
    const bool shards_equal = std::memcmp(whole.data(), drawer.Hits().LocalBuffer().data(), whole.size() * sizeof(lbvh_hit)) == 0;
    ctx.trace_forget();
    drawer.Update(cam, LBVH_TRACE_FAST);
    drawer.Container().GetAllGpuData();          // throws on a corrupted node (MeshBufferContainer.cs:181-195)
    drawer.Hits().GetData();
    uint64_t key_sum = 0, node_sum = 0;
    for (uint32_t i = 0; i < n; i++) key_sum += drawer.Container().Keys().LocalBuffer()[i];
    for (uint32_t i = 0; i + 1 < n; i++) {
        const auto& nd = drawer.Container().BvhInternalNode().LocalBuffer()[i];
        node_sum += (uint64_t)nd.leftNode * 3 + (uint64_t)nd.rightNode * 5 + (uint64_t)nd.parent * 7 + nd.leftNodeType + nd.rightNodeType;
    }
    size_t hits = 0;
    double tsum = 0;
    for (size_t i = 0; i < (size_t)w * h; i++)
        if (drawer.Hits().LocalBuffer()[i].t < LBVH_MAX_FLOAT) { hits++; tsum += drawer.Hits().LocalBuffer()[i].t; }
    std::printf("{\"triangles\": %u, \"rays\": %d, \"awake_ms\": %.3f, \"update_ms\": %.3f, \"update_device_ms\": %.4f, "
                "\"key_sum\": %llu, \"node_sum\": %llu, \"hits\": %zu, \"t_sum\": %.6f, \"shards_equal\": %s}\n",
                n, w * h, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count(), update_device_ms, (unsigned long long)key_sum,
                (unsigned long long)node_sum, hits, tsum, shards_equal ? "true" : "false");
    return 0;
}

// lbvh::Error is a std::runtime_error, and the OBJ reader throws std::runtime_error: every failure is one line on stderr and status 1
int main(int argc, char** argv)
{
    static const struct { const char* name; int (*run)(int, char**); } commands[] = {
        {"crossings", crossings_main}, {"points", points_main}, {"knn", knn_main},   {"khits", khits_main}, {"gather", gather_main}, {"sortedhits", sortedhits_main}, {"sortedrecords", sortedrecords_main},
        {"sweep", sweep_main},         {"capsule", capsule_main}, {"boxcast", boxcast_main}, {"tricast", tricast_main}, {"castall", castall_main},         {"overlaps", overlaps_main}, {"tris", tris_main}, {"trisegs", trisegs_main}, {"sections", sections_main}, {"shapes", shapes_main}, {"contacts", contacts_main}, {"boxcontacts", boxcontacts_main}, {"segclosest", segclosest_main}, {"triclosest", triclosest_main}, {"triprox", triprox_main}, {"regions", regions_main}, {"rays", rays_main}, {"sort", sort_main},   {"multi", multi_main}};
    try {
        for (const auto& c : commands)
            if (argc > 1 && std::strcmp(argv[1], c.name) == 0) return c.run(argc, argv);
        return frame_main(argc, argv);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
