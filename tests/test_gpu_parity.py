"""GPU parity: every stage of the hot path, called through the C ABI (liblbvh.so), against the
CPU oracle on the same seeded inputs.  Bit-exact for keys, indices and node arrays; boxes compared
as floats (-0 == +0); hit t within 1e-5 (north_star), in practice bit-equal
because both sides compute in strict fp32 without FMA contraction."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as O
from query_support import H, N, _random_ray_states, _splitmix_mesh, words
from unitysimpleraytracing_amd import layouts as L
from unitysimpleraytracing_amd import scenes

pytestmark = pytest.mark.gpu

F = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def up(ctx, arr, dtype=None):
    a = np.ascontiguousarray(arr, dtype=dtype)
    b = H().DataBuffer(ctx, max(len(a), 1), a.dtype)
    b.local[: len(a)] = a
    b.sync()
    return b


# ---- a-2..a-5 sort ---------------------------------------------------------------------------------

def sort_inputs(count, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "random":
        keys = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    elif kind == "morton_pads":
        keys = (rng.integers(0, 1 << 30, size=count, dtype=np.uint64) >> 10 << 10).astype(np.uint32)
        keys[count - count // 7:] = F
    elif kind == "all_equal":
        keys = np.full(count, 0xDEADBEEF, dtype=np.uint32)
    elif kind == "few_digits":
        keys = rng.integers(0, 4, size=count, dtype=np.uint64).astype(np.uint32) * 0x01010101
    else:
        keys = np.arange(count, dtype=np.uint32)[::-1].copy()
    vals = rng.permutation(count).astype(np.uint32)
    return keys, vals


def gpu_sort(ctx, keys, vals):
    kb, vb = up(ctx, keys, np.uint32), up(ctx, vals, np.uint32)
    N().check(ctx.handle, N().lib.lbvh_sort_pairs(ctx.handle, kb.device, vb.device, len(keys)))
    k, v = kb.get_data()[: len(keys)].copy(), vb.get_data()[: len(keys)].copy()
    kb.dispose(); vb.dispose()
    return k, v


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 12289, 100003,
                                   524288, 1000000 + 37, (1 << 21) - 1, 1 << 21, (1 << 21) + 1, 8192 * 129 - 5,
                                   4096 * 1024 + 4095, 3 * 8192 * 16 * 8 + 1])
def test_sort_random_sizes(ctx, count):
    keys, vals = sort_inputs(count, count, "random")
    gk, gv = gpu_sort(ctx, keys, vals)
    ok, ov = O.sort_pairs(keys, vals)
    assert (gk == ok).all() and (gv == ov).all()


@pytest.mark.parametrize("kind", ["morton_pads", "all_equal", "few_digits", "reversed"])
@pytest.mark.parametrize("count", [5000, 131072, 300001])
def test_sort_stability_and_skew(ctx, kind, count):
    keys, vals = sort_inputs(count, 17, kind)
    gk, gv = gpu_sort(ctx, keys, vals)
    ok, ov = O.sort_pairs(keys, vals)
    assert (gk == ok).all() and (gv == ov).all()


def test_sort_single_ticket_queue_mode():
    """contexts that are not the full 8-XCD device behind an unmasked stream take tiles in plain ticket order
    (one queue).  lbvh_debug_switch(LBVH_DEBUG_SORT_QUEUES, 1) forces that mode on this box: same results, sizes beyond the
    point where the 8-queue form could have stranded tiles (> 9 M keys)."""
    c1 = H().Context(0)
    try:
        c1.debug_switch(N().DEBUG_SWITCH_SORT_QUEUES, 1)
        for count, kind in ((100003, "random"), (1 << 21, "morton_pads"), (12_000_001, "random")):
            keys, vals = sort_inputs(count, count % 97, kind)
            k, v = gpu_sort(c1, keys, vals)
            ok, ov = O.sort_pairs(keys, vals)
            assert (k == ok).all() and (v == ov).all()
    finally:
        c1.close()


# ---- round 5: the two-level form (one MSD pass + one bucket-local kernel) for 2^15 <= count < 2^21 --------------------------------

@pytest.fixture
def sort_form(ctx):
    """forces the sort's form on the shared context for one test (lbvh_debug_switch LBVH_DEBUG_SORT_FORM) and restores the default"""
    def force(form):
        ctx.debug_switch(N().DEBUG_SWITCH_SORT_FORM, form)
    yield force
    ctx.debug_switch(N().DEBUG_SWITCH_SORT_FORM, 0)


@pytest.mark.parametrize("count", [1 << 15, (1 << 15) + 1, 40000, 65536 + 63, 100003, 262144, 524288 - 1, 1000448, 1500001, (1 << 21) - 1])
def test_sort_two_level_random_sizes(ctx, sort_form, count):
    """Both forms on the same input, each forced: the unique stable sort either way (oracle), for sizes across the form's range —
    buckets of ~128 .. ~8 192 pairs (uniform 32-bit keys: the bucket digit is the top byte)."""
    keys, vals = sort_inputs(count, count, "random")
    ok, ov = O.sort_pairs(keys, vals)
    for form in (2, 1):
        sort_form(form)
        gk, gv = gpu_sort(ctx, keys, vals)
        assert (gk == ok).all() and (gv == ov).all(), form


@pytest.mark.parametrize("kind", ["morton_pads", "all_equal", "few_digits", "reversed", "one_bucket_low_bits", "two_hot_buckets"])
@pytest.mark.parametrize("count", [40000, 131072, 300001])
def test_sort_two_level_skewed_buckets(ctx, sort_form, kind, count):
    """The two-level form forced on inputs whose buckets do NOT fit one workgroup's registers (everything in one bucket, a few
    hot buckets, duplicates only): the bucket kernel's chunk-by-chunk path through global memory — three passes, and four in the
    last bucket (0xDEADBEEF, the pads) with its copy back.  Stable: the values are a permutation, equal keys keep their order."""
    if kind == "one_bucket_low_bits":
        rng = np.random.default_rng(5)
        keys = (0x42000000 | rng.integers(0, 1 << 24, size=count, dtype=np.uint64)).astype(np.uint32)
        keys[: count // 3] = keys[count // 3: 2 * (count // 3)]      # duplicates too
        vals = rng.permutation(count).astype(np.uint32)
    elif kind == "two_hot_buckets":
        rng = np.random.default_rng(6)
        keys = rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
        hot = rng.random(count)
        keys[hot < 0.45] = (0x07000000 | (keys[hot < 0.45] & 0x00FFFFFF))
        keys[hot > 0.60] = (0xFF000000 | (keys[hot > 0.60] & 0x00FFFFFF))
        vals = rng.permutation(count).astype(np.uint32)
    else:
        keys, vals = sort_inputs(count, 17, kind)
    ok, ov = O.sort_pairs(keys, vals)
    sort_form(2)
    gk, gv = gpu_sort(ctx, keys, vals)
    assert (gk == ok).all() and (gv == ov).all()


def test_sort_form_follows_the_last_sorts_largest_bucket():
    """The default (no switch): a context's first sort takes the four passes and leaves its largest bucket behind; after a
    uniform input the next sort is two-level, after a skewed one it is four passes again — seen in the per-kernel profile.  Every
    result is the oracle's whatever the form."""
    c = H().Context(0)
    try:
        def kernels(keys, vals):
            kb, vb = up(c, keys, np.uint32), up(c, vals, np.uint32)
            c.profile_begin()
            N().check(c.handle, N().lib.lbvh_sort_pairs(c.handle, kb.device, vb.device, len(keys)))
            prof = c.profile_end()
            k, v = kb.get_data()[: len(keys)].copy(), vb.get_data()[: len(keys)].copy()
            kb.dispose(); vb.dispose()
            ok, ov = O.sort_pairs(keys, vals)
            assert (k == ok).all() and (v == ov).all()
            return prof
        uniform = sort_inputs(300001, 1, "random")
        skewed = sort_inputs(300001, 2, "all_equal")
        forms = []
        seq = [uniform] * 4 + [skewed, skewed] + [uniform] * 4 + [skewed, uniform] * 4
        for keys, vals in seq:
            prof = kernels(keys, vals)
            forms.append("two" if any("sort_bucket_kernel" in k for k in prof) else "four")
        # round 6: THREE sorts in a row must have left a hint in order (lbvh_sort.hip kSortStreak).  First: nothing known -> four, and
        # three more while the streak builds; then two.  The skewed input after a spread streak is still sorted two-level ONCE (the
        # bucket kernel's slow path), then four; three spread sorts later two again; an input that ALTERNATES never leaves the
        # four passes (it paid the slow path on every second sort)
        assert forms == ["four"] * 3 + ["two"] + ["two", "four"] + ["four"] * 3 + ["two"] + ["two", "four"] + ["four"] * 6, forms
    finally:
        c.close()


def test_sort_pairs_of_morton_codes_with_pads_goes_two_level_without_a_hint():
    """lbvh_sort_pairs has no key_bits hint: its fine bins are the keys' top 12 bits.  Morton codes below 2^30 plus 0xFFFFFFFF pads
    (the reference's own call sequence, ComputeBufferSorter.Sort on the padded key buffer) fill a quarter of them and would fill 64
    top-byte buckets of 16 k and more; the balanced buckets (ranges of fine bins of about count / 256 pairs) take them all the same:
    the first sorts measure (three in a row with every bucket inside one workgroup's registers), the next ones are two-level.
    Results are the oracle's."""
    c = H().Context(0)
    try:
        rng = np.random.default_rng(5)
        n = 1 << 20
        keys = rng.integers(0, 1 << 30, n, dtype=np.uint32)
        keys[n - 1000:] = 0xFFFFFFFF
        keys[::4097] = (255 << 22) | 5          # company for the pads in the last bucket
        vals = rng.permutation(n).astype(np.uint32)
        ok, ov = O.sort_pairs(keys, vals)
        forms = []
        for _ in range(5):
            kb, vb = up(c, keys, np.uint32), up(c, vals, np.uint32)
            c.profile_begin()
            N().check(c.handle, N().lib.lbvh_sort_pairs(c.handle, kb.device, vb.device, n))
            prof = c.profile_end()
            k, v = kb.get_data()[:n].copy(), vb.get_data()[:n].copy()
            kb.dispose(); vb.dispose()
            assert (k == ok).all() and (v == ov).all()
            forms.append("two" if any("sort_bucket_kernel" in q for q in prof) else "four")
        assert forms == ["four"] * 3 + ["two"] * 2, forms
    finally:
        c.close()


def test_rebuild_with_the_two_level_sort_is_bit_exact(ctx, sort_form):
    """lbvh_build_scene with the sort's form forced either way (the build's bucket digit is bits 22..29: Morton codes below 2^30,
    the pads and nothing else in the last bucket): keys, indices and every node word identical to the oracle on the tiled-torus
    scene (1/8 size), a scene with every triangle twice and a scene inside ONE Morton cell (one bucket: the slow path)."""
    scenes_ = {"torus": scenes.tiled_torus(nu=40, nv=25), "doubled": None, "one_cell": None}
    t = scenes.tiled_torus(nu=24, nv=16, grid=3)
    t[1::2] = t[0::2][: len(t[1::2])]
    scenes_["doubled"] = t
    small = scenes.random_triangles(60000, seed=9, extent=0.1, edge=0.01)
    scenes_["one_cell"] = small
    for name, tris in scenes_.items():
        b = None
        for form in (2, 1, 2):
            sort_form(form)
            d = H().RaytracingMeshDrawer(ctx, tris).awake()
            d.rebuild()
            c = d.container
            c.get_all_gpu_data()
            if b is None:
                b = O.Built(tris, capacity=c.capacity, threads=8)
            assert (c.keys.local == b.keys).all() and (c.triangle_index.local == b.indices).all(), (name, form)
            assert (words(c.bvh_internal_node.local) == words(b.internal)).all() and (words(c.bvh_leaf_node.local) == words(b.leaf)).all(), (name, form)
            d.on_destroy()


def test_sort_count_zero_and_repeat(ctx):
    kb, vb = up(ctx, np.zeros(4, np.uint32)), up(ctx, np.zeros(4, np.uint32))
    N().check(ctx.handle, N().lib.lbvh_sort_pairs(ctx.handle, kb.device, vb.device, 0))
    keys, vals = sort_inputs(70000, 2, "random")
    a = gpu_sort(ctx, keys, vals)
    b = gpu_sort(ctx, keys, vals)        # scratch reuse
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def _rocprim():
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "oracle", "librocprim_sort.so")
    assert os.path.exists(path), "build it with __graft_entry__.build() (oracle/Makefile)"
    lib = ctypes.CDLL(path)
    lib.rocprim_sort_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    lib.rocprim_sort_pairs.restype = ctypes.c_int
    return lib


@pytest.mark.parametrize("kind,count", [("random", 1 << 20), ("random", 3 * 8192 * 16 + 777), ("morton_pads", 1000000 + 37),
                                        ("few_digits", 300001), ("all_equal", 70000), ("reversed", 131072), ("random", 1 << 24)])
def test_sort_equals_rocprim_radix_sort(ctx, kind, count):
    """a THIRD implementation of "stable sort of (key, value) pairs", written by someone else and
    running on the same GPU — rocPRIM's DeviceRadixSort::SortPairs through hipCUB (oracle/rocprim_sort.hip, tests only).
    Keys AND values of lbvh_sort_pairs equal it on random, duplicate-heavy, padded, all-equal and reversed inputs, up
    to 16 M pairs (the oracle is not in this comparison at all)."""
    keys, vals = sort_inputs(count, count % 1013, kind)
    gk, gv = gpu_sort(ctx, keys, vals)
    rk, rv = keys.copy(), vals.copy()
    rc = _rocprim().rocprim_sort_pairs(rk.ctypes.data, rv.ctypes.data, count)
    assert rc == 0, f"hip error {rc} inside the rocPRIM checker"
    assert (gk == rk).all() and (gv == rv).all()


def test_sort_16m_properties(ctx):
    """cfg4 size (16 M keys): sortedness, stability and permutation without the oracle in the loop."""
    count = 16_000_000
    rng = np.random.default_rng(3)
    keys = (rng.integers(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)) >> 8 << 8   # duplicates
    vals = np.arange(count, dtype=np.uint32)
    gk, gv = gpu_sort(ctx, keys, vals)
    assert (gk[1:] >= gk[:-1]).all()
    assert (keys[gv] == gk).all()                                 # pairs stayed together
    eq = gk[1:] == gk[:-1]
    assert (gv[1:][eq] > gv[:-1][eq]).all()                       # stable: input order inside equal keys
    assert np.bincount(gv, minlength=count).max() == 1            # a permutation


# ---- a-1 Morton / AABB ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,cap", [(1, 1024), (4096, 4096), (4097, 5120), (12800, 13312)])
def test_morton_aabb(ctx, n, cap):
    tris = scenes.random_triangles(n, seed=n) if n != 12800 else scenes.grid_scene()
    c = H().MeshBufferContainer(ctx, tris, capacity=cap)
    ok, oi, oa = O.morton_aabb(tris, capacity=cap)
    assert (c.keys.get_data() == ok).all()
    assert (c.triangle_index.get_data() == oi).all()
    ga = c.triangle_aabb.get_data()
    assert (ga["min"][:n] == oa["min"][:n]).all() and (ga["max"][:n] == oa["max"][:n]).all()
    assert (ga["_dummy0"][:n] == 0).all() and (ga["_dummy1"][:n] == 0).all()
    c.dispose()


def test_morton_clamps_outside_scene_box(ctx):
    tris = scenes.random_triangles(3000, seed=8, extent=400.0)     # well outside +-125
    c = H().MeshBufferContainer(ctx, tris)
    ok, _, _ = O.morton_aabb(tris, capacity=c.capacity)
    assert (c.keys.get_data() == ok).all()
    c.dispose()


# ---- a-6 DistributeKeys ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 2047, 2048, 2049, 4096, 100001, 1000000])
def test_distribute_keys(ctx, n):
    rng = np.random.default_rng(n)
    keys = np.sort((rng.integers(0, 1 << 30, size=n, dtype=np.uint64) >> np.uint64(rng.integers(0, 16))).astype(np.uint32))
    buf = np.concatenate([keys, np.full(100, F, dtype=np.uint32)])
    kb = up(ctx, buf)
    N().check(ctx.handle, N().lib.lbvh_distribute_keys(ctx.handle, kb.device, n))
    assert (kb.get_data() == O.distribute_keys(buf, n)).all()
    kb.dispose()


def test_distribute_all_equal_and_already_unique(ctx):
    for keys in (np.full(5000, 77, dtype=np.uint32), np.arange(5000, dtype=np.uint32) * 3 + 9):
        kb = up(ctx, keys)
        N().check(ctx.handle, N().lib.lbvh_distribute_keys(ctx.handle, kb.device, len(keys)))
        assert (kb.get_data() == O.distribute_keys(keys, len(keys))).all()
        kb.dispose()


# ---- a-7 tree + a-8 refit -----------------------------------------------------------------------------------

def gpu_tree(ctx, keys, n, cap):
    kb = up(ctx, keys, np.uint32)
    ib = H().DataBuffer(ctx, cap, L.INTERNAL_NODE, L.NULL)
    lb = H().DataBuffer(ctx, cap, L.LEAF_NODE, L.NULL)
    N().check(ctx.handle, N().lib.lbvh_build_tree(ctx.handle, n, kb.device, ib.device, lb.device))
    return kb, ib, lb


@pytest.mark.parametrize("n", [2, 3, 6, 8, 1000, 4096, 65537, 1000000])
def test_build_tree_bit_exact(ctx, n):
    rng = np.random.default_rng(n + 1)
    raw = np.sort((rng.integers(0, 1 << 30, size=n, dtype=np.uint64) >> np.uint64(rng.integers(0, 12))).astype(np.uint32))
    keys = O.distribute_keys(raw, n)
    cap = n + 5
    kb, ib, lb = gpu_tree(ctx, keys, n, cap)
    oi, ol = O.build_tree(keys, n, capacity=cap, threads=8)
    assert (words(ib.get_data()) == words(oi)).all()
    assert (words(lb.get_data()) == words(ol)).all()
    for b in (kb, ib, lb):
        b.dispose()


def _wide_node_keys(shape, n):
    i = np.arange(n, dtype=np.uint64)
    if shape == "dense":                       # every range a power of two: searches end exactly on window borders
        k = i
    elif shape == "two_islands":               # the root splits 257 leaves from the left end
        k = np.where(i < 257, i, (1 << 31) + i)
    elif shape == "doubling_clusters":         # clusters of 1, 2, 4, ... keys, each under its own high bit pattern
        c = np.floor(np.log2(i + 1)).astype(np.uint64)
        k = (c << np.uint64(24)) + (i + 1 - (np.uint64(1) << c))
    elif shape == "sparse_top":                # long runs that differ in the low bits only, then one far key
        k = (i >> np.uint64(13) << np.uint64(20)) + (i & np.uint64(8191))
    else:                                      # "right_heavy": ranges that grow towards the END of the array (d = -1 searches)
        k = (np.uint64(1) << np.uint64(32)) - np.uint64(1) - _wide_node_keys("doubling_clusters", n)[::-1].astype(np.uint64)
    k = k.astype(np.uint32)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    return k


@pytest.mark.parametrize("shape", ["dense", "two_islands", "doubling_clusters", "sparse_top", "right_heavy"])
@pytest.mark.parametrize("n", [257, 65536, 200001])
def test_build_tree_wide_nodes_bit_exact(ctx, shape, n):
    """Nodes whose searches leave the workgroup's LDS key window are searched by the whole wave with a 64-ary search
    (wide_node_range / wide_node_split, lbvh_build.hip): same ranges and splits as BVH.compute:35-92 on key sets built to put range
    ends and splits on, just before and just after the window borders, in both search directions."""
    keys = _wide_node_keys(shape, n)
    cap = n + 3
    kb, ib, lb = gpu_tree(ctx, keys, n, cap)
    oi, ol = O.build_tree(keys, n, capacity=cap, threads=8)
    assert (words(ib.get_data()) == words(oi)).all()
    assert (words(lb.get_data()) == words(ol)).all()
    for b in (kb, ib, lb):
        b.dispose()


def _bitmap_key_sets():
    import importlib
    tb = importlib.import_module("test_tree_bitmaps")
    sets = [(name, np.sort(k)) for name, k in tb.key_sets()]
    rng = np.random.default_rng(77)
    # raw keys with EQUAL neighbours in some windows only (lbvh_build_tree on a caller's keys): those workgroups take the probe
    # loops, the others the lookups; a run of equal keys across a window border; all keys equal
    mixed = np.sort(rng.integers(0, 1 << 22, 9000, dtype=np.uint32))
    mixed[3000:3400] = mixed[3000]
    mixed[700:703] = mixed[700]
    sets.append(("equal_runs_in_some_windows", np.sort(mixed)))
    sets.append(("all_equal", np.full(2000, 12345, dtype=np.uint32)))
    big = np.unique(rng.integers(0, 1 << 30, 400000, dtype=np.uint32))
    sets.append(("random_400k", big))
    return sets


@pytest.mark.parametrize("name", [n for n, _ in _bitmap_key_sets()])
def test_build_tree_search_free_form_on_adversarial_key_sets(ctx, name):
    """The key sets of tests/test_tree_bitmaps.py (the CPU model of the tree kernel's bitmap lookups) through lbvh_build_tree on the
    GPU, plus raw keys with equal neighbours — in some windows only, across a window border, everywhere: such windows fall back to
    the reference's probe loops (tree_body) — every node and leaf word against the oracle (BVH.compute:35-149)."""
    keys = dict(_bitmap_key_sets())[name]
    n = len(keys)
    cap = n + 7
    kb, ib, lb = gpu_tree(ctx, keys, n, cap)
    oi, ol = O.build_tree(keys, n, capacity=cap, threads=8)
    gi, gl = ib.get_data().copy(), lb.get_data().copy()
    if len(np.unique(keys)) == n:
        assert (words(gi) == words(oi)).all(), name
        assert (words(gl) == words(ol)).all(), name
    else:
        # Equal keys make TreeConstructor write a malformed tree (the reason DistributeKeys exists, MeshBufferContainer.cs:154-169):
        # several nodes name the same child, and whose `parent` word survives is the reference's own race (BVH.compute:126,144 — the
        # oracle runs the nodes in index order, the GPU in any).  Every word a node writes about ITSELF, every leaf word, and the
        # parent word of every child that exactly one node names are compared.
        own = [0, 1, 2, 3, 5]
        assert (words(gi).reshape(-1, 6)[:, own] == words(oi).reshape(-1, 6)[:, own]).all(), name
        inner = oi[: n - 1]
        named = np.concatenate([inner["leftNode"][inner["leftNodeType"] == L.INTERNAL], inner["rightNode"][inner["rightNodeType"] == L.INTERNAL]])
        named = named[named < n - 1]
        once = np.nonzero(np.bincount(named, minlength=cap) == 1)[0]
        assert (gi["parent"][once] == oi["parent"][once]).all(), name
        never = np.nonzero(np.bincount(named, minlength=cap) == 0)[0]
        assert (gi["parent"][never] == oi["parent"][never]).all(), name          # (untouched: the fill value)
        leaf_named = np.concatenate([inner["leftNode"][inner["leftNodeType"] == L.LEAF], inner["rightNode"][inner["rightNodeType"] == L.LEAF]])
        leaf_named = leaf_named[leaf_named < n]
        lonce = np.nonzero(np.bincount(leaf_named, minlength=cap) <= 1)[0]
        assert (words(gl).reshape(-1, 2)[lonce] == words(ol).reshape(-1, 2)[lonce]).all(), name
    for b in (kb, ib, lb):
        b.dispose()


def test_build_tree_known_answer(ctx):
    keys = np.array([0, 1, 3, 4, 18, 23, 24, 29], dtype=np.uint32)
    kb, ib, lb = gpu_tree(ctx, keys, 8, 8)
    inner = words(ib.get_data()).reshape(-1, 6)[:7].tolist()
    assert inner == [[3, 0, 4, 0, F, 0], [0, 1, 1, 1, 2, 1], [1, 0, 2, 1, 3, 2], [2, 0, 3, 1, 0, 3],
                     [5, 0, 6, 0, 0, 4], [4, 1, 5, 1, 4, 5], [6, 1, 7, 1, 4, 6]]
    assert words(lb.get_data()).reshape(-1, 2).tolist() == [[1, 0], [1, 1], [2, 2], [3, 3], [5, 4], [5, 5],
                                                            [6, 6], [6, 7]]


def test_stage_argument_errors(ctx):
    n_ = N()
    kb = up(ctx, np.zeros(8, np.uint32))
    ib = H().DataBuffer(ctx, 8, L.INTERNAL_NODE, L.NULL)
    lb = H().DataBuffer(ctx, 8, L.LEAF_NODE, L.NULL)
    assert n_.lib.lbvh_build_tree(ctx.handle, 1, kb.device, ib.device, lb.device) == -1     # n < 2
    assert b"n >= 2" in n_.lib.lbvh_last_error(ctx.handle)
    assert n_.lib.lbvh_build_tree(ctx.handle, 4, None, ib.device, lb.device) == -1
    assert n_.lib.lbvh_sort_pairs(ctx.handle, None, None, 10) == -1
    f3 = (C.c_float * 3)(0, 0, 0)
    assert n_.lib.lbvh_morton_aabb(ctx.handle, None, 10, 5, f3, f3, kb.device, kb.device, None) == -1  # n > capacity
    with pytest.raises(n_.LbvhError):
        n_.check(ctx.handle, n_.lib.lbvh_refit(ctx.handle, 0, None, None, None, None, None))
    # the derived traversal scene indexes nodes and triangles with one 31-bit line index: 2^30 triangles are refused
    # before anything is allocated or launched
    d = H().RaytracingMeshDrawer(ctx, scenes.random_triangles(64, seed=1)).awake()
    s = d.container.scene()
    s.n = 1 << 30
    assert n_.lib.lbvh_build_fast_scene(ctx.handle, C.byref(s), f3, f3) == -1
    assert b"s.n" in n_.lib.lbvh_last_error(ctx.handle)
    d.on_destroy()


def build_both(ctx, tris, cap=None):
    d = H().RaytracingMeshDrawer(ctx, tris, cap).awake()
    c = d.container
    b = O.Built(tris, capacity=c.capacity, threads=8)
    return d, c, b


def assert_build_equal(c, b):
    bad_leaf, bad_inner = c.get_all_gpu_data()
    assert len(bad_leaf) == 0 and len(bad_inner) == 0             # MeshBufferContainer.cs:181-195
    n = b.n
    assert (c.keys.local == b.keys).all()
    assert (c.triangle_index.local == b.indices).all()
    assert (words(c.bvh_internal_node.local) == words(b.internal)).all()
    assert (words(c.bvh_leaf_node.local) == words(b.leaf)).all()
    assert (c.bvh_data.local["min"][: n - 1] == b.bvh["min"][: n - 1]).all()
    assert (c.bvh_data.local["max"][: n - 1] == b.bvh["max"][: n - 1]).all()
    assert (c.bvh_data.local["_dummy0"][: n - 1] == 0).all()


def test_cfg4_sixteen_million_triangles_on_one_gpu(ctx):
    """BASELINE configs[3]'s mesh (400x160 quads x 125 tiles) on one GPU: whole build bit-exact, traversal modes agree."""
    tris = scenes.tiled_torus(nu=400, nv=160)
    assert len(tris) == 16_000_000
    d, c, b = build_both(ctx, tris)
    assert_build_equal(c, b)
    cam = scenes.camera(480, 270, (0.0, 0.0, 250.0))
    d.update(cam, mode=L.TRACE_FAST)
    fast = d.hits()
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref = d.hits()
    assert (fast["t"] == ref["t"]).all()
    oh, _ = O.trace_primary(b, cam, step=(4, 4), threads=O.num_threads())
    assert (oh["t"] == ref["t"][::4, ::4][: oh.shape[0], : oh.shape[1]]).all()
    # the one-call rebuild at this size (two streams after the sort: beyond the merged launches' limit), poisoned node arrays
    c.bvh_internal_node.fill_u32(0x1357246, mirror=False)
    c.bvh_leaf_node.fill_u32(0x2468135, mirror=False)
    d.rebuild()
    assert_build_equal(c, b)
    d.update(cam, mode=L.TRACE_FAST)
    assert (d.hits()["t"] == ref["t"]).all()
    d.on_destroy()


@pytest.mark.parametrize("n,cap", [(2, None), (3, 8), (255, None), (256, 300), (257, None), (1023, 1024), (1024, None), (1025, 2048),
                                   (2047, None), (2048, 2049), (2049, None), (4097, 5000), (65_537, None)])
def test_build_scene_at_chunk_and_level_borders(ctx, n, cap):
    """The one-call rebuild (merged launches) where its pieces change shape: one / two workgroups of the 256-node tree kernel, the
    1024-leaf chunks of the gather (level 10 of the hierarchy: the top-levels workgroup appears at 1025 leaves), the 2048-key
    chunks of DistributeKeys, pad slots behind the tree (capacity > n) — poisoned node arrays, every word against the oracle, and
    the traced frame against the reference walk."""
    tris = scenes.random_triangles(n, seed=1000 + n, extent=100.0, edge=6.0)
    d, c, b = build_both(ctx, tris, cap)
    cam = scenes.camera(96, 64, (0.0, 0.0, 240.0))
    for rep in range(2):
        c.bvh_internal_node.fill_u32(0x3456789 + rep, mirror=False)
        c.bvh_leaf_node.fill_u32(0xABCDEF0 + rep, mirror=False)
        c.bvh_data.fill_u32(0x7FC00000, mirror=False)
        d.rebuild()
        assert_build_equal(c, b)
        d.update(cam, mode=L.TRACE_FAST)
        fast = d.hits()
        d.update(cam, mode=L.TRACE_REFERENCE)
        assert (fast["t"] == d.hits()["t"]).all()
    d.on_destroy()


@pytest.mark.parametrize("n", [2_097_152, 2_097_153])
def test_build_scene_on_both_sides_of_the_merged_launch_limit(ctx, n):
    """lbvh_build_scene runs the chain after the sort as three merged launches while the self-scanning apply passes cover the
    scene (2048 chunks of 1024 leaves), and as two streams beyond: the last size of the one form and the first of the other,
    poisoned arrays, against the oracle word for word, and the traced frame of the derived scene against the reference walk."""
    tris = scenes.random_triangles(n, seed=77, extent=118.0, edge=0.8)
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(240, 135, (0.0, 0.0, 255.0))
    for rep in range(4):                                              # (two streams: plain, captured, replayed, replayed)
        c.bvh_internal_node.fill_u32(0x2345678 + rep, mirror=False)
        c.bvh_leaf_node.fill_u32(0x9ABCDEF + rep, mirror=False)
        c.bvh_data.fill_u32(0x7FC00000, mirror=False)
        c.keys.fill_u32(0, mirror=False)
        d.rebuild()
        assert_build_equal(c, b)
        d.update(cam, mode=L.TRACE_FAST)
        fast = d.hits()
        d.update(cam, mode=L.TRACE_REFERENCE)
        assert (fast["t"] == d.hits()["t"]).all()
    d.on_destroy()


@pytest.mark.parametrize("scene", ["cfg1", "grid", "torus64k", "tiny2", "tiny3"])
def test_full_build_bit_exact(ctx, scene):
    tris = {"cfg1": lambda: scenes.random_triangles(4096, seed=1), "grid": scenes.grid_scene,
            "torus64k": lambda: scenes.tiled_torus(grid=2), "tiny2": lambda: scenes.random_triangles(2, seed=5),
            "tiny3": lambda: scenes.random_triangles(3, seed=6)}[scene]()
    d, c, b = build_both(ctx, tris)
    assert_build_equal(c, b)
    d.on_destroy()


@pytest.mark.parametrize("scene", ["cfg1", "torus64k", "rand300k"])
def test_build_scene_one_call_equals_the_staged_chain(ctx, scene):
    """lbvh_build_scene (two concurrent lanes after the sort) against the oracle and against the staged calls."""
    tris = {"cfg1": lambda: scenes.random_triangles(4096, seed=1), "torus64k": lambda: scenes.tiled_torus(grid=2),
            "rand300k": lambda: scenes.random_triangles(300_000, seed=9, extent=110.0, edge=1.5)}[scene]()
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(200, 150, (0.0, 0.0, 260.0))
    d.update(cam, mode=L.TRACE_FAST)
    staged = d.hits()
    for rep in range(3):
        c.bvh_data.fill_u32(0x7FC00000, mirror=False)
        c.keys.fill_u32(0, mirror=False)
        # LBVH_BUILD_RESET_NODES refills only what the tree kernel does not write (slots past the tree, the root's parent):
        # whatever stood in the arrays before, every word of all capacity slots must come out as a fresh build's
        c.bvh_internal_node.fill_u32(0x1234567 + rep, mirror=False)
        c.bvh_leaf_node.fill_u32(0x89ABCDE + rep, mirror=False)
        d.rebuild()                                   # lbvh_build_scene
        assert_build_equal(c, b)
        d.update(cam, mode=L.TRACE_FAST)
        one = d.hits()
        assert (one["t"] == staged["t"]).all() and (one["tri"] == staged["tri"]).all()
        d.update(cam, mode=L.TRACE_REFERENCE)
        assert (d.hits()["t"] == one["t"]).all()
    d.rebuild(staged=True)
    assert_build_equal(c, b)
    d.on_destroy()


def test_build_scene_graph_replay_survives_other_scenes_and_scratch_growth(ctx):
    """lbvh_build_scene replays a captured graph for repeated arguments; a bigger scene in between regrows the
    context's scratch, so the first scene's graph must be re-captured, not replayed with stale pointers."""
    small = scenes.random_triangles(20_000, seed=31, extent=80.0, edge=4.0)
    big = scenes.random_triangles(1_500_000, seed=32, extent=115.0, edge=1.0)
    ds, cs, bs = build_both(ctx, small)
    for _ in range(3):
        ds.rebuild()
    assert_build_equal(cs, bs)
    db, cb, bb = build_both(ctx, big)                 # every scratch buffer grows
    for _ in range(3):
        db.rebuild()
    assert_build_equal(cb, bb)
    cam = scenes.camera(160, 120, (0.0, 0.0, 240.0))
    for _ in range(3):
        cs.bvh_data.fill_u32(0x7FC00000, mirror=False)
        ds.rebuild()
    assert_build_equal(cs, bs)
    ds.update(cam, mode=L.TRACE_FAST)
    fast = ds.hits()
    ds.update(cam, mode=L.TRACE_REFERENCE)
    assert (fast["t"] == ds.hits()["t"]).all()
    db.rebuild()
    assert_build_equal(cb, bb)
    ds.on_destroy()
    db.on_destroy()


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16385, 65537, 131071])
def test_build_at_boundary_sizes(ctx, n):
    """Triangle counts around the wave / workgroup / refit-block / range-level boundaries, through the staged calls
    and twice through lbvh_build_scene (second call = graph replay), every array compared with the oracle."""
    tris = scenes.random_triangles(n, seed=1000 + n, extent=100.0, edge=2.5)
    d, c, b = build_both(ctx, tris)
    assert_build_equal(c, b)
    for _ in range(2):
        c.bvh_data.fill_u32(0x7FC00000, mirror=False)
        c.keys.fill_u32(0, mirror=False)
        d.rebuild()
        assert_build_equal(c, b)
    cam = scenes.camera(96, 64, (0.0, 0.0, 260.0))
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref = d.hits()
    for _ in range(2):
        d.update(cam, mode=L.TRACE_FAST)
        assert (d.hits()["t"] == ref["t"]).all()
    d.on_destroy()


def test_refit_race_stress(ctx):
    """Many small trees, repeated: the flag hand-off must never read a stale sibling box."""
    for rep in range(30):
        tris = scenes.random_triangles(700 + 37 * rep, seed=100 + rep, extent=20.0)
        d, c, b = build_both(ctx, tris)
        assert_build_equal(c, b)
        d.rebuild()                               # flags re-zeroed per build
        assert_build_equal(c, b)
        d.on_destroy()


@pytest.mark.parametrize("n", [1025, 5000, 70000, 300001])
def test_refit_does_not_depend_on_the_roots_parent_word_or_stale_boxes(ctx, n):
    """The root's parent word is never written by ConstructTree (BVH.compute:126,144): whatever the caller's buffer
    held there must not matter, and every node box must be rewritten (no reliance on an earlier build's boxes)."""
    tris = scenes.random_triangles(n, seed=n, extent=90.0, edge=3.0)
    d, c, b = build_both(ctx, tris)
    h, nn = ctx.handle, N()
    nodes = c.bvh_internal_node.get_data()
    for garbage in (0, 7, n // 2, n - 2):
        nodes["parent"][0] = garbage
        c.bvh_internal_node.sync()
        c.bvh_data.fill_u32(0x7FC00000, mirror=False)          # NaNs: a node left unwritten cannot pass
        nn.check(h, nn.lib.lbvh_refit(h, n, c.bvh_internal_node.device, c.bvh_leaf_node.device, c.triangle_aabb.device,
                                      c.triangle_index.device, c.bvh_data.device))
        got = c.bvh_data.get_data()
        assert (got["min"][: n - 1] == b.bvh["min"][: n - 1]).all() and (got["max"][: n - 1] == b.bvh["max"][: n - 1]).all()
    # the derived traversal structure after an unrelated scene used the same context scratch
    other = scenes.random_triangles(n + 1234, seed=5, extent=60.0, edge=9.0)
    d2 = H().RaytracingMeshDrawer(ctx, other).awake()
    d2.on_destroy()
    nodes["parent"][0] = 0xFFFFFFFF
    c.bvh_internal_node.sync()
    d.rebuild()
    cam = scenes.camera(160, 120, (0.0, 0.0, 260.0))
    d.update(cam, mode=L.TRACE_FAST)
    fast = d.hits()
    d.update(cam, mode=L.TRACE_REFERENCE)
    assert (fast["t"] == d.hits()["t"]).all()
    d.on_destroy()


def _fixture_scene(name):
    """(triangles, camera dict, fixture) of a committed golden: inputs come from the fixture itself where the mesh is one of
    the reference's assets (the GPU box has no /root/reference), from the seeded generators otherwise."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    if "triangles" in g.files:
        tris = g["triangles"]
    elif name == "cfg1_4096":
        tris = scenes.random_triangles(4096, seed=1)
        assert (np.stack([tris["a"], tris["b"], tris["c"]], axis=1) == g["positions"]).all()
    else:
        tris = scenes.grid_scene()
    w, h = (int(x) for x in g["resolution"])
    cam = {"screen_width": w, "screen_height": h, "camera_fov": float(g["camera_fov"]), "near_plane": float(g["camera_near"]),
           "camera_to_world": g["camera_to_world"]}
    return np.ascontiguousarray(tris, dtype=L.TRIANGLE), cam, g


@pytest.mark.parametrize("name", ["cfg1_4096", "grid_80x80", "example_object3", "viking_room"])
def test_golden_fixtures_through_the_c_abi(ctx, name):
    """The committed fixtures were produced by the independent literal emulation (oracle/literal_emulation.py via
    tests/golden/make_golden.py), not by the C oracle: every array of the build and every field of the reference-order
    hit records, bit for bit, through the C ABI.  example_object3 / viking_room are the reference's own mesh assets
    (Assets/_Assets/*.obj) fed through ingest -> build -> trace (-> shade for the textured one): SURVEY 8(f) rank 4."""
    tris, cam, g = _fixture_scene(name)
    n = len(tris)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    c = d.container
    bad_leaf, bad_inner = c.get_all_gpu_data()
    assert len(bad_leaf) == 0 and len(bad_inner) == 0
    assert (c.keys.local == g["sorted_keys"]).all() and (c.triangle_index.local == g["sorted_indices"]).all()
    assert (words(c.bvh_internal_node.local).reshape(-1, 6)[: n - 1] == g["internal"]).all()
    assert (words(c.bvh_leaf_node.local).reshape(-1, 2)[:n] == g["leaf"]).all()
    assert (words(c.bvh_internal_node.local).reshape(-1, 6)[n - 1:] == F).all()            # NullLeaf slots untouched
    assert (c.triangle_aabb.local["min"][:n] == g["tri_min"]).all() and (c.triangle_aabb.local["max"][:n] == g["tri_max"]).all()
    assert (c.bvh_data.local["min"][: n - 1] == g["bvh_min"]).all() and (c.bvh_data.local["max"][: n - 1] == g["bvh_max"]).all()
    k = H().DataBuffer(ctx, c.capacity, np.uint32)                                         # the unsorted Morton codes
    i2 = H().DataBuffer(ctx, c.capacity, np.uint32)
    a2 = H().DataBuffer(ctx, c.capacity, L.AABB)
    f3 = C.POINTER(C.c_float)
    N().check(ctx.handle, N().lib.lbvh_morton_aabb(ctx.handle, c.triangle_data.device, n, c.capacity, c.box_min.ctypes.data_as(f3),
                                                   c.box_max.ctypes.data_as(f3), k.device, i2.device, a2.device))
    assert (k.get_data()[:n] == g["morton"]).all()
    for b_ in (k, i2, a2):
        b_.dispose()
    d.update(cam, mode=L.TRACE_REFERENCE, stats=True)
    h = d.hits()
    assert (h["t"] == g["hit_t"]).all() and (h["tri"] == g["hit_tri"]).all()
    assert (h["u"] == g["hit_u"]).all() and (h["v"] == g["hit_v"]).all()
    st = d.stats()
    assert [int(st[f]) for f in st.dtype.names] == g["stats"].tolist()
    if "shaded" in g.files:                                                                # Raytracing.compute:178-184
        d.set_texture(g["texture"])
        d.shade()
        assert (d.image().view(np.uint16) == g["shaded"]).all()
    for _ in range(2):                                                                     # fast mode: same t
        d.update(cam, mode=L.TRACE_FAST)
        fh = d.hits()
        assert (fh["t"] == g["hit_t"]).all()
        same = fh["tri"] == g["hit_tri"]
        assert (fh["u"][same] == g["hit_u"][same]).all() and (fh["v"][same] == g["hit_v"][same]).all()
    d.on_destroy()


# ---- a-9 traversal -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,cam_z,res", [("cfg1", 300.0, (256, 256)), ("grid", 15.7, (200, 120)),
                                             ("torus64k", 120.0, (320, 184)), ("tiny2", 150.0, (33, 17))])
def test_trace_reference_mode_bit_exact(ctx, scene, cam_z, res):
    tris = {"cfg1": lambda: scenes.random_triangles(4096, seed=1), "grid": scenes.grid_scene,
            "torus64k": lambda: scenes.tiled_torus(grid=2), "tiny2": lambda: scenes.random_triangles(2, seed=5, extent=5.0, edge=30.0)}[scene]()
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(res[0], res[1], (0.0, 0.0, cam_z))
    oh, ost = O.trace_primary(b, cam, threads=8)
    d.update(cam, mode=L.TRACE_REFERENCE, stats=True)
    gh, gst = d.hits(), d.stats()
    assert (gh["t"] == oh["t"]).all()
    assert (gh["tri"] == oh["tri"]).all() and (gh["u"] == oh["u"]).all() and (gh["v"] == oh["v"]).all()
    assert gst == ost                                              # P, B, L, T, hits identical
    # fast mode: same hit mask, same t (tolerance of north_star: 1e-5)
    d.update(cam, mode=L.TRACE_FAST)
    fh = d.hits()
    assert ((fh["t"] < L.MAX_FLOAT) == (oh["t"] < L.MAX_FLOAT)).all()
    assert np.allclose(fh["t"], oh["t"], rtol=1e-5, atol=1e-5)
    same = fh["tri"] == oh["tri"]
    # a different triangle may win only an exact tie in t
    assert (fh["t"][~same] == oh["t"][~same]).all()
    d.on_destroy()


def test_trace_rectangles_stitch_to_the_full_frame(ctx):
    """Rays shard across GPUs by rectangle (BVH replicated): the pieces equal the whole."""
    tris = scenes.random_triangles(4096, seed=1)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    cam = scenes.camera(250, 131, (0.0, 0.0, 300.0))
    for mode in (L.TRACE_REFERENCE, L.TRACE_FAST):
        d.update(cam, mode=mode)
        full = d.hits()
        stitched = np.zeros_like(full)
        for (x0, y0, x1, y1) in [(0, 0, 250, 33), (0, 33, 101, 131), (101, 33, 250, 90), (101, 90, 250, 131)]:
            d.update(cam, rect=(x0, y0, x1, y1), mode=mode)
            stitched[y0:y1, x0:x1] = d.hits()
        assert (stitched == full).all()
    assert N().lib.lbvh_trace_primary(ctx.handle, C.byref(N().Camera.from_dict(cam)), 0, 0, 251, 10,
                                      C.byref(d.container.scene()), 0, d._hits.device, None) == -1
    d.on_destroy()


def _rotated(cam, yaw_deg, pitch_deg):
    """the camera dict with its orientation turned (camera_to_world's 3x3 block replaced, position kept)"""
    import math
    cy, sy = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    cp, sp = math.cos(math.radians(pitch_deg)), math.sin(math.radians(pitch_deg))
    yaw = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    pitch = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]], dtype=np.float64)
    m = np.array(cam["camera_to_world"], dtype=np.float32).reshape(4, 4).copy()
    m[:3, :3] = (yaw @ pitch @ m[:3, :3].astype(np.float64)).astype(np.float32)
    out = dict(cam)
    out["camera_to_world"] = m.reshape(-1).copy()
    return out


@pytest.mark.parametrize("pos,yaw,pitch", [((3.0, 2.0, 1.0), 0.0, 0.0), ((3.0, 2.0, 1.0), 90.0, 0.0), ((-20.0, 5.0, 40.0), 37.0, -23.0),
                                           ((0.0, 0.0, 0.0), 180.0, 45.0), ((60.0, -70.0, 10.0), -120.0, 60.0)])
def test_trace_fast_from_inside_the_scene(ctx, pos, yaw, pitch):
    """Cameras inside the mesh, turned every way: tiles whose rays agree on the direction signs in all eight octants and
    tiles that do not, rays parallel to an axis, hits behind the origin (the reference has no t > 0 test) — the packet
    walk's ordered box tests and DPP operands against the oracle's reference-order walk, three frames each."""
    tris = scenes.tiled_torus(nu=24, nv=16, grid=3)                 # 20 736 triangles around the origin
    d, c, b = build_both(ctx, tris)
    cam = _rotated(scenes.camera(161, 97, pos), yaw, pitch)
    oh, _ = O.trace_primary(b, cam, threads=8)
    for frame in range(3):
        d.update(cam, mode=L.TRACE_FAST)
        fh = d.hits()
        assert (fh["t"] == oh["t"]).all()
        same = fh["tri"] == oh["tri"]
        assert same.mean() > 0.999 and (fh["u"][same] == oh["u"][same]).all() and (fh["v"][same] == oh["v"][same]).all()
        d.update(cam, mode=L.TRACE_FAST_EXACT)                     # ... and with the reference's choice on ties: every word
        assert (words(d.hits()) == words(oh)).all()
    d.on_destroy()


def test_trace_fast_camera_changes_between_frames(ctx):
    """The dispatch order of a frame comes from the previous frame's tile costs, looked up where the picture came from
    (file_tiles_kernel: the two cameras' rotation, the change of position at the scene centre's depth).  A hint only:
    whatever the camera does between two frames — turn, roll, move, look away from the scene and back, a sheared or
    singular or non-finite previous matrix, another lens — every frame's hits are the oracle's."""
    tris = scenes.tiled_torus(nu=24, nv=16, grid=3)
    d, c, b = build_both(ctx, tris)
    base = scenes.camera(200, 120, (0.0, 0.0, 150.0))

    def with_matrix(cam, fn):
        m = np.array(cam["camera_to_world"], dtype=np.float32).reshape(4, 4).copy()
        fn(m)
        out = dict(cam)
        out["camera_to_world"] = m.reshape(-1).copy()
        return out

    def roll(m):
        a = np.float32(0.3)
        r = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float32)
        m[:3, :3] = m[:3, :3] @ r

    def shear(m):
        m[0, 1] += np.float32(0.25)
        m[:3, :3] *= np.float32(1.5)

    def singular(m):
        m[:3, 2] = m[:3, 0]

    wide = dict(base)
    wide["camera_fov"] = np.float32(0.9)
    sequence = [base, _rotated(base, 1.0, 0.0), _rotated(base, 3.0, -2.0), with_matrix(base, roll),
                scenes.camera(200, 120, (4.0, -3.0, 146.0)), _rotated(base, 170.0, 0.0), base,
                with_matrix(base, shear), base, wide, base, _rotated(scenes.camera(200, 120, (30.0, 10.0, 90.0)), -25.0, 8.0)]
    for k, cam in enumerate(sequence):
        if d._hits is not None:
            d._hits.fill_u32(0xFFFFFFFF)
        d.update(cam, mode=L.TRACE_FAST)
        fh = d.hits()
        oh, _ = O.trace_primary(b, cam, threads=8)
        assert (fh["t"] == oh["t"]).all(), k
    # a previous camera whose matrix cannot be inverted, or holds no numbers at all: the next frame files in place
    ref, _ = O.trace_primary(b, base, threads=8)
    for fn in (singular, lambda m: m.fill(np.nan), lambda m: m.fill(0.0)):
        d.update(with_matrix(base, fn), mode=L.TRACE_FAST)          # (its own hits are whatever such a camera sees)
        d._hits.fill_u32(0xFFFFFFFF)
        d.update(base, mode=L.TRACE_FAST)
        assert (d.hits()["t"] == ref["t"]).all()
    d.on_destroy()


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_shards_union_equals_the_full_frame(ctx, shards):
    """lbvh_trace_primary_shard: one launch per GPU; the shards partition the frame exactly as bench.shard_tiles
    says and together reproduce the unsharded frame."""
    from bench import shard_tiles
    tris = scenes.random_triangles(4096, seed=1)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    cam = scenes.camera(250, 131, (0.0, 0.0, 300.0))
    d.update(cam, mode=L.TRACE_FAST)
    full = d.hits()
    stitched = np.zeros_like(full)
    for r in range(shards):
        owned = np.zeros(full.shape, dtype=bool)
        for x0, y0, x1, y1 in shard_tiles(r, shards, 250, 131):
            owned[y0:y1, x0:x1] = True
        for frame in range(3):        # frames 2, 3 of a shard use its dispatch history (and cooperative tiles)
            d._hits.fill_u32(0xFFFFFFFF)
            d.update_shard(cam, r, shards, mode=L.TRACE_FAST)
            part = d.hits()
            assert (part.view(np.uint32).reshape(131, 250, 4)[~owned] == 0xFFFFFFFF).all()     # other shards' pixels untouched
            assert (part[owned] == full[owned]).all()
        stitched[owned] = part[owned]
    assert (stitched == full).all()
    # reference mode shards too (8x8 tiles): union equals its full frame
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref_full = d.hits()
    acc = np.zeros_like(ref_full)
    d._hits.fill_u32(0xFFFFFFFF)
    for r in range(shards):
        d.update_shard(cam, r, shards, mode=L.TRACE_REFERENCE)
    acc = d.hits()
    assert (acc == ref_full).all()
    d.on_destroy()


def test_repeated_frames_cost_ordered_and_cooperative_tiles(ctx):
    """From the second trace of a frame layout on, tiles are dispatched by their previous step counts and — when the
    frame is small enough to leave the chip under-filled — heavy tiles are walked by several waves sharing their
    best hits in LDS.  Every frame must still equal the reference order's result."""
    tris = scenes.tiled_torus(nu=60, nv=40, grid=3)                 # 129 600 triangles
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    # 3 600 / 4 096 tiles: the cooperative regime; 32 400 tiles: a full chip (XCD regions)
    for cam_z, res in ((140.0, (640, 360)), (60.0, (512, 512)), (150.0, (1920, 1080))):
        cam = scenes.camera(res[0], res[1], (3.0, -2.0, cam_z))
        d.update(cam, mode=L.TRACE_REFERENCE)
        ref = d.hits()
        costs = H().DataBuffer(ctx, (res[0] // 8) * (res[1] // 8), np.uint32)
        for frame in range(4):
            d.update(cam, mode=L.TRACE_FAST, stats=(frame == 3))
            got = d.hits()
            assert (got["t"] == ref["t"]).all()
            same = got["tri"] == ref["tri"]
            assert same.mean() > 0.9999                              # exact ties may pick the other triangle
            assert (got["u"][same] == ref["u"][same]).all() and (got["v"][same] == ref["v"][same]).all()
        d.update(cam, mode=L.TRACE_FAST_EXACT)                       # the exact mode: every word of the reference mode's frame
        assert (words(d.hits()) == words(ref)).all()
        assert int(d.stats()["hits"]) == int((ref["t"] < L.MAX_FLOAT).sum())
        # the profiling entry point reports per-tile steps in both regimes
        s = d.container.scene()
        st = H().DataBuffer(ctx, 1, L.TRACE_STATS)
        hb = H().DataBuffer(ctx, res[0] * res[1], L.HIT)
        N().check(ctx.handle, N().lib.lbvh_trace_tile_costs(ctx.handle, C.byref(N().Camera.from_dict(cam)), C.byref(s), hb.device,
                                                            st.device, costs.device))
        c = costs.get_data()
        assert c.max() >= 96 and int(c.sum()) == int(st.get_data()[0]["pops"])
    d.on_destroy()


def test_odd_frame_sizes_repeated(ctx):
    """Frame sizes around the tile / group / wave-count boundaries, each traced three times into a poisoned buffer
    (the second and third frame run the cost-ordered / cooperative scheduling): every pixel equals reference order."""
    tris = scenes.tiled_torus(nu=30, nv=20, grid=3)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    rng = np.random.default_rng(77)
    sizes = [(1, 1), (7, 9), (8, 8), (9, 8), (64, 64), (65, 63), (257, 129), (511, 3), (3, 400)]
    sizes += [(int(rng.integers(1, 400)), int(rng.integers(1, 300))) for _ in range(6)]
    for w, h in sizes:
        cam = scenes.camera(w, h, (2.0, 1.0, 130.0))
        d.update(cam, mode=L.TRACE_REFERENCE)
        ref = d.hits()
        for frame in range(3):
            d.update(cam, mode=L.TRACE_FAST)
            got = d.hits()
            assert (got["t"] == ref["t"]).all(), (w, h, frame)
            same = got["tri"] == ref["tri"]
            assert (got["u"][same] == ref["u"][same]).all() and (got["v"][same] == ref["v"][same]).all()
    d.on_destroy()


def test_equal_t_hits_pick_the_lowest_triangle_index_on_every_path(ctx):
    """coincident triangles are hit at exactly the same t.  The reference keeps whichever its visit order meets
    first; LBVH_TRACE_FAST keeps the lowest triangle index — on the one-wave packet path, on the cooperative heavy-tile
    path and for every shard count alike, frame after frame (the dispatch history decides which path a tile takes)."""
    base = scenes.tiled_torus(nu=40, nv=24, grid=3)                 # 51 840 triangles
    rng = np.random.default_rng(5)
    dup = base[rng.choice(len(base), size=len(base) // 2, replace=False)]      # every second triangle exists twice
    tris = np.concatenate([base, dup])
    tris = tris[rng.permutation(len(tris))]
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(320, 200, (2.0, -1.0, 95.0))
    oh, _ = O.trace_primary(b, cam, threads=8)
    # the expected index of a hit pixel: the lowest index among the triangles that give exactly the oracle's t there
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref = d.hits()
    assert (ref["t"] == oh["t"]).all() and (ref["tri"] == oh["tri"]).all()
    frames = []
    for frame in range(3):                                       # full frame: packet path, then cost-ordered
        d.update(cam, mode=L.TRACE_FAST)
        frames.append(d.hits())
    for shards in (2, 8):                                        # shares: cooperative heavy tiles from the second frame on
        for frame in range(3):
            d._hits.fill_u32(0x7FC00000)
            for r in range(shards):
                d.update_shard(cam, r, shards, mode=L.TRACE_FAST)
            frames.append(d.hits())
    first = frames[0]
    assert (first["t"] == oh["t"]).all()
    for f in frames[1:]:
        assert (f == first).all()                                # every field, every frame, every path
    hit = first["t"] < L.MAX_FLOAT
    # where the reference's choice has a duplicate with a lower index, the fast mode reports that lower index
    key = np.stack([tris["a"], tris["b"], tris["c"]], axis=1).reshape(len(tris), -1)
    _, inverse = np.unique(key, axis=0, return_inverse=True)
    lowest = np.full(inverse.max() + 1, len(tris), dtype=np.int64)
    np.minimum.at(lowest, inverse, np.arange(len(tris)))
    twin = lowest[inverse]                                       # lowest index of each triangle's coincident group
    same_group = inverse[first["tri"][hit]] == inverse[oh["tri"][hit]]
    assert same_group.mean() > 0.999                              # (other exact ties: shared edges)
    assert (first["tri"][hit][same_group] == twin[oh["tri"][hit]][same_group]).all()
    assert (first["tri"][hit] != oh["tri"][hit]).any()            # the case is really exercised
    d.on_destroy()


def test_camera_inside_the_scene_and_negative_t(ctx):
    """The reference accepts t < 0 hits (no t > 0 test, Raytracing.compute:70) when the leaf box
    straddles the origin; both traversal modes must keep that."""
    tris = scenes.random_triangles(20000, seed=12, extent=30.0, edge=6.0)
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(160, 120, (1.0, -2.0, 3.0))
    oh, _ = O.trace_primary(b, cam, threads=8)
    for mode in (L.TRACE_REFERENCE, L.TRACE_FAST):
        d.update(cam, mode=mode)
        gh = d.hits()
        assert ((gh["t"] < L.MAX_FLOAT) == (oh["t"] < L.MAX_FLOAT)).all()
        assert np.allclose(gh["t"], oh["t"], rtol=1e-5, atol=1e-5)
    d.on_destroy()


# ---- BASELINE size: 1 M triangles, 1080p -------------------------------------------------------------------

def test_tile_costs_exported_and_imported_between_shards(ctx):
    """lbvh_trace_costs_export / _import.  Two contexts stand for two ranks tracing the two shards of
    a frame under a turning camera and exchanging their per-tile step counts after every frame: the export of a shard
    holds exactly the step counts of its own tiles (against lbvh_trace_tile_costs of the same frame) and leaves the other
    shard's alone; with the merged array imported every frame's hits still equal the oracle's (the costs are a dispatch
    hint only); wrong frame sizes are refused."""
    tris = scenes.tiled_torus(nu=24, nv=16, grid=3)
    w, h = 328, 200                                            # ragged right / bottom tiles
    tx, ty = (w + 7) // 8, (h + 7) // 8
    c2 = H().Context(0)
    try:
        ctxs = [ctx, c2]
        drawers = [H().RaytracingMeshDrawer(c, tris).awake() for c in ctxs]
        b = O.Built(tris, capacity=drawers[0].container.capacity, threads=8)
        hits = H().DataBuffer(ctx, w * h, L.HIT)
        hits2 = H().DataBuffer(c2, w * h, L.HIT)
        frame = H().DataBuffer(ctx, tx * ty, np.uint32)
        whole = H().DataBuffer(ctx, tx * ty, np.uint32)
        stats = H().DataBuffer(ctx, 1, L.TRACE_STATS)
        from bench import yawed, shard_tiles
        base = scenes.camera(w, h, (0.0, 0.0, 140.0))
        for k in range(5):
            cam = yawed(base, 1.5 * k)
            ccam = N().Camera.from_dict(cam)
            for r, (c, d, hb) in enumerate(zip(ctxs, drawers, (hits, hits2))):
                s = d.container.scene()
                hb.fill_u32(0x7FC00000, mirror=False)
                N().check(c.handle, N().lib.lbvh_trace_primary_shard(c.handle, C.byref(ccam), r, 2, C.byref(s), L.TRACE_FAST, hb.device, None))
                c.sync()
            oh, _ = O.trace_primary(b, cam, threads=8)
            g0, g1 = hits.get_data().reshape(h, w), hits2.get_data().reshape(h, w)
            own0 = np.zeros((h, w), bool)
            for (x0, y0, x1, y1) in shard_tiles(0, 2, w, h):
                own0[y0:y1, x0:x1] = True
            assert (np.where(own0, g0["t"], g1["t"]) == oh["t"]).all()
            # exchange: each rank writes its own tiles into the zeroed frame array
            frame.fill_u32(0, mirror=False)
            ctx.sync()
            ctx.trace_costs_export(frame, tx, ty)
            ctx.sync()
            only0 = frame.get_data().copy()
            c2.trace_costs_export(frame, tx, ty)
            c2.sync()
            merged = frame.get_data().copy()
            tile_own0 = own0[::8, ::8][:ty, :tx].reshape(-1)
            assert (only0[~tile_own0] == 0).all() and (only0[tile_own0] > 0).all()
            assert (merged[tile_own0] == only0[tile_own0]).all() and (merged[~tile_own0] > 0).all()
            for c in ctxs:
                c.trace_costs_import(frame, tx, ty)
                c.sync()
        # the exported counts are the frame's per-tile node fetches (one-wave tiles; cooperative tiles count all their waves)
        s0 = drawers[0].container.scene()
        ccam = N().Camera.from_dict(yawed(base, 1.5 * 4))
        N().check(ctx.handle, N().lib.lbvh_trace_tile_costs(ctx.handle, C.byref(ccam), C.byref(s0), hits.device, stats.device, whole.device))
        ref = whole.get_data()
        assert (ref > 0).all() and np.median(np.abs(ref[tile_own0].astype(np.int64) - merged[tile_own0].astype(np.int64))) == 0
        assert N().lib.lbvh_trace_costs_export(ctx.handle, frame.device, tx + 1, ty) == -1          # not the traced frame's layout
        assert N().lib.lbvh_trace_costs_import(ctx.handle, None, tx, ty) == -1
        # a sub-rectangle with the SAME tile counts but another origin is not a frame to export (its costs would
        # land shifted by a tile)
        big = N().Camera.from_dict(scenes.camera(w + 8, h + 8, (0.0, 0.0, 140.0)))
        N().check(ctx.handle, N().lib.lbvh_trace_primary(ctx.handle, C.byref(big), 8, 8, w + 8, h + 8, C.byref(s0), L.TRACE_FAST, hits.device, None))
        assert N().lib.lbvh_trace_costs_export(ctx.handle, frame.device, tx, ty) == -1
        assert b"(0, 0)" in N().lib.lbvh_last_error(ctx.handle)
        ctx.sync()
        for d in drawers:
            d.on_destroy()
    finally:
        c2.close()


def test_fast_mode_image_differs_from_reference_mode_only_where_t_ties(ctx, capsys):
    """LBVH_TRACE_FAST resolves hits at EXACTLY equal t to the lowest triangle index, the reference
    to its own visit order (Raytracing.compute:95, strict `<`): a shaded FAST frame may differ from the reference's on those
    pixels.  Bound it at the metric's own size — the 1 M-triangle / 1080p frame of cfg2, a second camera inside the
    scene, and a scene with every second triangle duplicated: t is identical everywhere, the hit record differs ONLY on
    pixels where two triangles are hit at the same t (verified by testing the other triangle with the oracle), the
    RGBA16F images are identical everywhere else, and the pixel counts are printed."""
    rng = np.random.default_rng(5)
    tex = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    cases = [("cfg2 1M tris, camera z=250", scenes.tiled_torus(), (0.0, 0.0, 250.0), 1920, 1080, 64),
             ("cfg2 1M tris, camera inside", scenes.tiled_torus(), (3.0, 2.0, 20.0), 1920, 1080, 64)]
    dup = scenes.tiled_torus(nu=40, nv=24, grid=3)
    dup = np.concatenate([dup, dup[::2]])                                  # coincident triangles: ties on every hit of theirs
    cases.append(("every second triangle duplicated", dup, (0.0, 0.0, 140.0), 640, 360, 1 << 30))
    for name, tris, pos, w, h, max_diff in cases:
        d = H().RaytracingMeshDrawer(ctx, tris).awake()
        d.set_texture(tex)
        cam = scenes.camera(w, h, pos)
        frames = {}
        for mode in (L.TRACE_REFERENCE, L.TRACE_FAST):
            d.update(cam, mode=mode)
            hits = d.hits().copy()
            d.shade()
            frames[mode] = (hits, d.image().copy())
        (rh, rimg), (fh, fimg) = frames[L.TRACE_REFERENCE], frames[L.TRACE_FAST]
        assert (rh["t"] == fh["t"]).all()                                  # what north_star pins: identical, not within 1e-5
        differs = (words(rh) != words(fh)).reshape(h, w, 4).any(axis=2)
        assert (differs == (rh["tri"] != fh["tri"]).reshape(h, w)).all()   # a record differs iff another triangle won
        # on those pixels BOTH triangles are hit at that very t: test the other mode's triangle with the oracle's arithmetic
        ys, xs = np.nonzero(differs)
        assert len(ys) <= max_diff, (name, len(ys))
        if len(ys):
            st = O.path_begin(cam).reshape(h, w)
            for y, x in list(zip(ys, xs))[:200]:
                for other in (rh, fh):
                    t = O.ray_triangle(st[y, x]["origin"], st[y, x]["dir"], tris[int(other.reshape(h, w)[y, x]["tri"])])
                    assert t == rh.reshape(h, w)[y, x]["t"], (name, y, x)
        same = ~differs
        assert (fimg.view(np.uint16).reshape(h, w, 4)[same] == rimg.view(np.uint16).reshape(h, w, 4)[same]).all()
        img_diff = (fimg.view(np.uint16).reshape(h, w, 4) != rimg.view(np.uint16).reshape(h, w, 4)).any(axis=2)
        assert (img_diff <= differs).all()
        with capsys.disabled():
            print(f"\n  [{name}] {w}x{h}: {int(differs.sum())} pixel(s) of {w * h} resolve a t tie differently; "
                  f"{int(img_diff.sum())} of them shade differently; fast picks the lower index on "
                  f"{int((fh['tri'].reshape(h, w)[differs] < rh['tri'].reshape(h, w)[differs]).sum())}")
        assert (fh["tri"].reshape(h, w)[differs] < rh["tri"].reshape(h, w)[differs]).all()      # the documented rule
        d.on_destroy()


def test_fast_exact_mode_equals_the_reference_mode_word_for_word(ctx, capsys):
    """LBVH_TRACE_FAST_EXACT = the packet walk + the rays that met two triangles at exactly the same t traced again by the
    reference's own loop: every word of every hit record equals LBVH_TRACE_REFERENCE's — at the metric's size (1 M triangles,
    1080p, camera outside and inside the scene), on a scene with every second triangle duplicated (ties on every hit of
    theirs: ~2 000 pixels), on a scene where EVERY triangle is duplicated (every hit ties: the list holds most of the frame), on
    one with four coincident copies of every triangle (the list runs over: the fallback through the reference's loop),
    with a moving camera (history reprojected), from a cold start, for shares of a frame (1 / 2 / 3 / 8 shards: cooperative
    heavy tiles with their LDS keys) and for packed shares."""
    dup = scenes.tiled_torus(nu=40, nv=24, grid=3)
    half = np.concatenate([dup, dup[::2]])
    twice = np.concatenate([dup, dup])
    cases = [("cfg2, camera z=250", scenes.tiled_torus(), (0.0, 0.0, 250.0), 1920, 1080),
             ("cfg2, camera inside", None, (3.0, 2.0, 20.0), 1920, 1080),
             ("every second triangle duplicated", half, (0.0, 0.0, 140.0), 640, 360),
             ("every triangle duplicated", twice, (0.0, 0.0, 140.0), 640, 360),
             # four coincident copies: three candidates drop out per hit ray, the one-per-ray list runs over -> the marked rays go
             # through the reference's loop
             ("every triangle four times", np.concatenate([dup[: len(dup) // 3]] * 4), (0.0, 0.0, 140.0), 320, 180)]
    d = None
    for name, tris, pos, w, h in cases:
        if tris is not None:
            if d is not None:
                d.on_destroy()
            d = H().RaytracingMeshDrawer(ctx, tris).awake()
        cam = scenes.camera(w, h, pos)
        d.update(cam, mode=L.TRACE_REFERENCE)
        ref = words(d.hits()).copy()
        ctx.trace_forget()
        seen = []
        for frame in range(3):                                           # cold, then twice with the dispatch history
            d._hits.fill_u32(0x7FC00000, mirror=False)
            d.update(cam, mode=L.TRACE_FAST_EXACT)
            got = words(d.hits())
            assert (got == ref).all(), (name, frame, int((got != ref).any(axis=-1).sum()))
        d.update(cam, mode=L.TRACE_FAST)
        fast_differs = int((words(d.hits()) != ref).reshape(-1, 4).any(axis=1).sum())
        seen.append(fast_differs)
        # a camera that turns and moves: reprojected history
        for k in range(1, 4):
            c2 = dict(scenes.camera(w, h, (pos[0] + 0.3 * k, pos[1], pos[2] - 0.5 * k)))
            d.update(c2, mode=L.TRACE_REFERENCE)
            r2 = words(d.hits()).copy()
            d.update(c2, mode=L.TRACE_FAST_EXACT)
            assert (words(d.hits()) == r2).all(), (name, "moved", k)
        # shares of the frame into one poisoned full-frame buffer, and packed shares
        for shards in (1, 2, 3, 8):
            d._hits.fill_u32(0x7FC00000, mirror=False)
            for rep in range(2):                                         # second round: with each share's history
                for r in range(shards):
                    d.update_shard(cam, r, shards, mode=L.TRACE_FAST_EXACT)
            assert (words(d.hits()) == ref).all(), (name, "shards", shards)
        if tris is not None and len(tris) < 200_000:                   # packed shares of the tie-heavy scenes (record slot = item * 64 + lane)
            from unitysimpleraytracing_amd import _native as N
            ccam, s3 = N.Camera.from_dict(cam), d.container.scene()
            stride = int(N.lib.lbvh_shard_records(w, h, 0, 3))
            packed = H().DataBuffer(ctx, stride * 3, L.HIT)
            frame_buf = H().DataBuffer(ctx, w * h, L.HIT)
            for rep in range(2):
                packed.fill_u32(0x7FC00000, mirror=False)
                for r in range(3):
                    at = C.c_void_p(packed.device.value + r * stride * 16)
                    N.check(ctx.handle, N.lib.lbvh_trace_primary_shard_packed(ctx.handle, C.byref(ccam), r, 3, C.byref(s3), L.TRACE_FAST_EXACT, at, None))
                frame_buf.fill_u32(0x7FC00000, mirror=False)
                N.check(ctx.handle, N.lib.lbvh_frame_unpack(ctx.handle, packed.device, stride, 0, 3, 3, w, h, frame_buf.device))
                assert (words(frame_buf.get_data().reshape(h, w)) == ref).all(), (name, "packed", rep)
            packed.dispose()
            frame_buf.dispose()
        with capsys.disabled():
            print(f"\n  [{name}] {w}x{h}: LBVH_TRACE_FAST alone differs from the reference mode on {seen[0]} pixel(s); LBVH_TRACE_FAST_EXACT on none")
    d.on_destroy()


def test_cfg2_full_size(ctx):
    tris = scenes.tiled_torus()                                    # 1 000 000 triangles
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    c = d.container
    n = c.triangles_length
    b = O.Built(tris, capacity=c.capacity, threads=8)
    assert_build_equal(c, b)                                       # whole 1 M build, bit for bit
    # size-independent structure: every node except the root has exactly one parent
    inner = c.bvh_internal_node.local[: n - 1]
    li = inner["leftNodeType"] == L.INTERNAL
    ri = inner["rightNodeType"] == L.INTERNAL
    child_int = np.concatenate([inner["leftNode"][li], inner["rightNode"][ri]])
    child_leaf = np.concatenate([inner["leftNode"][~li], inner["rightNode"][~ri]])
    assert np.array_equal(np.sort(child_int), np.arange(1, n - 1, dtype=np.uint32))
    assert np.array_equal(np.sort(child_leaf), np.arange(n, dtype=np.uint32))
    aabb = c.triangle_aabb.local[:n]
    assert (c.bvh_data.local["min"][0] == aabb["min"].min(axis=0)).all()
    assert (c.bvh_data.local["max"][0] == aabb["max"].max(axis=0)).all()
    # 1080p: oracle on every 16th pixel, fast vs reference mode on the full frame
    cam = scenes.camera(1920, 1080, (0.0, 0.0, 250.0))
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref = d.hits()
    d.update(cam, mode=L.TRACE_FAST)
    fast = d.hits()
    oh, _ = O.trace_primary(b, cam, step=(16, 16), threads=8)
    assert (ref[::16, ::16]["t"] == oh["t"]).all() and (ref[::16, ::16]["tri"] == oh["tri"]).all()
    assert ((fast["t"] < L.MAX_FLOAT) == (ref["t"] < L.MAX_FLOAT)).all()
    assert np.allclose(fast["t"], ref["t"], rtol=1e-5, atol=1e-5)
    frac = float((ref["t"] < L.MAX_FLOAT).mean())
    assert 0.2 < frac < 0.95
    # BASELINE configs[2] at its own size: the 8 shards of this 1080p frame (what each of 8 GPUs traces with the BVH
    # replicated), one after the other on this GPU, three frames each into a NaN-poisoned full-frame buffer — frames 2
    # and 3 of a shard run its dispatch history and the cooperative heavy tiles (4 050 tiles per shard: trace_shared_kernel
    # on the 1 M-triangle scene).  Stitched frame == unsharded fast frame == reference-mode frame == oracle samples.
    from bench import shard_tiles
    stitched = np.zeros_like(fast)
    covered = np.zeros(fast.shape, dtype=np.int32)
    for r in range(8):
        owned = np.zeros(fast.shape, dtype=bool)
        for x0, y0, x1, y1 in shard_tiles(r, 8, 1920, 1080):
            owned[y0:y1, x0:x1] = True
        covered += owned
        for frame in range(3):
            d._hits.fill_u32(0x7FC00000)
            d.update_shard(cam, r, 8, mode=L.TRACE_FAST)
            part = d.hits()
            assert (part.view(np.uint32).reshape(1080, 1920, 4)[~owned] == 0x7FC00000).all()      # other shards' pixels untouched
            assert (part["t"][owned] == ref["t"][owned]).all(), (r, frame)
            same = (part["tri"] == ref["tri"]) & owned
            assert same.sum() >= 0.9999 * owned.sum()                                              # exact ties in t only
            assert (part["u"][same] == ref["u"][same]).all() and (part["v"][same] == ref["v"][same]).all()
        stitched[owned] = part[owned]
    assert (covered == 1).all()
    assert (stitched["t"] == fast["t"]).all() and (stitched["t"] == ref["t"]).all()
    assert (stitched[::16, ::16]["t"] == oh["t"]).all()
    d.on_destroy()


def test_cfg2_timed_rebuild_path_word_for_word_at_its_own_size(ctx):
    """what bench.py's K steps run — lbvh_build_scene on the 1 M-triangle scene as REBUILDS (the sort in its
    two-level form: histogram + one MSD pass + sort_bucket_kernel; the three merged launches; the search-free tree_pair_kernel),
    not the first build of awake() — compared word for word with the oracle after each of three rebuilds, every array the chain
    writes poisoned before each (RaytracingMeshDrawer.cs:34-51 is the chain being rebuilt).  Then, on the last rebuild's scene,
    three LBVH_TRACE_FAST frames (the second and third with dispatch history, cooperative tiles) against the
    reference-mode frame and the oracle's samples."""
    tris = scenes.tiled_torus()
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    c = d.container
    n = c.triangles_length
    b = O.Built(tris, capacity=c.capacity, threads=8)
    poison = ((c.keys, 0x0BADBEEF), (c.triangle_index, 0x0BADBEEF), (c.triangle_aabb, 0x7FC00001), (c.bvh_internal_node, 0x01357246),
              (c.bvh_leaf_node, 0x02468135), (c.bvh_data, 0x7FC00002))
    for _ in range(4):      # (the sort takes its two-level form once three sorts in a row have left their hint in order)
        d.rebuild()
        ctx.sync()
    for k in range(3):
        for buf, word in poison:
            buf.fill_u32(word, mirror=False)
        if k == 1:          # one of the three under the library's per-kernel events: which kernels a rebuild is made of
            ctx.profile_begin()
            d.rebuild()
            prof = ctx.profile_end()
            names = " ".join(prof)
            assert "sort_bucket_kernel" in names and "HIST_FINE" in names, names           # the two-level sort, not four passes
            assert "tree_pair_kernel" in names and "gather_and_reduce_kernel" in names and "apply_pair_kernel" in names, names
            assert all(v[0] == 1 for v in prof.values()), prof                              # seven launches, each once
        else:
            d.rebuild()                      # (the second plain rebuild replays the captured graph)
        assert_build_equal(c, b)
        assert (c.triangle_aabb.local["min"][:n] == b.triangle_aabb["min"][:n]).all() and (c.triangle_aabb.local["max"][:n] == b.triangle_aabb["max"][:n]).all()
    cam = scenes.camera(1920, 1080, (0.0, 0.0, 250.0))
    d.update(cam, mode=L.TRACE_REFERENCE)
    ref = d.hits()
    oh, _ = O.trace_primary(b, cam, step=(16, 16), threads=8)
    assert (ref[::16, ::16]["t"] == oh["t"]).all() and (ref[::16, ::16]["tri"] == oh["tri"]).all()
    for frame in range(3):
        d.update(cam, mode=L.TRACE_FAST)
        fast = d.hits()
        assert (fast["t"] == ref["t"]).all(), frame
    d.update(cam, mode=L.TRACE_FAST_EXACT)
    assert (words(d.hits()) == words(ref)).all()
    d.on_destroy()


def test_derived_scene_is_keyed_to_its_scene(ctx):
    """VERDICT r1 item 7 / ADVICE: the derived traversal scene is a per-context cache; it must answer only for the scene
    it was built from, and only until a library call rewrites that scene's buffers.  Two scenes of EQUAL triangle
    count on one context, traced alternately; staged calls that move the triangles without lbvh_build_fast_scene; a
    freed buffer.  A stale cache is LBVH_ERR_INVALID_ARG, never old hits with status OK."""
    n_ = N()
    a_tris = scenes.random_triangles(5000, seed=41, extent=60.0, edge=5.0)
    b_tris = scenes.random_triangles(5000, seed=42, extent=60.0, edge=5.0)
    cam = scenes.camera(120, 90, (0.0, 0.0, 200.0))
    ccam = n_.Camera.from_dict(cam)
    da = H().RaytracingMeshDrawer(ctx, a_tris).awake()
    da.update(cam, mode=L.TRACE_REFERENCE)
    ref_a = da.hits()
    da.update(cam, mode=L.TRACE_FAST)
    assert (da.hits()["t"] == ref_a["t"]).all()
    db = H().RaytracingMeshDrawer(ctx, b_tris).awake()          # same n: the cache now belongs to scene B
    db.update(cam, mode=L.TRACE_REFERENCE)
    ref_b = db.hits()
    assert not (ref_a["t"] == ref_b["t"]).all()
    db.update(cam, mode=L.TRACE_FAST)
    assert (db.hits()["t"] == ref_b["t"]).all()
    # scene A again without rebuilding its derived scene: refused, not answered from B's geometry
    sa = da.container.scene()
    rc = n_.lib.lbvh_trace_primary(ctx.handle, C.byref(ccam), 0, 0, 120, 90, C.byref(sa), L.TRACE_FAST, da._hits.device, None)
    assert rc == -1 and b"lbvh_build_fast_scene" in n_.lib.lbvh_last_error(ctx.handle)
    for _ in range(2):                                          # alternate, rebuilding each time: always the right hits
        da.build_fast_scene()
        da.update(cam, mode=L.TRACE_FAST)
        assert (da.hits()["t"] == ref_a["t"]).all()
        db.build_fast_scene()
        db.update(cam, mode=L.TRACE_FAST)
        assert (db.hits()["t"] == ref_b["t"]).all()
    # the staged chain re-run on moved triangles, without lbvh_build_fast_scene: the cache is stale
    moved = b_tris.copy()
    for f in ("a", "b", "c"):
        moved[f] = moved[f] + np.float32(7.5)
    db.container.triangle_data.local[:5000] = moved
    db.container.triangle_data.sync()                           # lbvh_buffer_upload into the scene's triangles
    sb = db.container.scene()
    rc = n_.lib.lbvh_trace_primary(ctx.handle, C.byref(ccam), 0, 0, 120, 90, C.byref(sb), L.TRACE_FAST, db._hits.device, None)
    assert rc == -1 and b"stale" in n_.lib.lbvh_last_error(ctx.handle)
    db.rebuild(fast=False, staged=True)
    rc = n_.lib.lbvh_trace_primary(ctx.handle, C.byref(ccam), 0, 0, 120, 90, C.byref(sb), L.TRACE_FAST, db._hits.device, None)
    assert rc == -1
    db.update(cam, mode=L.TRACE_REFERENCE)
    ref_moved = db.hits()
    db.build_fast_scene()
    db.update(cam, mode=L.TRACE_FAST)
    assert (db.hits()["t"] == ref_moved["t"]).all() and not (ref_moved["t"] == ref_b["t"]).all()
    # lbvh_build_scene without LBVH_BUILD_FAST_SCENE re-sorts the indices: stale again; with the flag: valid (also replayed)
    db.rebuild(fast=False)
    assert n_.lib.lbvh_trace_primary(ctx.handle, C.byref(ccam), 0, 0, 120, 90, C.byref(sb), L.TRACE_FAST, db._hits.device, None) == -1
    for _ in range(4):
        db.rebuild(fast=True)
        db.update(cam, mode=L.TRACE_FAST)
        assert (db.hits()["t"] == ref_moved["t"]).all()
    # graph replay keeps the host-side key in step: big, big, big (captured + replayed), small, big (replayed), trace big
    for _ in range(3):
        da.rebuild(fast=True)
    db.rebuild(fast=True)
    da.rebuild(fast=True)
    da.update(cam, mode=L.TRACE_FAST)
    assert (da.hits()["t"] == ref_a["t"]).all()
    # a freed scene buffer cannot back the cache
    da.on_destroy()
    da2 = H().RaytracingMeshDrawer(ctx, a_tris)
    da2.awake(fast=False)                                       # very likely the same addresses again
    s2 = da2.container.scene()
    assert n_.lib.lbvh_trace_primary(ctx.handle, C.byref(ccam), 0, 0, 120, 90, C.byref(s2), L.TRACE_FAST, db._hits.device, None) == -1
    da2.on_destroy()
    db.on_destroy()


# ---- the compiled-language host layer (C++ classes over the C ABI) ---------------------------------------------

def test_cpp_host_driver_matches_oracle():
    """BASELINE config 1 through host/lbvh_host.hpp (Awake + Update in the reference's call order)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    res = json.loads(subprocess.run([exe, "4096", "256", "256"], check=True, capture_output=True, text=True).stdout)
    pos = _splitmix_mesh(4096)
    tris = np.zeros(4096, dtype=L.TRIANGLE)
    tris["a"], tris["b"], tris["c"] = pos[:, 0], pos[:, 1], pos[:, 2]
    b = O.Built(tris, capacity=4096, threads=8)
    assert res["key_sum"] == int(b.keys[:4096].astype(np.uint64).sum())
    nd = b.internal[:4095]
    node_sum = int((nd["leftNode"].astype(np.uint64) * np.uint64(3) + nd["rightNode"].astype(np.uint64) * np.uint64(5)
                    + nd["parent"].astype(np.uint64) * np.uint64(7) + nd["leftNodeType"].astype(np.uint64)
                    + nd["rightNodeType"].astype(np.uint64)).sum(dtype=np.uint64))
    assert res["node_sum"] == node_sum
    oh, _ = O.trace_primary(b, scenes.camera(256, 256, (0.0, 0.0, 300.0)), threads=8)
    hit = oh["t"] < L.MAX_FLOAT
    assert res["hits"] == int(hit.sum())
    assert abs(res["t_sum"] - float(oh["t"][hit].astype(np.float64).sum())) < 1e-3
    assert res["shards_equal"] is True and res["update_device_ms"] > 0.0       # UpdateShard x 3 == Update; lbvh::Event


def test_cpp_host_driver_ingests_an_obj_file(tmp_path):
    """VERDICT r2 item 6 / SURVEY 8(f) rank 4: the compiled host takes an OBJ asset without Python — lbvh::LoadObj ->
    MeshBufferContainer -> Sort -> DistributeKeys -> ConstructTree -> ConstructBVH -> Update — and lands on the oracle's
    keys, node words and hit distances for the same file (here the reference's ExampleObject3 grid, re-emitted as an OBJ
    with quads from the committed fixture's triangles)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    g = np.load(os.path.join(root, "tests", "golden", "example_object3.npz"))["triangles"]
    tris = np.ascontiguousarray(g, dtype=L.TRIANGLE)[:6000]
    lines = []
    for k, t in enumerate(tris):
        for f in ("a", "b", "c"):
            lines.append("v %r %r %r" % tuple(float(x) for x in t[f]))
            lines.append("vt %r %r" % tuple(float(x) for x in t[f + "_uv"]))
            lines.append("vn %r %r %r" % tuple(float(x) for x in t[f + "_normal"]))
        lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % tuple(3 * k + 1 + c for c in (0, 0, 0, 1, 1, 1, 2, 2, 2)))
    obj = tmp_path / "grid.obj"
    obj.write_text("\n".join(lines) + "\n")
    assert scenes.load_obj(str(obj)).tobytes() == tris.tobytes()                 # the file carries the fixture's floats exactly
    res = json.loads(subprocess.run([exe, "obj", str(obj), "160", "120", "15.7"], check=True, capture_output=True, text=True).stdout)
    n = len(tris)
    assert res["triangles"] == n
    b = O.Built(tris, capacity=scenes.capacity_for(n), threads=8)
    assert res["key_sum"] == int(b.keys[:n].astype(np.uint64).sum())
    nd = b.internal[: n - 1]
    node_sum = int((nd["leftNode"].astype(np.uint64) * np.uint64(3) + nd["rightNode"].astype(np.uint64) * np.uint64(5)
                    + nd["parent"].astype(np.uint64) * np.uint64(7) + nd["leftNodeType"].astype(np.uint64)
                    + nd["rightNodeType"].astype(np.uint64)).sum(dtype=np.uint64))
    assert res["node_sum"] == node_sum
    oh, _ = O.trace_primary(b, scenes.camera(160, 120, (0.0, 0.0, 15.7)), threads=8)
    hit = oh["t"] < L.MAX_FLOAT
    assert res["hits"] == int(hit.sum()) > 100
    assert abs(res["t_sum"] - float(oh["t"][hit].astype(np.float64).sum())) < 1e-3
    assert res["shards_equal"] is True


def test_cpp_dynamic_path_tracer_matches_oracle():
    """BASELINE configs[4] in miniature through host/lbvh_host.hpp DynamicPathTracer (animate, rebuild, 2 bounces)."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "unitysimpleraytracing_amd", "host", "lbvh_driver")
    res = json.loads(subprocess.run([exe, "4096", "128", "96", "dynamic"], check=True, capture_output=True, text=True).stdout)
    pos = _splitmix_mesh(4096)
    tris = np.zeros(4096, dtype=L.TRIANGLE)
    tris["a"], tris["b"], tris["c"] = pos[:, 0], pos[:, 1], pos[:, 2]
    body = np.arange(4096, dtype=np.uint32) % 8
    centres = np.zeros((8, 4), dtype=np.float32)
    for k in range(8):
        centres[k, :3] = [40.0 if k & 1 else -40.0, 40.0 if k & 2 else -40.0, 40.0 if k & 4 else -40.0]
    moved = O.animate(tris, body, centres, np.float32(0.1))
    b = O.Built(moved, capacity=4096, threads=8)
    img, _ = O.path_trace(b, scenes.camera(128, 96, (0.0, 0.0, 300.0)), bounces=2, t_min=1e-3, albedo=0.7, seed=3, threads=8)
    px = img.view(np.uint16).reshape(-1, 4).astype(np.uint64)
    assert res["image_sum"] == int((px * np.array([1, 3, 5, 7], dtype=np.uint64)).sum(dtype=np.uint64))


# ---- a-9 tail: shading ---------------------------------------------------------------------------------------

def test_shade_bit_exact(ctx):
    """lbvh_shade over a traced frame equals the oracle's shading of the oracle's hit records, half for half."""
    rng = np.random.default_rng(21)
    tris = scenes.random_triangles(4096, seed=1)
    for f in ("a_uv", "b_uv", "c_uv"):
        tris[f] = rng.uniform(-0.3, 1.3, (4096, 2))
    for f in ("a_normal", "b_normal", "c_normal"):
        v = rng.normal(size=(4096, 3))
        tris[f] = v / np.linalg.norm(v, axis=1, keepdims=True)
    tex = rng.integers(0, 256, (64, 128, 4), dtype=np.uint8)
    d, c, b = build_both(ctx, tris)
    cam = scenes.camera(200, 120, (0.0, 0.0, 300.0))
    d.set_texture(tex)
    d.update(cam, mode=L.TRACE_REFERENCE)
    d.shade()
    img = d.image()
    oh, _ = O.trace_primary(b, cam, threads=8)
    oimg = O.shade(oh, b.triangles, tex)
    assert (img.view(np.uint16) == oimg.view(np.uint16)).all()
    assert set(np.unique(img[..., 3]).tolist()) <= {0.0, 1.0} and (img[..., 3] == 1).sum() == (oh["t"] < L.MAX_FLOAT).sum()
    # fast mode: same image except where an exact tie picked another triangle
    d.update(cam, mode=L.TRACE_FAST)
    fh = d.hits()
    d.shade()
    same = fh["tri"] == oh["tri"]
    assert (d.image().view(np.uint16)[same] == oimg.view(np.uint16)[same]).all() and same.mean() > 0.999
    # OnRenderImage: the image composed over the camera's own rendering (ImageComposer.shader:44-52), in place
    d.update(cam, mode=L.TRACE_REFERENCE)
    d.shade()
    src = rng.uniform(0.0, 1.0, (120, 200, 4)).astype(np.float16)
    dest = d.on_render_image(src)
    odest = O.compose(src, oimg)
    assert (dest.view(np.uint16) == odest.view(np.uint16)).all()
    miss = oh["t"] >= L.MAX_FLOAT
    assert (dest[miss][:, :3] == src[miss][:, :3]).all() and (dest[..., 3] == 1).all()     # alpha 0 keeps the background
    d.on_destroy()


# ---- SURVEY 8(f) rank 3 (extension): dynamic scene + secondary rays -----------------------------------------

def test_animate_and_rebuild_bit_exact(ctx):
    tris, body, centres = scenes.tiled_torus(nu=20, nv=12, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres)
    for angle in (0.01, 0.37):
        pt.animate(angle)
        c = pt.drawer.container
        moved = O.animate(tris, body, centres, angle)
        got = c.triangle_data.get_data()[: len(tris)]
        for f in ("a", "b", "c", "a_normal", "b_normal", "c_normal", "a_uv", "c_uv"):
            assert (got[f] == moved[f]).all()
        assert_build_equal(c, O.Built(moved, capacity=c.capacity, threads=8))      # full rebuild on the moved mesh
    pt.drawer.on_destroy()


def test_secondary_rays_and_path_trace_bit_exact(ctx):
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=5)
    pt.animate(0.05)
    moved = O.animate(tris, body, centres, 0.05)
    b = O.Built(moved, capacity=pt.drawer.container.capacity, threads=8)
    cam = scenes.camera(160, 96, (0.0, 0.0, 110.0))
    pt.render(cam, bounces=4)
    img = pt.image()
    oimg, ost = O.path_trace(b, cam, bounces=4, t_min=1e-3, albedo=0.7, seed=5, threads=8)
    gst = pt.states.get_data()[: 160 * 96]
    # every path state and every pixel, bit for bit: the oracle's segments resolve exact t ties like the GPU's walkers do (lowest
    # triangle index: an order-independent rule), so nothing is left to "except ties"
    for field in ("origin", "dir", "throughput", "radiance"):
        assert (gst[field].view(np.uint32) == ost[field].view(np.uint32)).all(), field
    assert (gst["alpha"] == ost["alpha"]).all() and (gst["alive"] == ost["alive"]).all()
    assert (img.view(np.uint16) == oimg.view(np.uint16)).all()
    # one bounce in isolation: identical hit distances for identical rays
    st = O.path_begin(cam)
    ph, _ = O.trace_primary(b, cam, threads=8)
    O.path_scatter(b, ph.reshape(-1), st, 0, 5, 0.7)
    sb = H().DataBuffer(ctx, len(st), L.PATH_STATE)
    sb.local[:] = st
    sb.sync()
    hb = H().DataBuffer(ctx, len(st), L.HIT)
    s = pt.drawer.container.scene()
    N().check(ctx.handle, N().lib.lbvh_trace_rays(ctx.handle, sb.device, len(st), 1e-3, C.byref(s), hb.device))
    gh = hb.get_data()
    oh = O.trace_rays(b, st, 1e-3, threads=8)
    assert (words(gh) == words(oh)).all()               # t, triangle (ties: the lowest index on both sides), u, v
    pt.drawer.on_destroy()


def test_animate_build_scene_equals_animate_plus_rebuild(ctx):
    """lbvh_animate_build_scene (one fused animate + Morton kernel in front of the replayed chain) leaves every array exactly as
    lbvh_animate + lbvh_build_scene do: moved triangles, keys, indices, boxes, nodes — and the traced frame; over several
    frames (the second call on captures the graph, later ones replay it) and a triangle count off the workgroup size."""
    tris, body, centres = scenes.tiled_torus(nu=36, nv=22, grid=3, with_bodies=True)
    tris, body = tris[:-37], body[:-37]
    a = H().DynamicPathTracer(ctx, tris, body, centres, seed=3)
    c2 = H().Context(0)
    try:
        b = H().DynamicPathTracer(c2, tris, body, centres, seed=3)
        cam = scenes.camera(200, 120, (0.0, 0.0, 150.0))
        for f in range(4):
            a.animate(0.07 * (f + 1))                    # fused
            b.animate(0.07 * (f + 1), fused=False)       # two calls
            ca, cb = a.drawer.container, b.drawer.container
            ca.get_all_gpu_data(); cb.get_all_gpu_data()
            n = ca.triangles_length
            for x, y in ((ca.triangle_data, cb.triangle_data), (ca.keys, cb.keys), (ca.triangle_index, cb.triangle_index),
                         (ca.bvh_internal_node, cb.bvh_internal_node), (ca.bvh_leaf_node, cb.bvh_leaf_node)):
                assert (words(x.local) == words(y.local)).all()
            assert (words(ca.triangle_aabb.local[:n]) == words(cb.triangle_aabb.local[:n])).all()
            assert (words(ca.bvh_data.local[: n - 1]) == words(cb.bvh_data.local[: n - 1])).all()
            moved = O.animate(tris, body, centres, 0.07 * (f + 1))
            assert (words(ca.triangle_data.local[:n]) == words(moved)).all()
            a.render(cam, bounces=2); b.render(cam, bounces=2)
            assert (a.image().view(np.uint16) == b.image().view(np.uint16)).all()
        b.drawer.on_destroy()
    finally:
        c2.close()
    a.drawer.on_destroy()


def test_cfg5_full_size_frame_against_the_oracle(ctx):
    """BASELINE configs[4] at its own size: 1 000 000 triangles in 125 rotating bodies, 1920 x 1080, primary
    rays + 4 bounces — the frame DynamicPathTracer renders after an animated rebuild, against the oracle's path states on every
    16th pixel (a 4 x 4 grid of the frame; the oracle walks those paths only, the others are dead from the start).  As in the
    small scenes: a path that met two triangles at exactly the same t may continue from the other one; every other sampled
    path must agree bit for bit in origin, direction, throughput, radiance and in its RGBA16F pixel."""
    W, Ht = 1920, 1080
    tris, body, centres = scenes.tiled_torus(with_bodies=True)
    assert len(tris) == 1_000_000
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=9)
    angle = 0.03
    pt.animate(angle)
    cam = scenes.camera(W, Ht, (0.0, 0.0, 250.0))
    pt.render(cam, bounces=4)
    gst = pt.states.get_data()[: W * Ht].reshape(Ht, W)
    img = pt.image()
    # the rebuilt tree itself, at size, word for word
    moved = O.animate(tris, body, centres, angle)
    b = O.Built(moved, capacity=pt.drawer.container.capacity, threads=8)
    c = pt.drawer.container
    c.get_all_gpu_data()
    assert_build_equal(c, b)          # keys, indices, internal AND leaf nodes, every box
    # the oracle's paths on the grid x = 1, 5, 9, ...; y = 2, 6, 10, ...
    st = O.path_begin(cam).reshape(Ht, W)
    sampled = np.zeros((Ht, W), dtype=bool)
    sampled[2::4, 1::4] = True
    st["alive"][~sampled] = 0
    flat = st.reshape(-1)
    hits = O.trace_rays(b, flat, -3.0e38, threads=8)               # the primary segment: any t, ties to the lowest index (as LBVH_TRACE_FAST)
    O.path_scatter(b, hits, flat, 0, 9, 0.7)
    for k in range(1, 5):
        h = O.trace_rays(b, flat, 1e-3, threads=8)
        O.path_scatter(b, h, flat, k, 9, 0.7)
    oimg = O.path_resolve(flat).reshape(Ht, W, 4)
    g, o = gst[sampled], st[sampled]
    same = (g["origin"] == o["origin"]).all(axis=1) & (g["dir"] == o["dir"]).all(axis=1)
    assert len(g) == 270 * 480 and same.all(), same.mean()
    for field in ("throughput", "radiance"):
        assert (g[field].view(np.uint32) == o[field].view(np.uint32)).all(), field
    assert (g["alpha"] == o["alpha"]).all() and (g["alive"] == o["alive"]).all()
    assert (img[sampled].view(np.uint16)[same] == oimg[sampled].view(np.uint16)[same]).all()
    assert 0.3 < float((img[..., 3] > 0).mean()) < 0.6             # the primary hit fraction of cfg2's camera
    pt.drawer.on_destroy()


def test_ray_walk_statistics(ctx):
    """lbvh_ray_stats_target: the four-wide walkers' own counters (the algorithmic bytes of cfg5's roofline) — every live ray
    counted once, at least one node line per ray, counts identical for both four-wide kernels' instantiations with and
    without the counting (hit records unchanged), nothing counted once the target is cleared."""
    tris = scenes.tiled_torus(nu=24, nv=16, grid=2)
    d = H().RaytracingMeshDrawer(ctx, tris).awake()
    W, Ht = 160, 96
    cam = N().Camera.from_dict(scenes.camera(W, Ht, (0.0, 0.0, 120.0)))
    states = H().DataBuffer(ctx, W * Ht, L.PATH_STATE)
    hits = H().DataBuffer(ctx, W * Ht, L.HIT)
    stats = H().DataBuffer(ctx, 1, L.RAY_STATS)
    s = d.container.scene()
    N().check(ctx.handle, N().lib.lbvh_path_begin(ctx.handle, C.byref(cam), states.device))
    N().check(ctx.handle, N().lib.lbvh_trace_rays(ctx.handle, states.device, W * Ht, 0.0, C.byref(s), hits.device))
    plain = hits.get_data().copy()
    try:
        for walker in (1, 2):
            N().check(ctx.handle, N().lib.lbvh_debug_ray_walker(ctx.handle, walker))
            stats.fill_u32(0)
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, stats.device))
            N().check(ctx.handle, N().lib.lbvh_trace_rays(ctx.handle, states.device, W * Ht, 0.0, C.byref(s), hits.device))
            N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
            st = stats.get_data()[0].copy()
            assert int(st["rays"]) == W * Ht and int(st["node_fetches"]) >= W * Ht
            assert int(st["triangle_tests"]) >= int((plain["t"] < L.MAX_FLOAT).sum())
            assert (words(hits.get_data()) == words(plain)).all()
            N().check(ctx.handle, N().lib.lbvh_trace_rays(ctx.handle, states.device, W * Ht, 0.0, C.byref(s), hits.device))
            assert (words(stats.get_data()) == words(np.array([st]))).all()        # target cleared: nothing added
    finally:
        N().check(ctx.handle, N().lib.lbvh_ray_stats_target(ctx.handle, None))
        N().check(ctx.handle, N().lib.lbvh_debug_ray_walker(ctx.handle, 1))
    for bfr in (states, hits, stats):
        bfr.dispose()
    d.on_destroy()


@pytest.mark.parametrize("lds_entries", [1, 2, 5])
def test_secondary_rays_deep_stack_in_device_memory(ctx, lds_entries):
    """The per-ray walk keeps the first 16 stack entries of a lane in LDS and deeper ones in a device-memory slab.
    With the split lowered to 1 / 2 / 5 entries (lbvh_debug_ray_stack_split) ordinary rays use the slab all the time:
    hit records identical to the default split's, record for record, and `t` identical to the oracle's."""
    tris, body, centres = scenes.tiled_torus(nu=40, nv=24, grid=3, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=11)
    b = O.Built(tris, capacity=pt.drawer.container.capacity, threads=8)
    cam = scenes.camera(200, 120, (0.0, 0.0, 150.0))
    st = O.path_begin(cam)
    ph, _ = O.trace_primary(b, cam, threads=8)
    O.path_scatter(b, ph.reshape(-1), st, 0, 11, 0.7)
    assert st["alive"].sum() > 2000
    sb = H().DataBuffer(ctx, len(st), L.PATH_STATE)
    sb.local[:] = st
    sb.sync()
    hb = H().DataBuffer(ctx, len(st), L.HIT)
    s = pt.drawer.container.scene()
    n_ = N()
    assert n_.lib.lbvh_debug_ray_stack_split(ctx.handle, 0) == -1 and n_.lib.lbvh_debug_ray_stack_split(ctx.handle, 17) == -1
    try:
        frames = []
        for split in (16, lds_entries):
            n_.check(ctx.handle, n_.lib.lbvh_debug_ray_stack_split(ctx.handle, split))
            hb.local[:] = np.zeros(1, L.HIT)
            hb.local["t"] = np.nan
            hb.sync()
            n_.check(ctx.handle, n_.lib.lbvh_trace_rays(ctx.handle, sb.device, len(st), 1e-3, C.byref(s), hb.device))
            frames.append(hb.get_data().copy())
    finally:
        n_.check(ctx.handle, n_.lib.lbvh_debug_ray_stack_split(ctx.handle, 16))
    assert (words(frames[0]) == words(frames[1])).all()
    oh = O.trace_rays(b, st, 1e-3, threads=8)
    assert (frames[1]["t"] == oh["t"]).all()
    pt.drawer.on_destroy()


@pytest.mark.parametrize("scene", ["torus", "soup", "duplicates", "two", "three", "seven"])
def test_secondary_rays_four_wide_walk_equals_binary_walk(ctx, scene):
    """lbvh_trace_rays walks the derived scene as four-wide nodes (collapse_wide_kernel: every binary node with its
    largest children opened). Same leaves, same boxes, ties to the lower triangle index: the hit records equal the binary
    walk's (lbvh_debug_ray_walker(ctx, 0)) word for word — also with the stack split lowered so that waiting siblings go
    through the device-memory slab, and with the kernel the later bounces use (walker 2: the next node requested before the
    step's triangles are tested) — and `t` equals the oracle's everywhere."""
    if scene == "torus":
        tris = scenes.tiled_torus(nu=40, nv=24, grid=3)
    elif scene == "soup":
        tris = scenes.random_triangles(n=6000, seed=4, extent=60.0, edge=6.0)
    elif scene == "duplicates":
        base = scenes.random_triangles(n=2000, seed=6, extent=40.0, edge=8.0)
        tris = np.concatenate([base, base[::2]])               # every second triangle twice: exact t ties
    else:
        tris = scenes.random_triangles(n={"two": 2, "three": 3, "seven": 7}[scene], seed=8, extent=10.0, edge=6.0)
    d, c, b = build_both(ctx, tris)
    d.rebuild(fast=True)
    st = _random_ray_states(tris, 20000, seed=len(tris))
    sb = H().DataBuffer(ctx, len(st), L.PATH_STATE)
    sb.local[:] = st
    sb.sync()
    hb = H().DataBuffer(ctx, len(st), L.HIT)
    s = c.scene()
    n_ = N()
    assert n_.lib.lbvh_debug_ray_walker(ctx.handle, 3) == -1
    frames = {}
    try:
        for wide, split in ((0, 16), (1, 16), (1, 1), (1, 3), (2, 16), (2, 2)):
            n_.check(ctx.handle, n_.lib.lbvh_debug_ray_walker(ctx.handle, wide))
            n_.check(ctx.handle, n_.lib.lbvh_debug_ray_stack_split(ctx.handle, split))
            hb.local[:] = np.zeros(1, L.HIT)
            hb.local["t"] = np.nan
            hb.sync()
            n_.check(ctx.handle, n_.lib.lbvh_trace_rays(ctx.handle, sb.device, len(st), 1e-3, C.byref(s), hb.device))
            frames[(wide, split)] = hb.get_data().copy()
    finally:
        n_.check(ctx.handle, n_.lib.lbvh_debug_ray_walker(ctx.handle, 1))
        n_.check(ctx.handle, n_.lib.lbvh_debug_ray_stack_split(ctx.handle, 16))
    for key in ((1, 16), (1, 1), (1, 3), (2, 16), (2, 2)):
        assert (words(frames[(0, 16)]) == words(frames[key])).all(), key
    oh = O.trace_rays(b, st, 1e-3, threads=8)
    assert (frames[(1, 16)]["t"] == oh["t"]).all()
    hit = frames[(1, 16)]["t"] < 1e30
    assert hit.sum() > (0 if len(tris) < 10 else 1000)
    if scene == "duplicates":
        # a ray that meets a duplicated triangle meets its copy at the same t: the record names the lower index
        dup_of = {2000 + k: 2 * k for k in range(1000)}
        assert not np.isin(frames[(1, 16)]["tri"][hit], list(dup_of)).any()
    d.on_destroy()


@pytest.mark.parametrize("res", [(1, 1), (5, 3), (63, 1), (65, 9)])
def test_path_trace_tiny_frames(ctx, res):
    """Ray counts below / around one wave: live-ray compaction, lane refill and lbvh_path_bounce at the edges."""
    tris, body, centres = scenes.tiled_torus(nu=16, nv=10, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=9)
    pt.animate(0.2)
    moved = O.animate(tris, body, centres, 0.2)
    b = O.Built(moved, capacity=pt.drawer.container.capacity, threads=4)
    cam = scenes.camera(res[0], res[1], (0.0, 0.0, 70.0))
    for frame in range(2):
        pt.render(cam, bounces=3)
        img = pt.image()
        oimg, ost = O.path_trace(b, cam, bounces=3, t_min=1e-3, albedo=0.7, seed=9, threads=4)
        gst = pt.states.get_data()[: res[0] * res[1]]
        assert (gst["origin"] == ost["origin"]).all() and (gst["dir"] == ost["dir"]).all()
        assert (img.view(np.uint16) == oimg.view(np.uint16)).all()
    pt.drawer.on_destroy()


def test_path_first_bounce_equals_begin_plus_bounce_zero(ctx):
    """lbvh_path_first_bounce makes every pixel's path state from the camera inside the bounce-0 pass instead of loading what
    lbvh_path_begin stored: states and next-segment hit records identical to the two calls, word for word (a ragged frame,
    hits and misses, rays that start inside boxes)."""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=21)
    w, h = 203, 117
    count = w * h
    s = pt.drawer.container.scene()
    hd, lib = ctx.handle, N().lib
    for pos in ((0.0, 0.0, 90.0), (1.0, 2.0, 6.0)):
        ccam = N().Camera.from_dict(scenes.camera(w, h, pos))
        out = []
        for fused in (True, False):
            states = H().DataBuffer(ctx, count, L.PATH_STATE)
            states.fill_u32(0x7FC00000, mirror=False)                              # nothing may survive from before
            hits = H().DataBuffer(ctx, count, L.HIT)
            N().check(hd, lib.lbvh_trace_primary(hd, C.byref(ccam), 0, 0, w, h, C.byref(s), L.TRACE_FAST, hits.device, None))
            if fused:
                N().check(hd, lib.lbvh_path_first_bounce(hd, C.byref(ccam), C.byref(s), states.device, hits.device, 21, 0.7, 1e-3))
            else:
                N().check(hd, lib.lbvh_path_begin(hd, C.byref(ccam), states.device))
                N().check(hd, lib.lbvh_path_bounce(hd, C.byref(s), states.device, hits.device, count, 0, 21, 0.7, 1e-3))
            out.append((states.get_data().copy(), hits.get_data().copy()))
            states.dispose(); hits.dispose()
        assert (words(out[0][0]) == words(out[1][0])).all() and (words(out[0][1]) == words(out[1][1])).all()
        assert out[0][0]["alive"].sum() > 100
    pt.drawer.on_destroy()


def test_light_whole_frames_take_the_eight_wave_cooperative_shape(ctx):
    """Round 5: a whole frame whose previous frames were LIGHT (the scene far away: few tiles hold all of it) walks its heavy
    tiles with workgroups of 8 waves instead of 4 — chosen from a work estimate two frames stale.  Six frames of a 250 k-triangle
    scene at 1080p from far away, each into a poisoned buffer: every frame's t equals the reference mode's bit for bit and the
    exact mode's records equal it word for word (the shape changes under way: first frames 4 waves or none, later ones 8), and
    the same camera close by (a busy frame: back to 4 waves) likewise."""
    tris = scenes.tiled_torus(nu=40, nv=25)
    d, c, b = build_both(ctx, tris)
    d.rebuild(fast=True)
    W, Ht = 1920, 1080
    s = c.scene()
    hb = H().DataBuffer(ctx, W * Ht, L.HIT)
    for pos in ((3.0, 2.0, 800.0), (3.0, 2.0, 250.0), (3.0, 2.0, 900.0)):
        cam = N().Camera.from_dict(scenes.camera(W, Ht, pos))
        hb.fill_u32(0x7FC00000, mirror=False)
        N().check(ctx.handle, N().lib.lbvh_trace_primary(ctx.handle, C.byref(cam), 0, 0, W, Ht, C.byref(s), L.TRACE_REFERENCE, hb.device, None))
        ref = hb.get_data().copy()
        for mode in (L.TRACE_FAST, L.TRACE_FAST_EXACT):
            for f in range(6):
                hb.fill_u32(0x7FC00000, mirror=False)
                N().check(ctx.handle, N().lib.lbvh_trace_primary(ctx.handle, C.byref(cam), 0, 0, W, Ht, C.byref(s), mode, hb.device, None))
                got = hb.get_data()
                assert (got["t"].view(np.uint32) == ref["t"].view(np.uint32)).all(), (pos, mode, f)
                if mode == L.TRACE_FAST_EXACT and not (words(got) == words(ref)).all():
                    # word for word the reference mode's frame, except where the reference's winner lies in front of its own
                    # triangle's box (include/lbvh.h): looked up in the oracle, not assumed away
                    unexplained, _ = O.unexplained_mismatches(b, scenes.camera(W, Ht, pos), ref[: W * Ht].reshape(Ht, W),
                                                              got[: W * Ht].reshape(Ht, W), words=True)
                    assert not unexplained, (pos, f, unexplained[:4])
        assert (ref["t"] < 1e30).sum() > 1000
    hb.dispose()
    d.on_destroy()


def test_path_bounces_from_the_live_list_equal_bounces_over_every_pixel(ctx):
    """Round 5: lbvh_path_bounce b >= 1 (and the frame's last lbvh_path_scatter) look only at the paths the bounce before listed as
    live, if they continue that very frame.  Same frame three ways — (a) as the host classes issue it (lists used), (b) with the
    path states sent through the host between the calls (an outside write: the list is dropped, every pixel is scanned), (c) with
    a foreign lbvh_trace_rays in between (takes the list buffer) — states, hit records and image word for word the same."""
    tris, body, centres = scenes.tiled_torus(nu=24, nv=16, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=33)
    w, h = 211, 123
    count = w * h
    s = pt.drawer.container.scene()
    hd, lib = ctx.handle, N().lib
    ccam = N().Camera.from_dict(scenes.camera(w, h, (2.0, 1.0, 95.0)))
    results = []
    for variant in ("lists", "states rewritten", "foreign rays"):
        states = H().DataBuffer(ctx, count, L.PATH_STATE)
        hits = H().DataBuffer(ctx, count, L.HIT)
        image = H().DataBuffer(ctx, count, np.uint64)
        other_states = H().DataBuffer(ctx, 64, L.PATH_STATE)
        other_hits = H().DataBuffer(ctx, 64, L.HIT)
        other_states.fill_u32(0, mirror=False)

        def disturb():
            if variant == "states rewritten":
                st = states.get_data().copy()
                states.local[:] = st
                states.sync()                                                      # lbvh_buffer_upload: an outside write
            elif variant == "foreign rays":
                N().check(hd, lib.lbvh_trace_rays(hd, other_states.device, 64, 1e-3, C.byref(s), other_hits.device))
        N().check(hd, lib.lbvh_trace_primary(hd, C.byref(ccam), 0, 0, w, h, C.byref(s), L.TRACE_FAST, hits.device, None))
        N().check(hd, lib.lbvh_path_first_bounce(hd, C.byref(ccam), C.byref(s), states.device, hits.device, 33, 0.7, 1e-3))
        for b in range(1, 4):
            disturb()
            N().check(hd, lib.lbvh_path_bounce(hd, C.byref(s), states.device, hits.device, count, b, 33, 0.7, 1e-3))
        disturb()
        N().check(hd, lib.lbvh_path_scatter(hd, C.byref(s), hits.device, count, 4, 33, 0.7, states.device))
        N().check(hd, lib.lbvh_path_resolve(hd, states.device, count, image.device))
        results.append((states.get_data().copy(), hits.get_data().copy(), image.get_data().copy()))
        for bfr in (states, hits, image, other_states, other_hits):
            bfr.dispose()
    for r in results[1:]:
        assert (words(r[0]) == words(results[0][0])).all() and (words(r[1]) == words(results[0][1])).all() and (r[2] == results[0][2]).all()
    assert results[0][0]["radiance"].sum() > 0
    pt.drawer.on_destroy()


def test_path_bounce_zero_treats_prefilled_hit_records_as_misses(ctx):
    """a hit buffer pre-filled with 0xFFFFFFFF words (what lbvh_driver.cpp does) and only partly traced holds
    {t >= MAX_FLOAT, triangle = 0xFFFFFFFF} records that are the CALLER's, not marks of paths that ended earlier: at
    bounce 0 lbvh_path_bounce must treat them as lbvh_path_scatter does (sky term, path ends) — states and next-segment
    hits identical to the two separate calls."""
    tris, body, centres = scenes.tiled_torus(nu=20, nv=12, grid=2, with_bodies=True)
    pt = H().DynamicPathTracer(ctx, tris, body, centres, t_min=1e-3, albedo=0.7, seed=3)
    cam = scenes.camera(96, 64, (0.0, 0.0, 90.0))
    ccam = N().Camera.from_dict(cam)
    count = 96 * 64
    s = pt.drawer.container.scene()
    h, lib = ctx.handle, N().lib
    out = []
    for fused in (True, False):
        states = H().DataBuffer(ctx, count, L.PATH_STATE)
        hits = H().DataBuffer(ctx, count, L.HIT)
        hits.fill_u32(0xFFFFFFFF, mirror=False)                                   # t = NaN-pattern >= MAX_FLOAT test: !(t < MAX)
        N().check(h, lib.lbvh_trace_primary(h, C.byref(ccam), 0, 0, 96, 32, C.byref(s), L.TRACE_FAST, hits.device, None))   # top half only
        N().check(h, lib.lbvh_path_begin(h, C.byref(ccam), states.device))
        if fused:
            N().check(h, lib.lbvh_path_bounce(h, C.byref(s), states.device, hits.device, count, 0, 3, 0.7, 1e-3))
        else:
            N().check(h, lib.lbvh_path_scatter(h, C.byref(s), hits.device, count, 0, 3, 0.7, states.device))
            N().check(h, lib.lbvh_trace_rays(h, states.device, count, 1e-3, C.byref(s), hits.device))
        out.append((states.get_data().copy(), hits.get_data().copy()))
        states.dispose(); hits.dispose()
    (st_f, hit_f), (st_s, hit_s) = out
    assert (words(st_f) == words(st_s)).all()
    untraced = np.arange(count) >= 96 * 32
    assert (st_f["alive"][untraced] == 0).all() and (st_f["radiance"][untraced] > 0).all()      # they got their sky term
    assert (hit_f["t"] == hit_s["t"]).all()
    pt.drawer.on_destroy()


def test_randomised_parity_soak_short():
    """tools/fuzz_parity.py for 15 seconds with a fixed seed: random sorts, random scenes (soup, tori, duplicated and
    degenerate triangles, one Morton cell, outside the scene box) built staged and through lbvh_build_scene, random
    cameras / resolutions / shard counts over several frames, all against the oracle.  (Longer runs: the tool itself.)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "15", "20261003"], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "all equal" in r.stdout
