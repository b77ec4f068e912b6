"""The image tail — lbvh_shade, lbvh_compose, lbvh_path_resolve, lbvh_animate, lbvh_path_scatter, lbvh_path_begin — at its numeric
edges, in two tiers: word for word against oracle/ (sharp), and against tests/image_reference.py, a float64 / numpy restatement of
include/lbvh.h that shares no code with either (independent).  The unmarked tests hold the oracle to the independent references on
the CPU; the gpu-marked ones hold the kernels to both.  Every bound of the independent tier is derived in image_reference.py from
fp32 unit roundoff, the operation count and the inputs' magnitudes, and every test asserts that its bound stays below half a
half-ulp of the result, on every record (nothing is skipped): a result may be either half next to the exact value, nothing else."""
import ctypes as C
import functools

import numpy as np
import pytest

import image_reference as R
import oracle as O
from query_support import H, N, words
from unitysimpleraytracing_amd import layouts as L
from unitysimpleraytracing_amd import scenes

gpu = pytest.mark.gpu
GUARD = 0xA5C35A3C
SLACK = 64
COUNTS = (1, 255, 256, 257, 256 + 37)


def up(ctx, arr):
    a = np.ascontiguousarray(arr)
    b = H().DataBuffer(ctx, max(len(a), 1), a.dtype)
    b.local[: len(a)] = a
    b.sync()
    return b


class Guarded:
    """an output buffer of n items + SLACK, every word prefilled with GUARD; read() checks that the slack is untouched"""

    def __init__(self, ctx, n, dtype, init=None):
        self.n = n
        self.buf = H().DataBuffer(ctx, n + SLACK, dtype)
        self.buf.local.view(np.uint32)[:] = GUARD
        if init is not None:
            self.buf.local[:n] = init
        self.buf.sync()
        self.device = self.buf.device

    def read(self, written=None):
        got = self.buf.get_data()
        assert (got[self.n if written is None else written:].view(np.uint32) == GUARD).all(), "written past the end"
        out = got[: self.n].copy()
        self.buf.dispose()
        return out


# ---- 1. the half store: lbvh_path_resolve over every half, every midpoint, both ends ----------------------------------------

@functools.lru_cache(maxsize=None)
def resolve_case():
    x = R.conversion_sweep()
    x = np.concatenate([x, np.zeros(-len(x) % 4, dtype=np.float32)])
    st = np.zeros(len(x) // 4, dtype=L.PATH_STATE)
    st["radiance"] = x.reshape(-1, 4)[:, :3]
    st["alpha"] = x.reshape(-1, 4)[:, 3]
    ref = R.to_half_bits(x).reshape(-1, 4)
    ref.setflags(write=False)
    return st, x, ref


def test_numpy_half_cast_equals_torch_half():
    _, x, ref = resolve_case()
    t = R.torch_half_bits(x)
    if t is not None:
        assert R.half_words_match(t.reshape(-1, 4), ref).all()
    assert len(x) > 250_000 and R.half_is_nan(ref).sum() == 8


def test_oracle_path_resolve_is_round_to_nearest_even():
    st, _, ref = resolve_case()
    got = O.path_resolve(st).view(np.uint16)
    assert R.half_words_match(got, ref).all()


@gpu
def test_path_resolve_is_round_to_nearest_even(ctx):
    """v_cvt_f16_f32 against numpy's cast on 256 028 floats.  NaN words the GPU returned, measured on an MI355X: 0x7E00, 0x7F2A,
    0x7FFF, 0xFE00, 0xFFFF for the eight NaN inputs of conversion_sweep — the sign, the quiet bit, and the top nine payload bits
    of the fp32 NaN (0x7FA55555 -> 0x7F2A; a signalling NaN comes out quiet).  The oracle returns 0x7E00 / 0xFE00 and numpy keeps
    payload bits its own way, so a NaN is compared by class only and lbvh.h calls its bits unspecified."""
    st, _, ref = resolve_case()
    sb = up(ctx, st)
    for count in (len(st),) + COUNTS:
        out = Guarded(ctx, count, np.uint64)
        N().check(ctx.handle, N().lib.lbvh_path_resolve(ctx.handle, sb.device, count, out.device))
        got = out.read().view(np.uint16).reshape(-1, 4)
        assert R.half_words_match(got, ref[:count]).all()
        if count == len(st):
            nan = R.half_is_nan(ref)
            print("GPU NaN words:", sorted({hex(w) for w in got[nan].tolist()}))
            assert (got == O.path_resolve(st).view(np.uint16))[~nan].all()
    sb.dispose()


# ---- 2. lbvh_compose over all halves -----------------------------------------------------------------------------------------

def _h(*v):
    return np.array(v, dtype=np.float16).view(np.uint16)


@functools.lru_cache(maxsize=None)
def compose_case():
    """(background, object) words [n, 4]: every half as alpha against fixed (background, object) pairs, and every finite half
    as background against alpha in {0, 1, 0.5, 2, -1}"""
    pairs = [(0.0, 0.0), (-0.0, 0.0), (0.5, 0.5), (65504.0, -65504.0), (-65504.0, 65504.0), (6e-8, 6.1e-5), (-6e-8, 3e-5),
             (np.inf, 1.0), (1.0, np.inf), (-np.inf, 2.0), (0.25, 1.0), (1000.0, 0.001)]
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    bgs, obs = [], []
    for g in range(0, len(pairs), 3):
        bg, ob = np.zeros((65536, 4), np.uint16), np.zeros((65536, 4), np.uint16)
        for k, (b, o) in enumerate(pairs[g: g + 3]):
            bg[:, k], ob[:, k] = _h(b)[0], _h(o)[0]
        bg[:, 3] = every[::-1]                    # the background's alpha is never read
        ob[:, 3] = every
        bgs.append(bg); obs.append(ob)
    pos = np.arange(0, 0x7C00, dtype=np.uint16)
    finite = np.concatenate([pos, pos | 0x8000])
    for a in (0.0, 1.0, 0.5, 2.0, -1.0):
        bg, ob = np.zeros((len(finite), 4), np.uint16), np.zeros((len(finite), 4), np.uint16)
        bg[:, 0], bg[:, 1], bg[:, 2], bg[:, 3] = finite, finite[::-1], finite, 0x7E00
        ob[:, :3] = _h(0.75, -3.0, 1000.0)
        ob[:, 3] = _h(a)[0]
        bgs.append(bg); obs.append(ob)
    bg, ob = np.concatenate(bgs), np.concatenate(obs)
    ref = R.compose32(bg, ob)
    for a in (bg, ob, ref):
        a.setflags(write=False)
    return bg, ob, ref


@functools.lru_cache(maxsize=None)
def compose_convex_case():
    """the float64 tier's inputs: convex combinations of non-negative values, where lerp cancels nothing: every finite half
    >= 0 as background, objects 0.25 / 1 / 1000, alpha in {0, 0.25, 0.5, 0.75}, and alpha 1 over the backgrounds <= the object."""
    pos = np.arange(0, 0x7C00, dtype=np.uint16)
    bgs, obs = [], []
    for a in (0.0, 0.25, 0.5, 0.75, 1.0):
        bg, ob = np.zeros((len(pos), 4), np.uint16), np.zeros((len(pos), 4), np.uint16)
        bg[:, :3] = pos[:, None]
        ob[:, :3] = _h(0.25, 1.0, 1000.0)
        ob[:, 3] = _h(a)[0]
        if a == 1.0:
            bg[:, :3] = np.minimum(bg[:, :3], ob[:, :3])         # positive halves order like their words
        bgs.append(bg); obs.append(ob)
    return np.concatenate(bgs), np.concatenate(obs)


# COMPOSE_BOUND = 1.01 * U * (2 |a (ob - bg)| + |result|): three fp32 roundings (difference, product, sum), derived in
# image_reference.compose64.  On compose_convex_case |a (ob - bg)| <= 3 |result|, so the bound is at most 7.1 U |result| =
# 4.2e-7 |result|, against half a half-ulp >= 2^-12 |result| = 2.4e-4 |result| (and 2^-25 against 0 in the subnormal range).
def check_compose_independent(fn):
    bg, ob = compose_convex_case()
    e, bound = R.compose64(bg, ob)
    assert (bound < 0.5 * R.half_ulp(e)).all()
    got = fn(bg, ob)
    assert R.half_interval_ok(got[:, :3], e, bound).all() and (got[:, 3] == 0x3C00).all()


def oracle_compose(bg, ob):
    return O.compose(bg.view(np.float16), ob.view(np.float16)).view(np.uint16)


def test_oracle_compose_over_all_halves():
    bg, ob, ref = compose_case()
    got = oracle_compose(bg, ob)
    assert R.half_words_match(got, ref).all() and (got[:, 3] == 0x3C00).all()
    check_compose_independent(oracle_compose)


def gpu_compose(ctx, bg, ob, count=None, in_place=False):
    count = len(bg) if count is None else count
    ob_b = up(ctx, ob.view(np.uint64).reshape(-1))
    if in_place:
        out = Guarded(ctx, count, np.uint64, init=bg[:count].view(np.uint64).reshape(-1))
        N().check(ctx.handle, N().lib.lbvh_compose(ctx.handle, out.device, ob_b.device, count, out.device))
    else:
        bg_b = up(ctx, bg.view(np.uint64).reshape(-1))
        out = Guarded(ctx, count, np.uint64)
        N().check(ctx.handle, N().lib.lbvh_compose(ctx.handle, bg_b.device, ob_b.device, count, out.device))
        assert (bg_b.get_data()[: len(bg)] == bg.view(np.uint64).reshape(-1)).all()       # inputs are left alone
        bg_b.dispose()
    got = out.read().view(np.uint16).reshape(-1, 4)
    ob_b.dispose()
    return got


@gpu
def test_compose_over_all_halves(ctx):
    bg, ob, ref = compose_case()
    oref = oracle_compose(bg, ob)
    for count in (len(bg),) + COUNTS:
        a = gpu_compose(ctx, bg, ob, count)
        b = gpu_compose(ctx, bg, ob, count, in_place=True)
        assert (a == b).all()
        assert R.half_words_match(a, ref[:count]).all() and (a[:, 3] == 0x3C00).all()
        nan = R.half_is_nan(ref[:count])
        assert (a == oref[:count])[~nan].all()                     # sharp tier (NaN words: see lbvh.h)
    check_compose_independent(lambda x, y: gpu_compose(ctx, x, y))


# ---- 3. / 4. lbvh_shade on synthetic hit records ------------------------------------------------------------------------------

TEXTURES = ((1, 1), (1, 7), (7, 1), (5, 3), (257, 2), (64, 128), (300, 300), (512, 2))      # (w, h)
BARY = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.25, 0.5), (0.5, 0.5), (-2.0 ** -20, 0.3), (0.6, 0.4 + 2.0 ** -20))
N_NORMAL_KINDS = 11


def make_texture(idx, w, h, rng):
    """R, G in [160, 255] (254 and 255 forced in), B flat 0, flat 1 or in {3, 4} by turns: wherever two neighbouring texels
    differ, their difference is at most 0.6 of the smaller one — what keeps the sampler's slope term |du| * w below half an ulp
    of the result (SHADE_BOUND).  0, 1, 254 and 255 all occur; the fourth channel is random and never read."""
    tex = np.zeros((h, w, 4), dtype=np.uint8)
    tex[..., :2] = rng.integers(160, 256, (h, w, 2))
    tex[0, 0, 0], tex[-1, -1, 0], tex[0, -1, 1], tex[-1, 0, 1] = 254, 255, 255, 254
    tex[..., 2] = (0, 1)[idx % 3] if idx % 3 < 2 else rng.integers(3, 5, (h, w))
    if w * h == 1:
        tex[0, 0, :3] = (255, 1, 0)
    tex[..., 3] = rng.integers(0, 256, (h, w))
    return tex


def axis_coordinates(size, rng):
    """texel centres and borders with their fp32 neighbours, the ends, far outside, and coordinates whose product with the size
    overflows fp32 (1e36 against 512)"""
    f = np.float32
    ks = np.unique(np.concatenate([np.arange(min(size, 4)), [size // 2, size - 2, size - 1, size], rng.integers(0, size, 6)]).clip(0, size))
    base = np.concatenate([(ks + 0.5) / size, ks / size]).astype(f)
    q = np.concatenate([base, np.nextafter(base, f(np.inf)), np.nextafter(base, f(-np.inf)),
                        np.array([0.0, 1.0, -0.0, np.nextafter(f(0), f(-1)), np.nextafter(f(1), f(2)), -5.25, 7.75, 1e9, -1e9, 1e36, -1e36], dtype=f)])
    return q.astype(f)


def tie_normal():
    """x with fl(0.57735026f * x) == 0.4f exactly, if fp32 has one: lambert sits on the floor's tie"""
    x = np.float32(0.4) / np.float32(0.57735026)
    for _ in range(8):
        x = np.nextafter(x, np.float32(0))
    for _ in range(17):
        if np.float32(np.float32(0.57735026) * x) == np.float32(0.4):
            return x
        x = np.nextafter(x, np.float32(1))
    return np.float32(0.4) / np.float32(0.57735026)


@functools.lru_cache(maxsize=None)
def shade_case(idx, count=24001):
    """hit records, one triangle per record, and the texture: (hits, ended, tris, tex, tex_other_alpha, reference)"""
    w, h = TEXTURES[idx]
    rng = np.random.default_rng(100 + idx)
    tex = make_texture(idx, w, h, rng)
    tex2 = tex.copy()
    tex2[..., 3] = 255 - tex2[..., 3]
    qu, qv = axis_coordinates(w, rng), axis_coordinates(h, rng)
    vfix = np.array([0.5 / h, 0.37, 1.0 / h], dtype=np.float32)
    ufix = np.array([0.5 / w, 0.61, 1.0 / w], dtype=np.float32)
    uv = np.concatenate([np.stack([qu, vfix[np.arange(len(qu)) % 3]], axis=1), np.stack([ufix[np.arange(len(qv)) % 3], qv], axis=1)])
    if len(uv) < count:
        uv = np.concatenate([uv, rng.uniform(-0.5, 1.5, (count - len(uv), 2)).astype(np.float32)])
    uv = uv[:count].astype(np.float32)
    i = np.arange(count)
    tris = np.zeros(count, dtype=L.TRIANGLE)
    tris.view(np.float32).reshape(count, 32)[:] = rng.uniform(-1, 1, (count, 32))                # positions and pads: never read
    for f in ("a_uv", "b_uv", "c_uv"):
        tris[f] = uv                                         # three equal corner uvs: the hit's uv is that uv up to rounding
    unit = rng.normal(size=(3, count, 3))
    unit /= np.linalg.norm(unit, axis=2, keepdims=True)
    kind = (i // 1) % N_NORMAL_KINDS
    r3 = np.float32(1 / np.sqrt(3))
    fixed = {1: (r3, r3, r3), 2: (-r3, -r3, -r3), 3: (tie_normal(), 0, 0), 4: (10, 0, 0), 5: (0, 1e5, 0), 6: (0, 0, 1e6),
             7: (0, 0, 0), 8: (113470, 0, 0), 9: (0, 113485, 0), 10: (0, 0, 113500)}
    for j, f in enumerate(("a_normal", "b_normal", "c_normal")):
        tris[f] = unit[j]
        for k, v in fixed.items():
            tris[f][kind == k] = v
    hits = np.zeros(count, dtype=L.HIT)
    bary = np.array(BARY, dtype=np.float32)[i % len(BARY)]
    hits["t"], hits["tri"], hits["u"], hits["v"] = 5.0, i, bary[:, 0], bary[:, 1]
    miss = (i % 13 == 12)
    hits["t"][miss], hits["tri"][miss], hits["u"][miss], hits["v"][miss] = L.MAX_FLOAT, 0, 0, 0
    if count > 40:
        hits["t"][40] = np.nan                               # not MAX_FLOAT: a hit, alpha 1
        hits["t"][41] = np.inf
        hits["t"][42] = -3.0
    ended = hits.copy()                                      # test 4: as lbvh_path_bounce marks a path that ended
    for j in {0, 63, 64, 65, count - 1}:
        if j < count:
            hits[j] = (L.MAX_FLOAT, 0, 0, 0)
            ended[j] = (L.MAX_FLOAT, 0xFFFFFFFF, 0, 0)
    ref = R.shade(hits, tris, tex)
    for a in (hits, ended, tris, tex, tex2) + ref:
        a.setflags(write=False)
    return hits, ended, tris, tex, tex2, ref


# SHADE_BOUND: image_reference.shade's third result, derived there.  With the textures of make_texture and these records:
# |du| <= 8U |uv| inside the texture (|uv| <= 1 where the taps differ; outside, both taps clamp to one texel and the slope is 0),
# so |dx| <= 10U w + 3U <= 3.1e-4 at w = 512; neighbouring texels differ by at most 0.6 of their value, so the slope term is at
# most 1.9e-4 of the result; the barycentric, lambert and bilinear roundings add less than 40U = 2.4e-6 of it (the tie and the
# floor: lambert >= 0.4, so its absolute error of a few U stays relative).  Half a half-ulp is at least 2^-12 = 2.44e-4 of the
# result.  check_shade asserts the inequality on every channel of every record.
def check_shade(idx, shade_fn, counts=()):
    hits, ended, tris, tex, tex2, (rgb, alpha, bound) = shade_case(idx)
    assert (bound < 0.5 * R.half_ulp(rgb)).all()
    got = shade_fn(hits, tris, tex, len(hits))
    ok = R.half_interval_ok(got[:, :3], rgb, bound)
    assert ok.all(), (TEXTURES[idx], np.argwhere(~ok)[:5], got[~ok.all(axis=1)][:5], rgb[~ok.all(axis=1)][:5])
    assert (got[:, 3] == np.where(alpha == 1.0, 0x3C00, 0)).all()
    assert not R.half_is_nan(got).any()
    assert (shade_fn(hits, tris, tex2, len(hits)) == got).all()                    # the fourth channel is never read
    assert (shade_fn(ended, tris, tex, len(hits)) == got).all()                    # 4.: ended-path records shade as plain misses
    for count in counts:
        assert (shade_fn(ended, tris, tex, count) == got[:count]).all()
    return got


def oracle_shade(hits, tris, tex, count):
    return O.shade(hits[:count], tris, tex).view(np.uint16).reshape(-1, 4)


@pytest.mark.parametrize("idx", range(len(TEXTURES)))
def test_oracle_shade_on_synthetic_records(idx):
    check_shade(idx, oracle_shade)


def test_shade_inputs_cover_their_edges():
    """the cases the issue names are really in the arrays: overflow of u * w, the floor and its tie, 65504 / 65520 / inf"""
    hits, _, tris, tex, _, (rgb, alpha, _) = shade_case(7)
    with np.errstate(over="ignore"):
        assert np.isinf(tris["a_uv"][:, 0] * np.float32(512)).sum() >= 2
    every = np.concatenate([shade_case(k)[3][..., :3].reshape(-1) for k in range(len(TEXTURES))])
    assert {0, 1, 254, 255} <= set(every.tolist())
    assert np.float32(np.float32(0.57735026) * tie_normal()) == np.float32(0.4)
    hits, _, tris, tex, _, (rgb, alpha, _) = shade_case(0)                  # the 1 x 1 texture: red = 1.0
    hb = R.to_half_bits(rgb[:, 0])
    assert (hb == 0x7BFF).any() and (hb == 0x7C00).any() and ((rgb[:, 0] > 65504) & (rgb[:, 0] < 65520)).any()
    assert (alpha == 0).sum() > 1000 and alpha[40] == 1


def gpu_shade_fn(ctx):
    cache = {}

    def fn(hits, tris, tex, count):
        key = (id(tris), id(tex))
        if key not in cache:
            for b in cache.pop("bufs", ()):
                b.dispose()
            cache.clear()
            cache[key] = cache["bufs"] = (up(ctx, tris), up(ctx, tex.reshape(-1, 4).view(np.uint32).reshape(-1)))
        tb, xb = cache[key]
        hb = up(ctx, hits)
        out = Guarded(ctx, count, np.uint64)
        N().check(ctx.handle, N().lib.lbvh_shade(ctx.handle, hb.device, count, tb.device, xb.device, tex.shape[1], tex.shape[0], out.device))
        got = out.read().view(np.uint16).reshape(-1, 4)
        hb.dispose()
        return got
    return fn


@gpu
@pytest.mark.parametrize("idx", range(len(TEXTURES)))
def test_shade_on_synthetic_records(ctx, idx):
    got = check_shade(idx, gpu_shade_fn(ctx), counts=(1, 255, 256, 257) if idx in (3, 6) else ())
    hits, _, tris, tex, _, _ = shade_case(idx)
    assert (got == oracle_shade(hits, tris, tex, len(hits))).all()                 # sharp tier


# ---- 5. lbvh_animate ---------------------------------------------------------------------------------------------------------

ANIMATE_N = (1, 2, 31, 32, 33, 255, 257, 4133)
COS_SIN = ((1.0, 0.0), (np.cos(np.pi / 2), np.sin(np.pi / 2)), (np.cos(np.pi), np.sin(np.pi)), (np.cos(0.37), np.sin(0.37)), (2.0, 0.0))
BODIES = ("one", "each", "descending")


@functools.lru_cache(maxsize=None)
def animate_case(n, bodies, far=True):
    rng = np.random.default_rng(n * 7 + len(bodies))
    rest = np.zeros(n, dtype=L.TRIANGLE)
    rest.view(np.float32).reshape(n, 32)[:] = rng.uniform(-1, 1, (n, 32))          # uv, pads and w lanes hold values of their own
    nb = 1 if bodies == "one" else n
    body = np.zeros(n, np.uint32) if bodies == "one" else np.arange(n, dtype=np.uint32) if bodies == "each" else np.arange(n, dtype=np.uint32)[::-1].copy()
    centres = np.zeros((nb, 4), dtype=np.float32)
    centres[:, :3] = rng.uniform(-1, 1, (nb, 3)) * 40 + (1e3 if far else 0.0)
    centres[:, 3] = rng.uniform(-1, 1, nb)
    for f in ("a", "b", "c"):
        rest[f] = (rng.uniform(-8, 8, (n, 3)) + centres[body][:, :3]).astype(np.float32)
    for a in (rest, body, centres):
        a.setflags(write=False)
    return rest, body, centres


# ANIMATE_BOUND: image_reference.animate — U (4 (|c| |x - cx| + |s| |z - cz|) + |x'|) * 1.01 for positions (about 1.2e-4 at 1e3),
# 3.03 U (|c| |nx| + |s| |nz|) for normals; results are fp32, so the comparison is |got - exact| <= bound, no half store.
def check_animate(n, bodies, c, s, got):
    rest, body, centres = animate_case(n, bodies)
    ref = R.animate(rest, body, centres, c, s)
    for f, (v, b) in ref.items():
        assert (np.abs(got[f].astype(np.float64) - v) <= b).all(), (f, n, bodies, c, s)
    gw, rw = words(got).reshape(n, 32), words(rest).reshape(n, 32)
    keep = [3, 7, 11] + list(range(12, 20)) + [23, 27, 31] + [1, 5, 9, 21, 25, 29]      # w lanes, uv + pad, every y
    assert (gw[:, keep] == rw[:, keep]).all()
    if (c, s) == (2.0, 0.0):                                    # the formula, not a rotation: twice as far from the centre
        ctr = centres[body][:, :3].astype(np.float64)
        assert np.allclose(got["a"][:, [0, 2]] - ctr[:, [0, 2]], 2 * (rest["a"][:, [0, 2]].astype(np.float64) - ctr[:, [0, 2]]), atol=1e-3)
        assert (got["a_normal"][:, 0] == 2 * rest["a_normal"][:, 0]).all()


@pytest.mark.parametrize("bodies", BODIES)
def test_oracle_animate_against_float64(bodies):
    for n in ANIMATE_N:
        for c, s in COS_SIN:
            check_animate(n, bodies, c, s, O.animate_cs(*animate_case(n, bodies), c, s))


@gpu
@pytest.mark.parametrize("bodies", BODIES)
def test_animate_every_word(ctx, bodies):
    for n in ANIMATE_N:
        rest, body, centres = animate_case(n, bodies)
        rb, bb, cb = up(ctx, rest), up(ctx, body), up(ctx, centres.reshape(-1))
        for c, s in COS_SIN:
            out = Guarded(ctx, n, L.TRIANGLE)
            N().check(ctx.handle, N().lib.lbvh_animate(ctx.handle, rb.device, n, bb.device, cb.device, float(np.float32(c)), float(np.float32(s)), out.device))
            got = out.read()
            assert (words(got) == words(O.animate_cs(rest, body, centres, c, s))).all()        # sharp tier: all 32 words
            check_animate(n, bodies, c, s, got)
        for b in (rb, bb, cb):
            b.dispose()


@gpu
@pytest.mark.parametrize("n", (2, 33, 257, 4133))
def test_animate_build_scene_equals_the_two_calls(ctx, n):
    rest, body, centres = animate_case(n, "descending", far=False)
    pt = H().DynamicPathTracer(ctx, rest, body, centres)
    c = pt.drawer.container
    f3 = C.POINTER(C.c_float)
    lib, h = N().lib, ctx.handle
    bufs = (c.triangle_data, c.keys, c.triangle_index, c.triangle_aabb, c.bvh_internal_node, c.bvh_leaf_node, c.bvh_data)

    def snapshot():
        c.get_all_gpu_data()
        return [words(b.local[: n - 1 if b is c.bvh_data else n]).copy() for b in bufs]

    for cs, sn in COS_SIN[3:] + COS_SIN[:1]:
        cs, sn = float(np.float32(cs)), float(np.float32(sn))
        N().check(h, lib.lbvh_animate(h, pt.rest.device, n, pt.body.device, pt.centres.device, cs, sn, c.triangle_data.device))
        pt.drawer.rebuild(fast=True)
        two = snapshot()
        pt.animate(1.0, fused=False)                            # another pose in between: the fused call must write everything
        N().check(h, lib.lbvh_animate_build_scene(
            h, pt.rest.device, pt.body.device, pt.centres.device, cs, sn, c.triangle_data.device, n, c.capacity,
            c.box_min.ctypes.data_as(f3), c.box_max.ctypes.data_as(f3), c.keys.device, c.triangle_index.device, c.triangle_aabb.device,
            c.bvh_internal_node.device, c.bvh_leaf_node.device, c.bvh_data.device, L.BUILD_RESET_NODES | L.BUILD_FAST_SCENE))
        one = snapshot()
        for x, y in zip(one, two):
            assert (x == y).all()
        assert (one[0] == words(O.animate_cs(rest, body, centres, cs, sn))).all()
    pt.drawer.on_destroy()


# ---- 6. lbvh_path_scatter in isolation ----------------------------------------------------------------------------------------

def scatter_triangles():
    """integer corners: 0 normal +Y, 1 the other winding (-Y), 2 three equal corners, 3 collinear, 4 normal +Z, 5 normal (-3,-2,6)/7"""
    t = np.zeros(6, dtype=L.TRIANGLE)
    t["a"] = [(0, 0, 0), (0, 0, 0), (2, 3, 4), (0, 0, 0), (0, 0, 0), (1, 1, 1)]
    t["b"] = [(0, 0, 4), (4, 0, 0), (2, 3, 4), (1, 2, 3), (3, 0, 0), (3, 1, 2)]
    t["c"] = [(4, 0, 0), (0, 0, 4), (2, 3, 4), (3, 6, 9), (0, 4, 0), (1, 4, 2)]
    return t


@functools.lru_cache(maxsize=None)
def scatter_case(count, seed=5):
    rng = np.random.default_rng(count + seed)
    st = np.zeros(count, dtype=L.PATH_STATE)
    st.view(np.uint32).reshape(count, 16)[:] = rng.integers(0, 1 << 32, (count, 16), dtype=np.uint64).astype(np.uint32)   # pads, dead paths
    i = np.arange(count)
    d = rng.normal(size=(count, 3))
    d[i % 4 == 1] *= (1, -1, 1)
    st["dir"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    st["origin"] = rng.uniform(-10, 10, (count, 3))
    st["throughput"] = rng.uniform(0.1, 1.0, (count, 3))
    st["radiance"] = rng.uniform(0.0, 2.0, (count, 3))
    st["alpha"] = np.where(i % 2 == 0, 0.0, 0.25)
    live = i % 5 != 4
    st["alive"] = np.where(live, 1, 0)
    dead = st[~live].copy()
    st2 = st.copy()
    st2[~live] = dead
    hits = np.zeros(count, dtype=L.HIT)
    hits["t"], hits["tri"] = rng.uniform(0.5, 20.0, count), i % 6
    hits["u"], hits["v"] = rng.uniform(0, 0.5, count), rng.uniform(0, 0.5, count)
    hits["t"][i % 3 == 2] = L.MAX_FLOAT
    hits["tri"][i % 3 == 2] = 0
    hits["tri"][i % 9 == 8] = 0xFFFFFFFF                      # a caller's prefill: an ordinary miss to lbvh_path_scatter
    hits["t"][i % 31 == 7] = np.nan                          # not < MAX_FLOAT: a miss
    hits["tri"][i % 31 == 7] = 0
    hits["tri"][hits["t"] < L.MAX_FLOAT] %= 6
    st.setflags(write=False); hits.setflags(write=False)
    return st, hits


# SCATTER_BOUND: image_reference.scatter, per field and per path.  States: |origin| <= 10, |t| <= 20, throughput and radiance <= 3.
def check_scatter(count, bounce, seed, albedo, got):
    st, hits = scatter_case(count)
    tris = scatter_triangles()
    ref = R.scatter(tris, hits, st, bounce, seed, albedo)
    assert not ref["ambiguous"].any()
    for f in ("radiance", "origin", "throughput", "dir"):
        assert (np.abs(got[f].astype(np.float64) - ref[f]) <= ref[f + "_bound"]).all(), (f, count, bounce)
    assert (got["alive"] == ref["alive"]).all() and (got["alpha"] == ref["alpha"]).all()
    gw, sw = words(got).reshape(count, 16), words(st).reshape(count, 16)
    assert (gw[~ref["touched"]] == sw[~ref["touched"]]).all()                  # dead on entry: all 16 words
    assert (gw[:, [7, 11]] == sw[:, [7, 11]]).all()                            # pads
    missed = ref["touched"] & ~ref["hit"]
    assert (gw[missed][:, 4:12] == sw[missed][:, 4:12]).all() and (gw[missed][:, 0:3] == sw[missed][:, 0:3]).all()
    hit = ref["hit"]
    side = (got["dir"][hit].astype(np.float64) * ref["normal"][hit]).sum(axis=1)
    assert (side >= -1e-6).all()                                                # stays on the incoming ray's side
    assert ((st["dir"][hit].astype(np.float64) * ref["normal"][hit]).sum(axis=1) <= 0).all()
    if bounce == 0:
        assert (got["alpha"][hit] == 1).all()
    else:
        assert (got["alpha"] == st["alpha"]).all()
    degenerate = hit & np.isin(hits["tri"], (2, 3))
    assert degenerate.sum() > 0 or count < 20
    assert (np.abs(ref["normal"][degenerate]) == (0, 1, 0)).all()


def oracle_scatter(count, bounce, seed, albedo):
    st, hits = scatter_case(count)
    return O.path_scatter(O.TrianglesOnly(scatter_triangles()), hits, st.copy(), bounce, seed, albedo)


@pytest.mark.parametrize("bounce", (0, 3))
def test_oracle_scatter_against_float64(bounce):
    for count in (1, 513, 6151):
        check_scatter(count, bounce, 9, 0.7, oracle_scatter(count, bounce, 9, 0.7))


def gpu_scatter(ctx, tris, hits, st, bounce, seed, albedo):
    tb, hb = up(ctx, tris), up(ctx, hits)
    out = Guarded(ctx, len(st), L.PATH_STATE, init=st)
    s = N().Scene()
    s.n, s.triangles = len(tris), tb.device.value
    N().check(ctx.handle, N().lib.lbvh_path_scatter(ctx.handle, C.byref(s), hb.device, len(st), bounce, seed, albedo, out.device))
    got = out.read()
    assert (hb.get_data()[: len(hits)].view(np.uint32) == words(hits)).all()    # lbvh_path_scatter leaves the records alone
    tb.dispose(); hb.dispose()
    return got


@gpu
@pytest.mark.parametrize("bounce", (0, 3))
def test_scatter_in_isolation(ctx, bounce):
    for count in (1, 511, 512, 513, 2047, 2048, 2049, 6151):
        st, hits = scatter_case(count)
        got = gpu_scatter(ctx, scatter_triangles(), hits, st, bounce, 9, 0.7)
        assert (words(got) == words(oracle_scatter(count, bounce, 9, 0.7))).all()        # sharp tier: the whole state
        check_scatter(count, bounce, 9, 0.7, got)


STAT_N = 1 << 20
STAT_SEED = 11


def stat_inputs():
    st = np.zeros(STAT_N, dtype=L.PATH_STATE)
    st["dir"], st["origin"], st["throughput"], st["alive"] = (0, -1, 0), (1, 5, 1), 1, 1
    hits = np.zeros(STAT_N, dtype=L.HIT)
    hits["t"] = 5.0                                           # triangle 0: normal +Y
    return st, hits


def check_scatter_statistics(run):
    """run(bounce, seed) -> new directions [N, 3] of N paths that all hit a triangle with normal +Y from above.
    A cosine-weighted lobe about +Y: E d.y = 2/3 with variance 1/18; E d.x = E d.z = 0 with variance 1/6.  Margins: 5 standard
    errors at N = 2^20: 5 sqrt(1 / (18 N)) = 1.151e-3, 5 sqrt(1 / (6 N)) = 1.993e-3; correlations |r| < 5 / sqrt(N) = 4.883e-3."""
    n = STAT_N
    figures = {}
    d0 = run(0, STAT_SEED).astype(np.float64)
    # the paths whose first seven tries all fail (0.2146^7 of them: about 22 here) take the eighth try or, failing that too, the
    # pole (0, 0, 1): the only paths that tell eight tries from seven.  Against the float64 reference, each one.
    late = np.nonzero(R.marsaglia_rejections(STAT_SEED, np.arange(n), 0) >= 7)[0]
    assert len(late) >= 8 and (R.marsaglia_rejections(STAT_SEED, late, 0) == 8).any()
    st, hits = stat_inputs()
    ref = R.scatter(scatter_triangles(), hits[late], st[late], 0, STAT_SEED, 0.7, index=late)
    assert not ref["ambiguous"].any() and (np.abs(d0[late] - ref["dir"]) <= ref["dir_bound"]).all()
    d1 = run(1, STAT_SEED).astype(np.float64)
    d2 = run(0, STAT_SEED + 1).astype(np.float64)
    for name, d in (("bounce 0", d0), ("bounce 1", d1), ("seed + 1", d2)):
        assert (np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 4 * 2.0 ** -23).all()
        assert (d[:, 1] >= -1e-6).all()
        my, mx, mz = d[:, 1].mean(), d[:, 0].mean(), d[:, 2].mean()
        figures[name] = (my, mx, mz)
        assert abs(my - 2.0 / 3.0) < 5 * np.sqrt(1 / (18 * n)), (name, my)
        assert abs(mx) < 5 * np.sqrt(1 / (6 * n)) and abs(mz) < 5 * np.sqrt(1 / (6 * n)), (name, mx, mz)

    def r(a, b):
        return float(np.corrcoef(a, b)[0, 1])
    for k, axis in enumerate("xyz"):
        figures["r " + axis] = (r(d0[:-1, k], d0[1:, k]), r(d0[:, k], d1[:, k]), r(d0[:, k], d2[:, k]))
        assert all(abs(v) < 5 / np.sqrt(n) for v in figures["r " + axis]), (axis, figures["r " + axis])
    print("scatter statistics:", figures)
    return figures


def test_oracle_scatter_statistics():
    st, hits = stat_inputs()
    tris = O.TrianglesOnly(scatter_triangles())
    check_scatter_statistics(lambda bounce, seed: O.path_scatter(tris, hits, st.copy(), bounce, seed, 0.7)["dir"])


@gpu
def test_scatter_statistics(ctx):
    st, hits = stat_inputs()
    check_scatter_statistics(lambda bounce, seed: gpu_scatter(ctx, scatter_triangles(), hits, st, bounce, seed, 0.7)["dir"])


# ---- 7. lbvh_path_begin ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("frame", ((1, 1), (17, 1), (1, 17), (33, 47)))
def test_path_begin_small_frames(ctx, frame):
    cam = scenes.camera(frame[0], frame[1], (3.0, -2.0, 120.0))
    ncam = N().Camera.from_dict(cam)
    out = Guarded(ctx, frame[0] * frame[1], L.PATH_STATE)
    N().check(ctx.handle, N().lib.lbvh_path_begin(ctx.handle, C.byref(ncam), out.device))
    got = out.read()
    assert (words(got) == words(O.path_begin(cam))).all()
    assert (np.abs(np.linalg.norm(got["dir"].astype(np.float64), axis=1) - 1.0) <= 4 * 2.0 ** -23).all()
    assert (got["alive"] == 1).all() and (got["throughput"] == 1).all() and (words(got).reshape(-1, 16)[:, 12:] == 0).all()
