"""Independent references for the image tail (lbvh_shade, lbvh_compose, lbvh_animate, lbvh_path_scatter, lbvh_path_resolve),
written in plain numpy from the text of include/lbvh.h — not from oracle/lbvh_oracle.c.  float64 throughout, except where the
contract itself is "in fp32" (compose) or "IEEE half, round to nearest even" (the RGBA16F stores: numpy's float16 cast).

Every *_bound function returns an a-priori error bound of the fp32 evaluation against the float64 one: from fp32 unit roundoff
U = 2^-24, the number of rounded operations and the magnitudes of the inputs.  None of them looks at a result under test."""
import numpy as np

U = 2.0 ** -24                       # fp32 unit roundoff (round to nearest)
MAX_FLOAT = np.float32(2139095040.0)
LIGHT = float(np.float32(0.57735026))  # the scalar lightDir, as the fp32 value the header names
FLOOR = float(np.float32(0.4))


# ---- IEEE half ---------------------------------------------------------------------------------------------------------------

def to_half_bits(x):
    """round-to-nearest-even float -> half, as words (numpy's cast; NaN payloads are numpy's own and compared by class only)"""
    with np.errstate(all="ignore"):
        return np.asarray(x).astype(np.float16).view(np.uint16)


def half_is_nan(bits):
    bits = np.asarray(bits, dtype=np.uint16)
    return ((bits & 0x7C00) == 0x7C00) & ((bits & 0x03FF) != 0)


def half_words_match(got, ref):
    """word for word; where the reference is a NaN any NaN will do"""
    got, ref = np.asarray(got, dtype=np.uint16), np.asarray(ref, dtype=np.uint16)
    nan = half_is_nan(ref)
    return np.where(nan, half_is_nan(got), got == ref)


def torch_half_bits(x32):
    """torch's CPU float -> half, or None without torch (the cross-check of the numpy cast)"""
    try:
        import torch
    except Exception:
        return None
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).half().view(torch.int16).numpy().view(np.uint16)


def half_ulp(e):
    """spacing of the halves around |e|: the subnormal spacing 2^-24 below 2^-14; past the largest half the spacing an unbounded
    exponent would give, which is what round-to-nearest's overflow rule (65520 and up become inf) is defined by"""
    a = np.abs(np.asarray(e, dtype=np.float64))
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (ex - 10)


def half_interval_ok(got_bits, e, bound):
    """got = RN_half(c) for some c in [e - bound, e + bound]: RN is monotone, so RN(e - bound) <= got <= RN(e + bound)"""
    with np.errstate(all="ignore"):
        lo = (np.asarray(e) - bound).astype(np.float16).astype(np.float64)
        hi = (np.asarray(e) + bound).astype(np.float16).astype(np.float64)
        g = np.asarray(got_bits, dtype=np.uint16).view(np.float16).astype(np.float64)
    return (g >= lo) & (g <= hi)


def conversion_sweep():
    """fp32 inputs of the half-store sweep: every finite half of both signs, every midpoint between neighbouring halves with its
    fp32 neighbours, the overflow threshold, the underflow threshold, the ends of fp32, zeros, infinities and NaNs."""
    pos = np.arange(0, 0x7C00, dtype=np.uint16)
    h = np.concatenate([pos, pos | 0x8000]).view(np.float16).astype(np.float32)               # exact
    p = pos.view(np.float16).astype(np.float64)
    mid = ((p[:-1] + p[1:]) / 2).astype(np.float32)                                            # exact: one more bit than a half
    assert (mid.astype(np.float64) == (p[:-1] + p[1:]) / 2).all()
    mids = np.concatenate([mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf))])
    mids = np.concatenate([mids, -mids])
    f = np.float32
    edge = np.array([65520.0, np.nextafter(f(65520.0), f(0)), -65520.0, -np.nextafter(f(65520.0), f(0)), np.nextafter(f(65520.0), f(np.inf)),
                     2.0 ** -25, np.nextafter(f(2.0 ** -25), f(1)), -2.0 ** -25, np.nextafter(f(2.0 ** -25), f(0)),
                     np.finfo(f).max, -np.finfo(f).max, 1e-40, -1e-40, 1.4e-45, 0.0, -0.0, np.inf, -np.inf], dtype=f)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA55555, 0xFFFFFFFF, 0x7F801000, 0x7FFFE000],
                    dtype=np.uint32).view(f)
    return np.concatenate([h, mids, edge, nans])


# ---- shade -------------------------------------------------------------------------------------------------------------------

def _bary(hits, tris, field, k):
    bu, bv = hits["u"].astype(np.float64), hits["v"].astype(np.float64)
    w = 1.0 - bu - bv
    a, b, c = (tris[p + field][:, k].astype(np.float64) for p in ("a_", "b_", "c_"))
    val = w * a + bu * b + bv * c
    # fp32: w = (1 - u) - v, two roundings, |error| <= 2U(1 + |u| + |v|), carried by a; then three products and two sums,
    # gamma_3 < 4U on the sum of the magnitudes
    err = U * (4.0 * (np.abs(w * a) + np.abs(bu * b) + np.abs(bv * c)) + 2.0 * (1.0 + np.abs(bu) + np.abs(bv)) * np.abs(a))
    return val, err


def shade(hits, triangles, tex):
    """lbvh_shade in float64.  Returns (rgb [n, 3], alpha [n], bound [n, 3]): the exact colour, the alpha flag, and the bound
    on |fp32 colour - exact| before the half store.
    Clamp addressing: texel index clamped to [0, w - 1] on the exact coordinate, so a uv however large gives the edge texel.
    Bound, with U = 2^-24 (SHADE_BOUND in the tests refers here):
      uv, normal: _bary above.
      lambert = max(0.4, (l nx + l ny) + l nz): l * (error of n) + gamma_3 * l * sum|n_k|  (max is 1-Lipschitz).
      x = u w - 0.5: |dx| <= |du| w + 2U(|u| w + 0.5) — the sampler's slope term |du| * w plus the product's and the sum's rounding;
        the weights fx, 1 - fx carry dx + 2U.  Bilinear interpolation is continuous and piecewise linear with slope at most
        Dx = the largest difference of two horizontally neighbouring texels (Dy vertically), and flat where both taps clamp to the
        same edge texel (x + dx < 0 or x - dx >= w - 1; always when w == 1).
      colour = texel / 255 (one rounding), three products and sums of non-negative terms per axis: 8U relative.
      colour * lambert: one more rounding."""
    hits = np.ascontiguousarray(hits)
    tris_all = np.ascontiguousarray(triangles)
    tex = np.asarray(tex, dtype=np.uint8)
    H, W = tex.shape[:2]
    alpha = (hits["t"] != MAX_FLOAT).astype(np.float64)             # a NaN t is "not MAX_FLOAT": alpha 1
    # the triangle the record names: 0 on a traced miss, and 0 for the mark of an ended path, {MAX_FLOAT, 0xFFFFFFFF, 0, 0}
    tri = np.where((hits["t"] == MAX_FLOAT) & (hits["tri"] == 0xFFFFFFFF), 0, hits["tri"])
    t = tris_all[tri]
    tu, du = _bary(hits, t, "uv", 0)
    tv, dv = _bary(hits, t, "uv", 1)
    n, dn = zip(*(_bary(hits, t, "normal", k) for k in range(3)))
    s = LIGHT * (n[0] + n[1] + n[2])
    lam = np.maximum(FLOOR, s)
    dlam = LIGHT * (dn[0] + dn[1] + dn[2]) + 4.0 * U * LIGHT * (np.abs(n[0]) + np.abs(n[1]) + np.abs(n[2]))
    T = tex[..., :3].astype(np.float64) / 255.0                     # the fourth channel is never read

    def axis(q, dq, size):
        x = q * size - 0.5
        dx = dq * size + 2.0 * U * (np.abs(q) * size + 0.5)
        fl = np.floor(x)
        i0 = np.clip(fl, 0, size - 1).astype(np.int64)
        i1 = np.clip(fl + 1, 0, size - 1).astype(np.int64)
        flat = (x + dx < 0) | (x - dx >= size - 1) | (size == 1)
        return i0, i1, x - fl, np.where(flat, 0.0, dx + 2.0 * U)

    x0, x1, fx, ex = axis(tu, du, W)
    y0, y1, fy, ey = axis(tv, dv, H)
    fx, fy = fx[:, None], fy[:, None]
    col = (T[y0, x0] * (1 - fx) + T[y0, x1] * fx) * (1 - fy) + (T[y1, x0] * (1 - fx) + T[y1, x1] * fx) * fy
    Dx = np.abs(np.diff(T, axis=1)).max(axis=(0, 1)) if W > 1 else np.zeros(3)
    Dy = np.abs(np.diff(T, axis=0)).max(axis=(0, 1)) if H > 1 else np.zeros(3)
    dcol = ex[:, None] * Dx[None, :] + ey[:, None] * Dy[None, :] + 8.0 * U * col
    rgb = col * lam[:, None]
    bound = lam[:, None] * dcol + col * dlam[:, None] + 2.0 * U * np.abs(rgb)
    return rgb, alpha, bound


# ---- compose -----------------------------------------------------------------------------------------------------------------

def compose32(bg_bits, ob_bits):
    """the contract's own definition: out.rgb = bg + a * (ob - bg) with one fp32 rounding per operation, out.a = 1; halves in
    and out as words [n, 4]"""
    bg = np.asarray(bg_bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    ob = np.asarray(ob_bits, dtype=np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(all="ignore"):
        a = ob[:, 3:4]
        d = (ob[:, :3] - bg[:, :3]).astype(np.float32)
        t = (a * d).astype(np.float32)
        r = (bg[:, :3] + t).astype(np.float32)
    out = np.empty(bg.shape, dtype=np.uint16)
    out[:, :3] = to_half_bits(r)
    out[:, 3] = 0x3C00
    return out


def compose64(bg_bits, ob_bits):
    """float64 value and the bound of the fp32 evaluation: d = ob - bg, t = a d, r = bg + t, one rounding each:
    |error| <= U (2 |a d| + |r|) to first order; 1.01 covers the second-order terms."""
    bg = np.asarray(bg_bits, dtype=np.uint16).view(np.float16).astype(np.float64)
    ob = np.asarray(ob_bits, dtype=np.uint16).view(np.float16).astype(np.float64)
    a = ob[:, 3:4]
    ad = a * (ob[:, :3] - bg[:, :3])
    r = bg[:, :3] + ad
    return r, 1.01 * U * (2.0 * np.abs(ad) + np.abs(r))


# ---- animate -----------------------------------------------------------------------------------------------------------------

def animate(rest, body, centres, c, s):
    """rotation about Y through the body centre, float64: returns {field: (value [n, 3], bound [n, 3])} for the six moved
    fields.  Bound: x - cx (one rounding), two products and their sum (gamma_3 < 4U on |c||x - cx| + |s||z - cz|), + cx (one
    more, on the result): U (4 (|c| X + |s| Z) + |x'|) * 1.01; the normals lack the two translations: 3U (|c||nx| + |s||nz|) * 1.01.
    y is copied: bound 0."""
    c, s = float(np.float32(c)), float(np.float32(s))
    ctr = np.asarray(centres, dtype=np.float32).reshape(-1, 4)[np.asarray(body)].astype(np.float64)
    out = {}
    for f in ("a", "b", "c"):
        p = rest[f].astype(np.float64)
        x, z = p[:, 0] - ctr[:, 0], p[:, 2] - ctr[:, 2]
        v = np.stack([c * x + s * z + ctr[:, 0], p[:, 1], c * z - s * x + ctr[:, 2]], axis=1)
        m = np.abs(c * x) + np.abs(s * z), np.abs(c * z) + np.abs(s * x)
        b = np.stack([1.01 * U * (4 * m[0] + np.abs(v[:, 0])), np.zeros(len(p)), 1.01 * U * (4 * m[1] + np.abs(v[:, 2]))], axis=1)
        out[f] = (v, b)
    for f in ("a_normal", "b_normal", "c_normal"):
        p = rest[f].astype(np.float64)
        x, z = p[:, 0], p[:, 2]
        v = np.stack([c * x + s * z, p[:, 1], c * z - s * x], axis=1)
        b = np.stack([3.03 * U * (np.abs(c * x) + np.abs(s * z)), np.zeros(len(p)), 3.03 * U * (np.abs(c * z) + np.abs(s * x))], axis=1)
        out[f] = (v, b)
    return out


# ---- scatter -----------------------------------------------------------------------------------------------------------------

def pcg_hash(v):
    v = np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF
    state = (v * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return (word >> 22) ^ word


def path_rnd(seed, index, bounce, draw):
    """PCG hash of (seed, path index, bounce, draw), top 24 bits as a number in [0, 1)"""
    index = np.asarray(index, dtype=np.uint64)
    h = pcg_hash(pcg_hash(pcg_hash((seed + 0x9E3779B9 * index) & 0xFFFFFFFF) + bounce) + draw)
    return (h >> 8).astype(np.float64) / 16777216.0


def marsaglia_rejections(seed, index, bounce, tries=8):
    """how many of the first `tries` pairs of draws fall outside the unit disc, one after the other from the first"""
    index = np.asarray(index, dtype=np.uint64)
    n, going = np.zeros(len(index), dtype=np.int64), np.ones(len(index), dtype=bool)
    for k in range(0, 2 * tries, 2):
        x1 = 2.0 * path_rnd(seed, index, bounce, k) - 1.0
        x2 = 2.0 * path_rnd(seed, index, bounce, k + 1) - 1.0
        going &= ~(x1 * x1 + x2 * x2 < 1.0)
        n += going
    return n


def scatter(tris, hits, states, bounce, seed, albedo, index=None):
    """lbvh_path_scatter in float64 on copies of the states (`index`: their path indices, 0, 1, 2, ... if None).  Returns a dict of float64 arrays and bounds:
    radiance/throughput/origin/dir, alive, alpha, the flipped geometric normal, `touched` (live on entry) and `ambiguous`
    (a Marsaglia test x1^2 + x2^2 < 1 within 4U of 1: fp32 may decide it the other way; the tests choose seeds with none).
    Bounds (U = 2^-24):
      sky: s = 0.5 (dy + 1), (1 - s) + s c: eight roundings on values <= 1 -> 8U; times the throughput (+1) and added to the
           radiance (+1 on the result): U (10 |thr| + 2 |rad'|).
      origin' = o + d t: product and sum: U (2 |d t| + |o'|) * 1.01.   throughput' = thr * albedo: one rounding, U |thr'| * 1.01.
      direction: n from integer-coordinate triangles is exact up to the division by its length: 3U.  p = (2 x1 r, 2 x2 r, 1 - 2 ss)
           with r = sqrt(1 - ss): 1 - ss carries 3U absolute, the root 3U / (2 r) + U, so |dp| <= 4U + 3U / r.  v = n + p and
           d = v / |v|: 2 (dn + dp + U) / |v| + 3U."""
    albedo = float(np.float32(albedo))
    n_paths = len(states)
    st = {f: states[f].astype(np.float64) for f in ("origin", "dir", "throughput", "radiance")}
    alive_in = states["alive"] != 0
    alpha = states["alpha"].astype(np.float64).copy()
    missed = ~(hits["t"] < MAX_FLOAT)
    miss = alive_in & missed
    hit = alive_in & ~missed
    t = hits["t"].astype(np.float64)
    sk = 0.5 * (st["dir"][:, 1] + 1.0)
    sky = (1.0 - sk)[:, None] + sk[:, None] * np.array([0.5, float(np.float32(0.7)), 1.0])[None, :]
    rad = np.where(miss[:, None], st["radiance"] + st["throughput"] * sky, st["radiance"])
    rad_b = np.where(miss[:, None], U * (10 * np.abs(st["throughput"]) + 2 * np.abs(rad)), 0.0)
    if bounce == 0:
        alpha[hit] = 1.0
    tr = tris[np.where(hit, hits["tri"], 0)]
    a, b, c = (tr[f].astype(np.float64) for f in ("a", "b", "c"))
    n = np.cross(b - a, c - a)
    nl = np.linalg.norm(n, axis=1)
    n = np.where((nl > 0)[:, None], n / np.where(nl > 0, nl, 1.0)[:, None], np.array([0.0, 1.0, 0.0])[None, :])
    flip = (n * st["dir"]).sum(axis=1) > 0
    n = np.where(flip[:, None], -n, n)
    dt = st["dir"] * t[:, None]
    org = np.where(hit[:, None], st["origin"] + np.where(hit[:, None], dt, 0.0), st["origin"])
    org_b = np.where(hit[:, None], 1.01 * U * (2 * np.abs(np.where(hit[:, None], dt, 0.0)) + np.abs(org)), 0.0)
    thr = np.where(hit[:, None], st["throughput"] * albedo, st["throughput"])
    thr_b = np.where(hit[:, None], 1.01 * U * np.abs(thr), 0.0)
    idx = np.arange(n_paths, dtype=np.uint64) if index is None else np.asarray(index, dtype=np.uint64)
    p = np.tile(np.array([0.0, 0.0, 1.0]), (n_paths, 1))
    done = np.zeros(n_paths, dtype=bool)
    amb = np.zeros(n_paths, dtype=bool)
    rmin = np.ones(n_paths)
    for k in range(0, 16, 2):                                   # Marsaglia 1972, at most 8 tries
        x1 = 2.0 * path_rnd(seed, idx, bounce, k) - 1.0
        x2 = 2.0 * path_rnd(seed, idx, bounce, k + 1) - 1.0
        ss = x1 * x1 + x2 * x2
        amb |= ~done & (np.abs(ss - 1.0) < 4 * U)
        take = ~done & (ss < 1.0)
        r = np.sqrt(np.where(take, 1.0 - ss, 1.0))
        p[take] = np.stack([2 * x1 * r, 2 * x2 * r, 1 - 2 * ss], axis=1)[take]
        rmin[take] = r[take]
        done |= take
    v = n + p
    vl = np.linalg.norm(v, axis=1)
    d = np.where((vl > 1e-6)[:, None], v / np.where(vl > 0, vl, 1.0)[:, None], n)
    dp = 4 * U + 3 * U / np.maximum(rmin, 1e-12)
    d_b = 2 * (3 * U + dp + U) / np.maximum(vl, 1e-12) + 3 * U
    new_dir = np.where(hit[:, None], d, st["dir"])
    return {"radiance": rad, "radiance_bound": rad_b, "origin": org, "origin_bound": org_b, "throughput": thr, "throughput_bound": thr_b,
            "dir": new_dir, "dir_bound": np.where(hit, d_b, 0.0)[:, None] * np.ones(3), "alive": (alive_in & ~missed).astype(np.uint32),
            "alpha": alpha, "normal": n, "touched": alive_in, "hit": hit, "ambiguous": amb & hit}
