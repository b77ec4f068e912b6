"""Host side of the hot path: the reference's C# classes mirrored over the C ABI.

Same names, call order and argument meaning as Assets/_Scripts/{DataBuffer, MeshBufferContainer,
ComputeBufferSorter, BVHConstructor, RaytracingMeshDrawer}.cs, so a test reads like the
reference's Awake()/Update().  Every method is one C-ABI call (include/lbvh.h); nothing here
computes.  (The compiled-language twin of this file is host/lbvh_host.hpp; the C# [DllImport]
shim a Unity maintainer would add is in INTEGRATION.md.)
"""
import ctypes as C

import numpy as np

from . import _native as N
from . import layouts as L
from .scenes import capacity_for

# RaytracingMeshDrawer.point_crossings' default directions: three fp32 unit vectors, no two in a coordinate plane together
DEFAULT_DIRS = (np.array([[1.0, 1.0, 1.0], [-1.0, 2.0, 3.0], [4.0, -1.0, 2.0]]) /
                np.sqrt([[3.0], [14.0], [21.0]])).astype(np.float32)


def inside(parity, n_dirs):
    """Inside / outside from lbvh_point_crossings words: more than half of the n_dirs directions saw an odd crossing count."""
    p = np.asarray(parity, dtype=np.uint32)
    ones = np.zeros(p.shape, dtype=np.int64)
    for j in range(n_dirs):
        ones += (p >> np.uint32(j)) & np.uint32(1)
    return ones > n_dirs / 2


# ---- plane builders for lbvh_region_overlaps: conveniences, computed in float64 and rounded once to fp32.  The contract is on
# the planes (include/lbvh.h), not on these builders: a plane {nx, ny, nz, d} keeps n . x + d >= 0, normals point inward. ------------

def _regions(planes):
    out = np.zeros(planes.shape[:-2], dtype=L.REGION)
    out["plane"] = planes.astype(np.float32)
    return out if out.ndim else out.reshape(1)


def aabb_planes(lo, hi):
    """The box [lo, hi] (arrays of shape (..., 3)) as layouts.REGION records: unit axis normals, d = -lo for +axis, d = +hi for -axis
    (exact in fp32 for fp32 bounds: in TOUCHING mode the region is lbvh_box_overlaps' box)."""
    lo, hi = np.broadcast_arrays(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
    planes = np.zeros(lo.shape[:-1] + (6, 4))
    for k in range(3):
        planes[..., 2 * k, k], planes[..., 2 * k, 3] = 1.0, -lo[..., k]
        planes[..., 2 * k + 1, k], planes[..., 2 * k + 1, 3] = -1.0, hi[..., k]
    return _regions(planes)


def obb_planes(centre, axes3x3, half_extents):
    """The oriented box { centre + sum_k s_k * axes3x3[k] : |s_k| <= half_extents[k] } (rows of axes3x3: the box's axes; they are
    normalised here and assumed orthogonal) as layouts.REGION records: planes {+-axis_k, half_extents[k] -+ axis_k . centre}.
    Shapes (..., 3), (..., 3, 3), (..., 3)."""
    c, ax, he = np.asarray(centre, dtype=np.float64), np.asarray(axes3x3, dtype=np.float64), np.asarray(half_extents, dtype=np.float64)
    ax = ax / np.linalg.norm(ax, axis=-1, keepdims=True)
    along = (ax * c[..., None, :]).sum(axis=-1)                       # axis_k . centre
    planes = np.zeros(np.broadcast_shapes(c.shape[:-1], ax.shape[:-2], he.shape[:-1]) + (6, 4))
    for k in range(3):
        planes[..., 2 * k, :3], planes[..., 2 * k, 3] = ax[..., k, :], he[..., k] - along[..., k]
        planes[..., 2 * k + 1, :3], planes[..., 2 * k + 1, 3] = -ax[..., k, :], he[..., k] + along[..., k]
    return _regions(planes)


def obb_half_axes(half_extents, rotation3x3=None):
    """The three half-axis vectors (ax, ay, az) of layouts.BOX_RAY for a box of the given half extents turned by rotation3x3, whose
    COLUMNS are the box's axes in world space (a rotation matrix as it multiplies a column vector; None: an AABB): ax =
    rotation[:, 0] * half_extents[0] and so on, rounded to fp32 once.  Shapes (..., 3) and (..., 3, 3) -> three arrays (..., 3).
    Nothing is normalised or made orthogonal: a sheared matrix gives a sheared box, which lbvh_box_cast takes as it is."""
    he = np.asarray(half_extents, dtype=np.float64)
    rot = np.eye(3) if rotation3x3 is None else np.asarray(rotation3x3, dtype=np.float64)
    axes = np.swapaxes(rot, -1, -2) * he[..., :, None]                # row k = column k of the rotation, scaled
    return tuple(np.ascontiguousarray(axes[..., k, :], dtype=np.float32) for k in range(3))


def capsule_shapes(origin, axis, radius):
    """layouts.CAPSULE records for lbvh_capsule_overlaps: the capsules with the segments origin .. origin + axis (shapes (..., 3),
    broadcast against each other) and the given radii, rounded to fp32 once."""
    o, h = np.broadcast_arrays(np.asarray(origin, dtype=np.float32), np.asarray(axis, dtype=np.float32))
    out = np.zeros(o.shape[:-1], dtype=L.CAPSULE)
    out["origin"], out["axis"], out["radius"] = o, h, np.asarray(radius, dtype=np.float32)
    return out if out.ndim else out.reshape(1)


def segment_queries(origins, axes, max_dist2=np.inf):
    """layouts.SEGMENT_QUERY records for segment_closest_points / segment_within_distance: the segments origins .. origins + axes
    (shapes (..., 3), broadcast against each other) with the given SQUARED search radii (+inf: unbounded), rounded to fp32 once."""
    o, h = np.broadcast_arrays(np.asarray(origins, dtype=np.float32), np.asarray(axes, dtype=np.float32))
    out = np.zeros(o.shape[:-1], dtype=L.SEGMENT_QUERY)
    out["origin"], out["axis"], out["max_dist2"] = o, h, np.asarray(max_dist2, dtype=np.float32)
    return out if out.ndim else out.reshape(1)


def obb_shapes(centre, half_extents, rotation3x3=None):
    """layouts.OBB records for lbvh_obb_overlaps: boxes of the given half extents turned by rotation3x3 (COLUMNS = the box's axes in
    world space; None: AABBs) about `centre`, the half-axis vectors as obb_half_axes makes them.  Shapes (..., 3), (..., 3) and
    (..., 3, 3)."""
    ax, ay, az = obb_half_axes(half_extents, rotation3x3)
    c = np.asarray(centre, dtype=np.float32)
    out = np.zeros(np.broadcast_shapes(c.shape[:-1], ax.shape[:-1]), dtype=L.OBB)
    out["centre"], out["ax"], out["ay"], out["az"] = c, ax, ay, az
    return out if out.ndim else out.reshape(1)


def tri_queries_from_mesh(triangles, skip_self=False):
    """layouts.TRI_QUERY records for triangle_intersections / triangle_intersection_segments from another mesh — or the same one:
    `triangles` is an array of layouts.TRIANGLE, or a tuple (a, b, c) of (n, 3) vertex arrays.  skip_self=True sets skip = each
    query's own index (a mesh against itself: a triangle never reports itself; neighbours that share a vertex are the caller's to
    remove from the returned pairs), else layouts.NULL."""
    if isinstance(triangles, np.ndarray) and triangles.dtype == L.TRIANGLE:
        a, b, c = (triangles[k][:, :3] for k in "abc")
    else:
        a, b, c = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in triangles)
    out = np.zeros(len(a), dtype=L.TRI_QUERY)
    out["a"], out["b"], out["c"] = a, b, c
    out["skip"] = np.arange(len(a), dtype=np.uint32) if skip_self else L.NULL
    return out


def tri_casts(a, b, c, direction, t_max=np.inf, skip=None):
    """layouts.TRI_RAY records for triangle_cast / triangle_cast_any: the triangles (a, b, c) (shapes (..., 3), broadcast against
    each other and against `direction`) moving along `direction` for 0 <= t < t_max (+inf: open), with `skip` (ORIGINAL triangle
    indices never reported; None: layouts.NULL), rounded to fp32 once."""
    a, b, c, d = np.broadcast_arrays(*(np.asarray(x, dtype=np.float32) for x in (a, b, c, direction)))
    out = np.zeros(a.shape[:-1], dtype=L.TRI_RAY)
    out["a"], out["b"], out["c"], out["dir"], out["t_max"] = a, b, c, d, t_max
    out["skip"] = L.NULL if skip is None else skip
    return out if out.ndim else out.reshape(1)


def tri_casts_from_mesh(triangles, direction, t_max=np.inf, skip_self=False):
    """layouts.TRI_RAY records that move another mesh — or the same one — along `direction` (one (3,) vector, or one per triangle):
    `triangles` is an array of layouts.TRIANGLE, or a tuple (a, b, c) of (n, 3) vertex arrays.  skip_self=True sets skip = each
    cast's own index (a part of the scene moved against the scene: a triangle never reports itself), else layouts.NULL."""
    if isinstance(triangles, np.ndarray) and triangles.dtype == L.TRIANGLE:
        a, b, c = (triangles[k][:, :3] for k in "abc")
    else:
        a, b, c = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in triangles)
    return tri_casts(a, b, c, direction, t_max, np.arange(len(a), dtype=np.uint32) if skip_self else None)


def triangle_cast_contact(casts, hits, scene_triangles):
    """The contact point and the unit normal of each lbvh_triangle_cast record, in float64 from the fp32 values: `casts`
    layouts.TRI_RAY, `hits` layouts.TRI_CAST_HIT, `scene_triangles` the scene as layouts.TRIANGLE or a tuple (a, b, c) of (n, 3)
    arrays.  -> (points, normals), each (n, 3); NaN rows for a miss record and for a start in overlap (feature & TRI_CAST_START:
    no single point, no normal).
        feature 0 - 2: the moved vertex X + dir * t and the scene face's normal cross(e1, e2)
        feature 3 - 5: the scene vertex and the moving face's normal cross(b - a, c - a)
        feature 6 - 14: the point Q + F * w on the scene edge and cross(E, F) of the two edges
    each normal turned against dir, so that it points from the scene to the moving triangle."""
    if isinstance(scene_triangles, np.ndarray) and scene_triangles.dtype == L.TRIANGLE:
        sa, sb, sc = (scene_triangles[k][:, :3] for k in "abc")
    else:
        sa, sb, sc = scene_triangles
    casts, hits = np.atleast_1d(casts), np.atleast_1d(hits)
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    tri = hits["tri"].astype(np.int64)
    v0, e1, e2 = f8(sa)[tri], f8(sb)[tri] - f8(sa)[tri], f8(sc)[tri] - f8(sa)[tri]
    a, b, c, d = (f8(casts[k]) for k in ("a", "b", "c", "dir"))
    t, w, feature = f8(hits["t"])[:, None], f8(hits["w"])[:, None], hits["feature"].astype(np.int64)
    moving = np.stack([a, b, c], axis=1)                              # [cast, vertex]
    scene = np.stack([v0, v0 + e1, v0 + e2], axis=1)
    rows = np.arange(len(hits))
    m, n = np.clip((feature - 6) // 3, 0, 2), np.clip((feature - 6) % 3, 0, 2)
    edge = (np.roll(moving, -1, axis=1) - moving)[rows, m]            # E_ab, E_bc, E_ca
    q = scene[rows, np.array([0, 0, 1])[n]]
    f = np.stack([e1, e2, e2 - e1], axis=1)[rows, n]
    point = np.where((feature < 3)[:, None], moving[rows, np.clip(feature, 0, 2)] + d * t,
                     np.where((feature < 6)[:, None], scene[rows, np.clip(feature - 3, 0, 2)], q + f * w))
    normal = np.where((feature < 3)[:, None], np.cross(e1, e2), np.where((feature < 6)[:, None], np.cross(b - a, c - a), np.cross(edge, f)))
    with np.errstate(all="ignore"):
        normal = normal / np.linalg.norm(normal, axis=1, keepdims=True)
        normal = np.where(np.sum(normal * d, axis=1, keepdims=True) > 0, -normal, normal)
    none = (hits["t"] >= L.MAX_FLOAT) | (feature >= L.TRI_CAST_START)
    point[none], normal[none] = np.nan, np.nan
    return point, normal


def tri_distance_queries(a, b, c, max_dist2=np.inf, skip=None):
    """layouts.TRI_DISTANCE_QUERY records for triangle_closest_points / triangle_within_distance: the triangles (a, b, c) (shapes
    (..., 3), broadcast against each other) with the given SQUARED search radii (+inf: unbounded) and `skip` (ORIGINAL triangle
    indices never reported; None: layouts.NULL), rounded to fp32 once."""
    a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype=np.float32) for x in (a, b, c)))
    out = np.zeros(a.shape[:-1], dtype=L.TRI_DISTANCE_QUERY)
    out["a"], out["b"], out["c"], out["max_dist2"] = a, b, c, np.asarray(max_dist2, dtype=np.float32)
    out["skip"] = L.NULL if skip is None else np.asarray(skip, dtype=np.uint32)
    return out if out.ndim else out.reshape(1)


def tri_distance_queries_from_mesh(triangles, max_dist2=np.inf, self_skip=False):
    """The same from another mesh — or the same one: `triangles` is an array of layouts.TRIANGLE, or a tuple (a, b, c) of (n, 3)
    vertex arrays.  self_skip=True sets skip = each query's own index (a mesh against itself: a triangle never reports itself;
    neighbours that share a vertex or an edge are at the distance 0 and are the caller's to tell apart), else layouts.NULL."""
    if isinstance(triangles, np.ndarray) and triangles.dtype == L.TRIANGLE:
        a, b, c = (triangles[k][:, :3] for k in "abc")
    else:
        a, b, c = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in triangles)
    return tri_distance_queries(a, b, c, max_dist2, np.arange(len(a), dtype=np.uint32) if self_skip else None)


def tri_closest_witness(queries, scene_triangles, records):
    """The two nearest points that layouts.TRI_CLOSEST `records` name, for the layouts.TRI_DISTANCE_QUERY `queries` they answer and
    the scene's triangles (`scene_triangles`: an array of layouts.TRIANGLE in ORIGINAL order, or a tuple (a, b, c) of (n, 3) vertex
    arrays).  -> (point_on_query, point_on_scene), float64 (count, 3); NaN rows for none-records.  `edge` says which edge holds
    the point P + D*s — an edge of the query (0 .. 2: from a, b, c) or of scene triangle `tri` (3 .. 5: v0-v1, v0-v2, v1-v2) — and
    `delta` leads from the scene's point to the query's: nothing is found again by comparing floats."""
    if isinstance(scene_triangles, np.ndarray) and scene_triangles.dtype == L.TRIANGLE:
        sa, sb, sc = (scene_triangles[k][:, :3] for k in "abc")
    else:
        sa, sb, sc = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in scene_triangles)
    queries, records = np.atleast_1d(queries), np.atleast_1d(records)
    found = records["dist2"] != L.MAX_FLOAT
    tri = np.where(found, records["tri"], 0).astype(np.int64)
    v = [x[tri].astype(np.float64) for x in (sa, sb, sc)]
    q = [queries[k].astype(np.float64) for k in "abc"]
    m = (records["edge"] & 7).astype(np.int64)
    starts = np.stack([q[0], q[1], q[2], v[0], v[0], v[1]])
    ends = np.stack([q[1], q[2], q[0], v[1], v[2], v[2]])
    rows = np.arange(len(records))
    on_edge = starts[m, rows] + (ends[m, rows] - starts[m, rows]) * records["s"].astype(np.float64)[:, None]
    delta = records["delta"].astype(np.float64)
    query_edge = (m < 3)[:, None]
    on_query = np.where(query_edge, on_edge, on_edge + delta)
    on_scene = np.where(query_edge, on_edge - delta, on_edge)
    on_query[~found], on_scene[~found] = np.nan, np.nan
    return on_query, on_scene


def unique_self_pairs(offsets, records, triangles):
    """The pairs of a self-proximity pass (proximity_pairs(mesh, margin, self_skip=True) on the mesh itself: query k IS triangle
    k), each once and without the neighbours: a pair (i, j) = (query, records["tri"]) is kept only for i < j — (j, i) is the same
    pair found from the other side —, and not when the two triangles share a vertex (equal coordinates, word for word: they touch
    by construction and are at the distance 0).  `triangles`: an array of layouts.TRIANGLE in ORIGINAL order, or a tuple (a, b, c)
    of (n, 3) vertex arrays.  -> (pairs, kept): an (m, 2) int64 array of (i, j) and the m layouts.TRI_CLOSEST records, in the
    list's order.  Pure numpy."""
    if isinstance(triangles, np.ndarray) and triangles.dtype == L.TRIANGLE:
        a, b, c = (triangles[k][:, :3] for k in "abc")
    else:
        a, b, c = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in triangles)
    offsets = np.asarray(offsets, dtype=np.uint64)
    records = np.atleast_1d(records)
    i = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets).astype(np.int64))
    j = records["tri"].astype(np.int64)
    verts = np.ascontiguousarray(np.stack([a, b, c], axis=1), dtype=np.float32).view(np.uint32)        # [triangle, vertex, word]
    shared = (verts[i][:, :, None, :] == verts[j][:, None, :, :]).all(axis=3).any(axis=(1, 2))
    keep = (i < j) & ~shared
    return np.stack([i[keep], j[keep]], axis=1), records[keep]


def segment_edges(records):
    """The `edges` word of layouts.TRI_SEGMENT records, unpacked: -> (passed, from_p0, from_p1): passed is a bool array (..., 6),
    passed[..., j] = edge test j passed (j = 0, 1, 2: the query's edges from a, b, c; j = 3, 4, 5: the scene triangle's edges
    v0-v1, v0-v2, v1-v2); from_p0 / from_p1 the test that gave p0 / p1 — an end from j < 3 lies on that edge of the query triangle, one
    from j >= 3 on that edge of scene triangle `tri`, so a cut polyline is stitched by (triangle, edge), not by comparing floats."""
    e = np.asarray(records["edges"] if getattr(records, "dtype", None) == L.TRI_SEGMENT else records, dtype=np.uint32)
    passed = ((e[..., None] >> np.arange(6, dtype=np.uint32)) & 1).astype(bool)
    return passed, ((e >> 8) & 7).astype(np.uint32), ((e >> 12) & 7).astype(np.uint32)


def planes(normals, points):
    """layouts.PLANE records for plane_sections / cross_sections: the planes with the given normals (they need not be unit length)
    through the given points, d = -(n . point) formed in float64 and rounded once.  Either argument may be a single vector: a
    stack of parallel planes is planes(n, points), a fan through one point planes(normals, p)."""
    n = np.atleast_2d(np.asarray(normals, dtype=np.float64))
    p = np.atleast_2d(np.asarray(points, dtype=np.float64))
    n, p = np.broadcast_arrays(n, p)
    out = np.zeros(len(n), dtype=L.PLANE)
    out["n"] = n
    out["d"] = -(out["n"].astype(np.float64) * p).sum(axis=1)
    return out


def section_edges(edges):
    """The `edges` word of layouts.PLANE_SEGMENT records (or the records themselves), unpacked: -> (crossing, from_p0, from_p1,
    sides): crossing is a bool array (..., 3), crossing[..., k] = edge k of the triangle crosses the plane (k = 0, 1, 2: v0-v1,
    v1-v2, v2-v0); from_p0 / from_p1 the edge that gave p0 / p1; sides a bool array (..., 3), the side of v0, v1, v2 (True:
    n . x + d >= 0)."""
    e = np.asarray(edges["edges"] if getattr(edges, "dtype", None) == L.PLANE_SEGMENT else edges, dtype=np.uint32)
    three = np.arange(3, dtype=np.uint32)
    return ((e[..., None] >> three) & 1).astype(bool), ((e >> 8) & 3).astype(np.uint32), ((e >> 12) & 3).astype(np.uint32), \
        ((e[..., None] >> (three + np.uint32(16))) & 1).astype(bool)


def stitch_sections(segments, triangles):
    """Chains the layouts.PLANE_SEGMENT records of ONE plane into polylines: -> (loops, chains), each a list of (points, tris):
    points a float32 array (m, 3), tris the m triangles walked, in order.  A loop is closed (the last record's p1 lies on the edge
    of the first record's p0, the point is not repeated: m points, m records); an open chain starts at a p0 no record leads to and
    has m + 1 points for m records (a mesh with a border, or a record set that is not complete).
    Records are joined by EDGE KEYS made from the ORIGINAL vertex bytes of `triangles` (layouts.TRIANGLE, the scene's own records,
    indexed by `tri`): the key of edge k of a triangle is the sorted pair of the 12-byte positions of its two vertices, so two
    triangles agree on a shared edge exactly when the mesh stores the same vertex bytes in both.  No computed float is compared.
    On a consistently wound mesh the p1-edge of a record is the p0-edge of its neighbour, so every chain runs one way round."""
    segments = np.asarray(segments)
    _, from_p0, from_p1, _ = section_edges(segments)
    tri = segments["tri"].astype(np.int64)
    verts = [np.ascontiguousarray(triangles[k][tri][:, :3], dtype=np.float32) for k in "abc"]
    raw = [[v[i].tobytes() for i in range(len(tri))] for v in verts]

    def key(i, k):
        u, v = raw[k][i], raw[(k + 1) % 3][i]
        return (u, v) if u <= v else (v, u)

    starts = {}
    for i in range(len(tri)):
        starts.setdefault(key(i, int(from_p0[i])), []).append(i)
    used = np.zeros(len(tri), dtype=bool)

    def follow(first):
        order, i = [], first
        while True:
            used[i] = True
            order.append(i)
            nxt = [j for j in starts.get(key(i, int(from_p1[i])), ()) if not used[j]]
            if not nxt:
                return order, key(i, int(from_p1[i])) == key(first, int(from_p0[first]))
            i = nxt[0]

    ends = {}
    for i in range(len(tri)):
        ends[key(i, int(from_p1[i]))] = ends.get(key(i, int(from_p1[i])), 0) + 1
    loops, chains = [], []
    # open chains first, from the records no other record leads to; what is left are loops
    for i in range(len(tri)):
        if not used[i] and key(i, int(from_p0[i])) not in ends:
            order, _ = follow(i)
            chains.append((np.concatenate([segments["p0"][order], segments["p1"][order[-1:]]]), segments["tri"][order].copy()))
    for i in range(len(tri)):
        if not used[i]:
            order, closed = follow(i)
            if closed:
                loops.append((segments["p0"][order].copy(), segments["tri"][order].copy()))
            else:
                chains.append((np.concatenate([segments["p0"][order], segments["p1"][order[-1:]]]), segments["tri"][order].copy()))
    return loops, chains


class _DeviceWords:
    """`count` 32-bit floats at a device pointer, for torch.as_tensor (zero copy)"""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2, "strides": None}


def push_out(drawer, shapes, skin, iterations=4):
    """What capsule_deepest is for, as a convenience: up to `iterations` times, ask for the deepest contact of every capsule of the
    DataBuffer `shapes` (layouts.CAPSULE) and move every capsule with depth > 0 by normal * (depth + skin), in place on the device
    (torch); stop when no depth is > 0.  Returns (shapes, depths): the same DataBuffer and the float32 host array of the depths
    that capsule_deepest reports for the final positions (0 for a capsule that touches nothing).  One contact is resolved per
    iteration and capsule: a corner of k planes needs about k iterations.  Waits on the host in every iteration; not part of
    the word-for-word contract of include/lbvh.h.
    A DataBuffer of layouts.OBB is taken the same way through obb_deepest: the centre (words 0 .. 2 of each 16-word record) moves,
    the half-axis vectors stay.  A box that merely touches has depth 0 and is left where it is."""
    import torch
    if shapes.dtype not in (L.CAPSULE, L.OBB):
        raise ValueError("shapes must be a DataBuffer of layouts.CAPSULE or layouts.OBB")
    box = shapes.dtype == L.OBB
    stride = 16 if box else 8
    if not torch.cuda.is_available():
        # (a torch that brings a HIP runtime of its own sees the GPU only if it was imported before this package loaded the library)
        raise RuntimeError("push_out needs torch on the GPU: import torch before unitysimpleraytracing_amd")
    ctx, n = drawer.ctx, shapes.size
    dev = torch.device("cuda", ctx.device_id)
    out = DataBuffer(ctx, n, L.BOX_CONTACT if box else L.CONTACT)
    try:
        caps = torch.as_tensor(_DeviceWords(shapes.device.value, n * stride), device=dev).view(n, stride)
        recs = torch.as_tensor(_DeviceWords(out.device.value, n * 8), device=dev).view(n, 8)
        for it in range(int(iterations) + 1):
            (drawer.obb_deepest if box else drawer.capsule_deepest)(shapes, out)
            ctx.sync()                                              # the library's stream is not torch's
            deep = recs[:, 0] > 0
            if it == int(iterations) or not bool(deep.any()):
                break
            caps[:, 0:3] += torch.where(deep[:, None], recs[:, 4:7] * (recs[:, 0:1] + float(skin)), torch.zeros_like(recs[:, 4:7]))
            torch.cuda.synchronize(dev)
        shapes._synced = False
        return shapes, out.get_data()["depth"].copy()
    finally:
        out.dispose()


def box_cast_axis(cast, triangle_line, axis):
    """L_j of include/lbvh.h (lbvh_box_cast) for j = axis < 13, in float64 from the fp32 values: `cast` one layouts.BOX_RAY record,
    `triangle_line` = (a, e1, e2) of the reported triangle (e1 = b - a, e2 = c - a)."""
    _, e1, e2 = (np.asarray(x, dtype=np.float64) for x in triangle_line)
    b = [np.asarray(cast[k], dtype=np.float64) for k in ("ax", "ay", "az")]
    if axis == 0:
        return np.cross(e1, e2)
    if axis < 4:
        return np.cross(b[axis % 3], b[(axis + 1) % 3])
    return np.cross(b[(axis - 4) // 3], (e1, e2, e2 - e1)[(axis - 4) % 3])


def box_cast_normal(cast, triangle_line, axis):
    """The contact normal of a lbvh_box_cast record, pointing from the triangle to the box: -sign(v) * L / |L| with L the record's
    separating axis and v = dot(dir, L).  None for axis = layouts.BOX_AXIS_START (overlapping at the start: no normal).  The miss
    record has axis = 0 like a contact with the face: test t < layouts.MAX_FLOAT before asking for a normal.  A contact point is not
    defined by the record (a box touches a triangle in a point, a segment or a polygon)."""
    if axis >= L.BOX_AXIS_START:
        return None
    line = box_cast_axis(cast, triangle_line, axis)
    v = float(np.dot(np.asarray(cast["dir"], dtype=np.float64), line))
    return -np.sign(v) * line / np.linalg.norm(line)


def frustum_planes(camera, far, rect=None):
    """The view frustum of `camera` (the dict of scenes.camera or an N.Camera) as one layouts.REGION record, in the convention of
    lbvh_trace_primary's ray generation: the eye at camera_to_world * (0, 0, 0, 1), looking along the camera's -z; the image plane at
    depth near_plane is 2 * near_plane * camera_fov high (camera_fov is the tangent of half the vertical angle) and screen_width /
    screen_height times as wide.  Planes: left, right, bottom, top (through the eye), near (depth >= near_plane), far (depth <= far);
    depth is measured along the view axis.  rect = (x0, y0, x1, y1) in pixels narrows the four side planes to that part of the
    image (a tile or cluster frustum)."""
    if isinstance(camera, N.Camera):
        camera = {k: getattr(camera, k) for k in ("screen_width", "screen_height", "camera_fov", "near_plane")} | \
            {"camera_to_world": np.array(camera.camera_to_world[:], dtype=np.float32)}
    sw, sh = float(camera["screen_width"]), float(camera["screen_height"])
    t = float(np.float32(camera["camera_fov"]))
    near = float(np.float32(camera["near_plane"]))
    m = np.asarray(camera["camera_to_world"], dtype=np.float32).astype(np.float64).reshape(4, 4)
    x0, y0, x1, y1 = rect if rect is not None else (0.0, 0.0, sw, sh)
    ta = t * sw / sh
    # the slopes x / depth and y / depth of the rect's edges: pixel x maps to (-1 + 2 x / sw) * ta, pixel y to (-1 + 2 y / sh) * t
    xl, xr = (-1.0 + 2.0 * x0 / sw) * ta, (-1.0 + 2.0 * x1 / sw) * ta
    yb, yt = (-1.0 + 2.0 * y0 / sh) * t, (-1.0 + 2.0 * y1 / sh) * t
    cam = np.array([[1.0, 0.0, xl, 0.0],         # x_c - xl * depth >= 0, depth = -z_c
                    [-1.0, 0.0, -xr, 0.0],       # xr * depth - x_c >= 0
                    [0.0, 1.0, yb, 0.0],
                    [0.0, -1.0, -yt, 0.0],
                    [0.0, 0.0, -1.0, -near],     # depth - near >= 0
                    [0.0, 0.0, 1.0, float(far)]])  # far - depth >= 0
    return _regions(cam @ np.linalg.inv(m))      # a plane is a row vector: (n, d) . x_c = (n, d) . M^-1 . x_w


class Context:
    """One GPU + one HIP stream.  Stands in for the implicit Unity graphics device and the
    IShaderContainer kernel registry (Assets/_Scripts/ShaderContainer.cs:6-40)."""

    def __init__(self, device_id=0, stream=None):
        h = C.c_void_p()
        if stream is None:
            N.check(None, N.lib.lbvh_create(device_id, C.byref(h)))
        else:
            N.check(None, N.lib.lbvh_create_on_stream(device_id, C.c_void_p(stream), C.byref(h)))
        self.handle = h
        self.device_id = device_id

    def sync(self):
        N.check(self.handle, N.lib.lbvh_sync(self.handle))

    def close(self):
        if self.handle:
            N.lib.lbvh_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- measurement helpers ------------------------------------------------------------------
    def event(self):
        e = C.c_void_p()
        N.check(self.handle, N.lib.lbvh_event_create(self.handle, C.byref(e)))
        return e

    def record(self, ev):
        N.check(self.handle, N.lib.lbvh_event_record(self.handle, ev))

    def elapsed_ms(self, start, stop):
        ms = C.c_float()
        N.check(self.handle, N.lib.lbvh_event_elapsed_ms(self.handle, start, stop, C.byref(ms)))
        return ms.value

    def destroy_event(self, ev):
        N.lib.lbvh_event_destroy(self.handle, ev)

    def profile_begin(self):
        N.check(self.handle, N.lib.lbvh_profile_begin(self.handle))

    def profile_end(self):
        """{kernel name: (launches, total device ms)} since profile_begin."""
        rows = (N.ProfileRow * 64)()
        n = C.c_int32()
        N.check(self.handle, N.lib.lbvh_profile_end(self.handle, rows, 64, C.byref(n)))
        return {rows[i].name.decode(): (int(rows[i].launches), float(rows[i].total_ms)) for i in range(n.value)}

    def clock_probe(self):
        """shader clock held under a vector-ALU-bound load, MHz (lbvh_clock_probe)"""
        mhz = C.c_float()
        N.check(self.handle, N.lib.lbvh_clock_probe(self.handle, C.byref(mhz)))
        return mhz.value

    def trace_forget(self):
        """drop the traversal's dispatch history: the next LBVH_TRACE_FAST frame is a cold one"""
        N.check(self.handle, N.lib.lbvh_trace_forget(self.handle))

    def trace_costs_export(self, frame_costs, tiles_x, tiles_y):
        """this context's per-tile step counts of its last LBVH_TRACE_FAST trace into a full-frame DataBuffer (u32 per tile)"""
        N.check(self.handle, N.lib.lbvh_trace_costs_export(self.handle, frame_costs.device, tiles_x, tiles_y))

    def trace_costs_import(self, frame_costs, tiles_x, tiles_y):
        """the merged per-tile step counts of every rank's last trace: the next moved-camera frame's dispatch hint"""
        N.check(self.handle, N.lib.lbvh_trace_costs_import(self.handle, frame_costs.device, tiles_x, tiles_y))

    def copy_probe(self, dst, src, nbytes):
        N.check(self.handle, N.lib.lbvh_copy_bandwidth_probe(self.handle, dst, src, nbytes))

    # -- one frame from N GPUs (include/lbvh.h, "one frame from N GPUs") ---------------------------------
    def peer_enable(self, peer_device):
        """kernels of this context may store into memory of `peer_device` (the frame's owner)"""
        N.check(self.handle, N.lib.lbvh_peer_enable(self.handle, int(peer_device)))

    def sync_event(self):
        """an ORDERING event (system-scope release at its record), for wait_event of another context"""
        e = C.c_void_p()
        N.check(self.handle, N.lib.lbvh_sync_event_create(self.handle, C.byref(e)))
        return e

    def wait_event(self, ev):
        """this context's stream waits on the device for an event recorded on any context of the process"""
        N.check(self.handle, N.lib.lbvh_event_wait(self.handle, ev))

    def ipc_export(self, device_ptr):
        """64-byte cross-process handle of a buffer of this context (hipIpcGetMemHandle)"""
        h = (C.c_uint8 * 64)()
        N.check(self.handle, N.lib.lbvh_ipc_export(self.handle, device_ptr, h))
        return bytes(h)

    def ipc_import(self, handle_bytes):
        """the exporting process's buffer mapped here: a device pointer usable on this context"""
        h = (C.c_uint8 * 64).from_buffer_copy(handle_bytes)
        p = C.c_void_p()
        N.check(self.handle, N.lib.lbvh_ipc_import(self.handle, h, C.byref(p)))
        return p

    def ipc_close(self, device_ptr):
        N.check(self.handle, N.lib.lbvh_ipc_close(self.handle, device_ptr))

    def flags_alloc(self, n_words):
        """n_words zeroed completion flags a running kernel may poll while another GPU / process stores into them (uncached
        device memory, lbvh_flags_alloc); free with flags_free"""
        p = C.c_void_p()
        N.check(self.handle, N.lib.lbvh_flags_alloc(self.handle, int(n_words), C.byref(p)))
        return p

    def flags_free(self, flags_ptr):
        N.check(self.handle, N.lib.lbvh_buffer_free(self.handle, flags_ptr))

    def debug_switch(self, which, value):
        """include/lbvh_debug.h: test / measurement switches of this context (all 0 in the product)"""
        N.check(self.handle, N.lib.lbvh_debug_switch(self.handle, int(which), int(value)))

    def frame_signal(self, flags_ptr, slot, value):
        """flags[slot] := value (system-scope release) once everything enqueued so far has finished"""
        N.check(self.handle, N.lib.lbvh_frame_signal(self.handle, flags_ptr, slot, value))

    def frame_wait(self, flags_ptr, n_slots, value):
        """later work on this context starts only when flags[0..n_slots) have all reached `value` (bounded device-side wait)"""
        N.check(self.handle, N.lib.lbvh_frame_wait(self.handle, flags_ptr, n_slots, value))


class DataBuffer:
    """Assets/_Scripts/DataBuffer.cs: a device buffer (ComputeBuffer) + a host mirror (T[])."""

    def __init__(self, ctx, size, dtype, initial_value=None):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.size = int(size)
        self.local = np.zeros(self.size, dtype=self.dtype)          # _localBuffer
        p = C.c_void_p()
        N.check(ctx.handle, N.lib.lbvh_buffer_alloc(ctx.handle, self.size, self.dtype.itemsize, C.byref(p)))
        self.device = p                                             # _deviceBuffer
        self._synced = False
        if initial_value is not None:                               # DataBuffer(size, initialValue) :14-23
            self.fill_u32(initial_value)

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    def fill_u32(self, word, mirror=True):
        """Every 32-bit word of the buffer = `word` (0xFFFFFFFF = NullLeaf / uint.MaxValue).
        mirror=False leaves the host copy alone (per-frame rebuilds)."""
        N.check(self.ctx.handle, N.lib.lbvh_buffer_fill_u32(self.ctx.handle, self.device, word, self.nbytes // 4))
        if mirror:
            self.local.view(np.uint32)[:] = word
        self._synced = mirror

    def get_data(self):                                             # GetData :50-54 (blocking)
        N.check(self.ctx.handle, N.lib.lbvh_buffer_download(
            self.ctx.handle, self.local.ctypes.data_as(C.c_void_p), self.device, self.nbytes))
        self._synced = True
        return self.local

    def sync(self):                                                 # Sync() = SetData :56-60
        N.check(self.ctx.handle, N.lib.lbvh_buffer_upload(
            self.ctx.handle, self.device, self.local.ctypes.data_as(C.c_void_p), self.nbytes))
        self._synced = True

    def dispose(self):                                              # Dispose :72-75
        if self.device:
            N.lib.lbvh_buffer_free(self.ctx.handle, self.device)
            self.device = None


def sort_hit_segments(ctx, offsets, hits, count=None):
    """Every segment of a gathered list into (t, tri) order, in place, on the device (lbvh_sort_hit_segments): `offsets` the uint64
    DataBuffer a gather wrote (count + 1 entries; count defaults to offsets.size - 1), `hits` the layouts.HIT DataBuffer given to
    that gather — its size is the capacity; a segment that did not fit is left as it is.  Needs no scene.  Asynchronous.
    The layouts.BOX_HIT records of box_cast_all and the layouts.TRI_CAST_HIT records of triangle_cast_all are taken too: t and tri
    are in the same words, axis — or feature and w — travel with their record."""
    _sort_segments(N.lib.lbvh_sort_hit_segments, ctx, offsets, hits, hits.dtype if hits.dtype in (L.BOX_HIT, L.TRI_CAST_HIT) else L.HIT, count)


def sort_index_segments(ctx, offsets, tris, count=None):
    """The same for the uint32 DataBuffer `tris` of box_overlaps / gather_within_distance (lbvh_sort_index_segments): every
    segment ascending."""
    _sort_segments(N.lib.lbvh_sort_index_segments, ctx, offsets, tris, np.dtype(np.uint32), count)


def _record_orders():
    return {L.TRI_CLOSEST: N.SORT_RECORDS_ASCENDING, L.CONTACT: N.SORT_RECORDS_DESCENDING, L.BOX_CONTACT: N.SORT_RECORDS_DESCENDING,
            L.TRI_SEGMENT: N.SORT_RECORDS_BY_TRI, L.PLANE_SEGMENT: N.SORT_RECORDS_BY_TRI}


def sort_record_segments(ctx, offsets, records, order=None, count=None):
    """The same for a DataBuffer of 32-byte records (lbvh_sort_record_segments): layouts.TRI_CLOSEST, CONTACT, BOX_CONTACT,
    TRI_SEGMENT or PLANE_SEGMENT; its size is the capacity.  `order`: _native.SORT_RECORDS_ASCENDING — (word 0 as an fp32 value,
    word 1) —, SORT_RECORDS_DESCENDING — the greatest word 0 first, the lower word 1 on ties, NaNs last — or SORT_RECORDS_BY_TRI —
    word 3.  None chooses by the dtype: TRI_CLOSEST ascending (nearest first), CONTACT and BOX_CONTACT descending (deepest first),
    TRI_SEGMENT and PLANE_SEGMENT by tri.  Needs no scene.  Asynchronous."""
    orders = _record_orders()
    if records.dtype not in orders:
        raise ValueError("records must be a DataBuffer of layouts.TRI_CLOSEST, CONTACT, BOX_CONTACT, TRI_SEGMENT or PLANE_SEGMENT")
    order = orders[records.dtype] if order is None else int(order)
    if order not in (N.SORT_RECORDS_ASCENDING, N.SORT_RECORDS_DESCENDING, N.SORT_RECORDS_BY_TRI):
        raise ValueError("order must be one of _native.SORT_RECORDS_ASCENDING, SORT_RECORDS_DESCENDING, SORT_RECORDS_BY_TRI")
    _sort_segments(lambda h, o, n, d, cap: N.lib.lbvh_sort_record_segments(h, o, n, d, cap, order), ctx, offsets, records, records.dtype, count)


def _sort_records_by_dtype(ctx, offsets, records, count):
    """_csr_lists' segment_sort hook: sort_record_segments in the order the dtype names"""
    sort_record_segments(ctx, offsets, records, None, count)


def _sort_segments(fn, ctx, offsets, data, dtype, count):
    count = offsets.size - 1 if count is None else int(count)
    if offsets.dtype != np.uint64 or data.dtype != dtype or count < 0 or offsets.size < count + 1:
        raise ValueError(f"offsets must be a DataBuffer of uint64 with count + 1 entries and the data one of {dtype}")
    N.check(ctx.handle, fn(ctx.handle, offsets.device, count, data.device, data.size))


class MeshBufferContainer:
    """Assets/_Scripts/MeshBufferContainer.cs.  The constructor takes the triangle soup (the
    reference's Mesh -> Triangle[] conversion, :117-146, stays on the caller's side) and runs the
    per-triangle Morton/AABB loop on the GPU instead of the CPU."""

    def __init__(self, ctx, triangles, capacity=None, box_min=L.SCENE_BOX_MIN, box_max=L.SCENE_BOX_MAX):
        triangles = np.ascontiguousarray(triangles, dtype=L.TRIANGLE)
        n = len(triangles)
        self.ctx = ctx
        self.triangles_length = n                                    # _trianglesLength
        self.capacity = capacity_for(n) if capacity is None else int(capacity)
        cap = self.capacity
        self.keys = DataBuffer(ctx, cap, np.uint32)                  # :108 (filled by morton_aabb)
        self.triangle_index = DataBuffer(ctx, cap, np.uint32)        # :109
        self.triangle_data = DataBuffer(ctx, cap, L.TRIANGLE)        # :110
        self.triangle_aabb = DataBuffer(ctx, cap, L.AABB)            # :111
        self.bvh_data = DataBuffer(ctx, cap, L.AABB)                 # :113
        self.bvh_leaf_node = DataBuffer(ctx, cap, L.LEAF_NODE, L.NULL)        # :114
        self.bvh_internal_node = DataBuffer(ctx, cap, L.INTERNAL_NODE, L.NULL)  # :115
        self.triangle_data.local[:n] = triangles
        self.triangle_data.sync()                                    # :150
        self.box_min = np.ascontiguousarray(box_min, dtype=np.float32)
        self.box_max = np.ascontiguousarray(box_max, dtype=np.float32)
        self.generate_keys()

    def generate_keys(self):
        """The loop of :123-146 + the Sync()s of :148-151 as one kernel."""
        f3 = C.POINTER(C.c_float)
        N.check(self.ctx.handle, N.lib.lbvh_morton_aabb(
            self.ctx.handle, self.triangle_data.device, self.triangles_length, self.capacity,
            self.box_min.ctypes.data_as(f3), self.box_max.ctypes.data_as(f3),
            self.keys.device, self.triangle_index.device, self.triangle_aabb.device))

    def distribute_keys(self):                                       # DistributeKeys :154-169
        N.check(self.ctx.handle, N.lib.lbvh_distribute_keys(self.ctx.handle, self.keys.device, self.triangles_length))

    def get_all_gpu_data(self):                                      # GetAllGpuData :171-196
        for b in (self.keys, self.triangle_index, self.triangle_data, self.triangle_aabb,
                  self.bvh_data, self.bvh_leaf_node, self.bvh_internal_node):
            b.get_data()
        n = self.triangles_length
        leaf, inner = self.bvh_leaf_node.local, self.bvh_internal_node.local
        bad_leaf = np.nonzero((leaf["index"][:n] == L.NULL) & (leaf["parent"][:n] == L.NULL))[0]
        bad_inner = np.nonzero((inner["index"][:n - 1] == L.NULL) & (inner["parent"][:n - 1] == L.NULL))[0]
        return bad_leaf, bad_inner                                   # "LEAF/INTERNAL CORRUPTED" :181-195

    def scene(self):
        s = N.Scene()
        s.n = self.triangles_length
        s.sorted_indices = self.triangle_index.device.value
        s.triangle_aabb = self.triangle_aabb.device.value
        s.internal_nodes = self.bvh_internal_node.device.value
        s.leaf_nodes = self.bvh_leaf_node.device.value
        s.bvh = self.bvh_data.device.value
        s.triangles = self.triangle_data.device.value
        return s

    def dispose(self):                                               # Dispose :207-216
        for b in (self.keys, self.triangle_index, self.triangle_data, self.triangle_aabb,
                  self.bvh_data, self.bvh_leaf_node, self.bvh_internal_node):
            b.dispose()


class ComputeBufferSorter:
    """Assets/_Scripts/ComputeBufferSorter.cs.  As in the reference, `data_length` (the triangle
    count, RaytracingMeshDrawer.cs:36) only bounds the sortedness validation (:150-177); Sort()
    always sorts the whole padded buffers (every dispatch covers DATA_ARRAY_COUNT, :107,116)."""

    def __init__(self, ctx, data_length, keys, values):
        self.ctx, self.data_length, self.keys, self.values = ctx, int(data_length), keys, values

    def sort(self):                                                  # Sort() :100-126
        N.check(self.ctx.handle, N.lib.lbvh_sort_pairs(
            self.ctx.handle, self.keys.device, self.values.device, self.keys.size))

    def validate_sorted_data(self):                                  # ValidateSortedData :150-177
        k = self.keys.get_data()[: self.data_length]
        return bool(np.all(k[1:] >= k[:-1])), int(np.count_nonzero(k[1:] == k[:-1]))

    def dispose(self):                                               # scratch lives in the context
        pass


class BVHConstructor:
    """Assets/_Scripts/BVHConstructor.cs."""

    def __init__(self, ctx, triangles_count, sorted_morton_codes, sorted_triangle_indices, triangle_aabb,
                 internal_nodes, leaf_nodes, bvh_data):
        self.ctx = ctx
        self.n = int(triangles_count)
        self.keys, self.indices, self.triangle_aabb = sorted_morton_codes, sorted_triangle_indices, triangle_aabb
        self.internal, self.leaf, self.bvh = internal_nodes, leaf_nodes, bvh_data

    def construct_tree(self):                                        # ConstructTree :61-64
        N.check(self.ctx.handle, N.lib.lbvh_build_tree(
            self.ctx.handle, self.n, self.keys.device, self.internal.device, self.leaf.device))

    def construct_bvh(self):                                         # ConstructBVH :66-69
        N.check(self.ctx.handle, N.lib.lbvh_refit(
            self.ctx.handle, self.n, self.internal.device, self.leaf.device, self.triangle_aabb.device,
            self.indices.device, self.bvh.device))

    def dispose(self):
        pass


class RaytracingMeshDrawer:
    """Assets/_Scripts/RaytracingMeshDrawer.cs: awake() = the build chain of Awake() :30-51,
    update() = the per-frame dispatch of Update() :76-84 (hit records instead of shaded pixels)."""

    def __init__(self, ctx, triangles, capacity=None):
        self.ctx = ctx
        self._triangles = triangles
        self._capacity = capacity
        self.container = None
        self._hits = None
        self._stats = None

    def awake(self, fast=True):
        ctx = self.ctx
        self.container = c = MeshBufferContainer(ctx, self._triangles, self._capacity)           # :34
        self.sorter = ComputeBufferSorter(ctx, c.triangles_length, c.keys, c.triangle_index)     # :36
        self.sorter.sort()                                                                       # :37
        c.distribute_keys()                                                                      # :39
        self.bvh_constructor = BVHConstructor(ctx, c.triangles_length, c.keys, c.triangle_index,
                                              c.triangle_aabb, c.bvh_internal_node, c.bvh_leaf_node,
                                              c.bvh_data)                                        # :41-48
        self.bvh_constructor.construct_tree()                                                    # :50
        self.bvh_constructor.construct_bvh()                                                     # :51
        if fast:
            self.build_fast_scene()
        return self

    def rebuild(self, fast=True, staged=False):
        """Per-frame rebuild on the same buffers (dynamic scenes): Morton -> ... -> refit (+ the derived traversal
        scene).  One lbvh_build_scene call (the two chains after the sort run concurrently); staged=True issues
        the reference's stage calls one by one instead — same results."""
        c = self.container
        if staged:
            c.bvh_leaf_node.fill_u32(L.NULL, mirror=False)
            c.bvh_internal_node.fill_u32(L.NULL, mirror=False)
            c.generate_keys()
            self.sorter.sort()
            c.distribute_keys()
            self.bvh_constructor.construct_tree()
            self.bvh_constructor.construct_bvh()
            if fast:
                self.build_fast_scene()
            return
        f3 = C.POINTER(C.c_float)
        N.check(self.ctx.handle, N.lib.lbvh_build_scene(
            self.ctx.handle, c.triangle_data.device, c.triangles_length, c.capacity, c.box_min.ctypes.data_as(f3),
            c.box_max.ctypes.data_as(f3), c.keys.device, c.triangle_index.device, c.triangle_aabb.device,
            c.bvh_internal_node.device, c.bvh_leaf_node.device, c.bvh_data.device,
            L.BUILD_RESET_NODES | (L.BUILD_FAST_SCENE if fast else 0)))

    def build_fast_scene(self):
        c = self.container
        s = c.scene()
        f3 = C.POINTER(C.c_float)
        N.check(self.ctx.handle, N.lib.lbvh_build_fast_scene(self.ctx.handle, C.byref(s), c.box_min.ctypes.data_as(f3),
                                                             c.box_max.ctypes.data_as(f3)))

    def trace_closest(self, rays, hits):
        """Closest hit of each ray of the DataBuffer `rays` (layouts.RAY: origin, t_min, dir, t_max) into the DataBuffer `hits`
        (layouts.HIT), over the derived scene (awake(fast=True) / rebuild(fast=True)).  Asynchronous; read with hits.get_data()."""
        self._per_query(N.lib.lbvh_trace_closest, rays, "RAY", hits, L.HIT, "rays")

    def trace_occluded(self, rays, flags):
        """1 into the uint32 DataBuffer `flags` for each ray of `rays` that meets anything in (t_min, t_max), else 0."""
        self._per_query(N.lib.lbvh_trace_occluded, rays, "RAY", flags, np.uint32, "rays")

    def _per_query(self, fn, queries, layout, out, dtype, noun, out_noun="the output"):
        """One record or flag per query: fn(ctx, queries, count, scene, out) on a DataBuffer of layouts.<layout> (`noun` in the
        message) and one of `dtype` that holds as many entries."""
        if queries.dtype != getattr(L, layout) or out.dtype != dtype or out.size < queries.size:
            raise ValueError(f"{noun} must be a DataBuffer of layouts.{layout} and {out_noun} one of {np.dtype(dtype)} with at least as many entries")
        s = self.container.scene()
        N.check(self.ctx.handle, fn(self.ctx.handle, queries.device, queries.size, C.byref(s), out.device))

    def sphere_cast(self, casts, hits):
        """First contact of each moving sphere of the DataBuffer `casts` (layouts.SPHERE_RAY: origin, radius, dir, t_max) with the
        mesh into the DataBuffer `hits` (layouts.HIT: t, tri, and the barycentrics u, v of the contact point), over the derived
        scene.  The centre is at origin + dir * t; no contact in [0, t_max): the miss record.  Asynchronous; read with
        hits.get_data()."""
        self._per_query(N.lib.lbvh_sphere_cast, casts, "SPHERE_RAY", hits, L.HIT, "casts")

    def sphere_cast_any(self, casts, flags):
        """1 into the uint32 DataBuffer `flags` for each sphere of `casts` that touches anything on its way, else 0."""
        self._per_query(N.lib.lbvh_sphere_cast_any, casts, "SPHERE_RAY", flags, np.uint32, "casts")

    def capsule_cast(self, casts, hits):
        """First contact of each moving capsule of the DataBuffer `casts` (layouts.CAPSULE_RAY: origin, radius, dir, t_max, axis —
        the axis is the segment from origin to origin + axis, every point within `radius` of it the capsule) with the mesh into the
        DataBuffer `hits` (layouts.HIT: t, tri, and the barycentrics u, v of the contact point on the triangle), over the derived
        scene.  The axis starts at origin + dir * t; no contact in [0, t_max): the miss record.  Asynchronous; read with
        hits.get_data()."""
        self._per_query(N.lib.lbvh_capsule_cast, casts, "CAPSULE_RAY", hits, L.HIT, "casts")

    def capsule_cast_any(self, casts, flags):
        """1 into the uint32 DataBuffer `flags` for each capsule of `casts` that touches anything on its way, else 0."""
        self._per_query(N.lib.lbvh_capsule_cast_any, casts, "CAPSULE_RAY", flags, np.uint32, "casts")

    def box_cast(self, casts, hits):
        """First contact of each moving box of the DataBuffer `casts` (layouts.BOX_RAY: centre, t_max, dir and the half-axis vectors
        ax, ay, az, as obb_half_axes makes them) with the mesh into the DataBuffer `hits` (layouts.BOX_HIT: t, tri, and the
        separating axis that gave the time — box_cast_normal turns it into the contact normal), over the derived scene.  The centre
        is at centre + dir * t; no contact in [0, t_max): the miss record.  Asynchronous; read with hits.get_data()."""
        self._per_query(N.lib.lbvh_box_cast, casts, "BOX_RAY", hits, L.BOX_HIT, "casts")

    def box_cast_any(self, casts, flags):
        """1 into the uint32 DataBuffer `flags` for each box of `casts` that touches anything on its way, else 0."""
        self._per_query(N.lib.lbvh_box_cast_any, casts, "BOX_RAY", flags, np.uint32, "casts")

    def triangle_cast(self, casts, hits):
        """First contact of each moving triangle of the DataBuffer `casts` (layouts.TRI_RAY: a, skip, b, t_max, c, dir, as tri_casts
        makes them) with the mesh into the DataBuffer `hits` (layouts.TRI_CAST_HIT: t, tri, the feature pair that gave the time and
        w, the position on the scene edge for an edge against an edge — triangle_cast_contact turns a record into the contact
        point and normal), over the derived scene.  The triangle is at a + dir * t, b + dir * t, c + dir * t; no contact in
        [0, t_max): the miss record.  Asynchronous; read with hits.get_data()."""
        self._per_query(N.lib.lbvh_triangle_cast, casts, "TRI_RAY", hits, L.TRI_CAST_HIT, "casts")

    def triangle_cast_any(self, casts, flags):
        """1 into the uint32 DataBuffer `flags` for each triangle of `casts` that touches anything on its way, else 0."""
        self._per_query(N.lib.lbvh_triangle_cast_any, casts, "TRI_RAY", flags, np.uint32, "casts")

    def mesh_sweep(self, other_triangles, direction, t_max=np.inf):
        """Convenience: how far the whole mesh `other_triangles` (layouts.TRIANGLE, or a tuple (a, b, c) of (n, 3) arrays) may
        move along `direction` before it touches this mesh: one triangle_cast per triangle and the least record over them, by
        (t, the moving triangle's index).  Returns (record, index): the layouts.TRI_CAST_HIT record and the index of the moving
        triangle that gave it; (the miss record, -1) if nothing touches for 0 <= t < t_max.  Blocking."""
        casts = tri_casts_from_mesh(other_triangles, direction, t_max)
        buf, hits = DataBuffer(self.ctx, len(casts), L.TRI_RAY), DataBuffer(self.ctx, len(casts), L.TRI_CAST_HIT)
        try:
            buf.local[:] = casts
            buf.sync()
            self.triangle_cast(buf, hits)
            got = hits.get_data().copy()
        finally:
            buf.dispose()
            hits.dispose()
        k = int(np.argmin(got["t"]))                                   # the first least t; a miss record has LBVH_MAX_FLOAT
        return (got[k], k) if got["t"][k] < L.MAX_FLOAT else (got[k], -1)

    def closest_points(self, queries, out):
        """Nearest triangle of each point of the DataBuffer `queries` (layouts.POINT_QUERY: p, max_dist2) into the DataBuffer `out`
        (layouts.CLOSEST_POINT: dist2, tri, u, v), over the derived scene.  Asynchronous; read with out.get_data()."""
        self._per_query(N.lib.lbvh_closest_point_query, queries, "POINT_QUERY", out, L.CLOSEST_POINT, "queries")

    def within_distance(self, queries, flags):
        """1 into the uint32 DataBuffer `flags` for each point of `queries` with a triangle nearer than sqrt(max_dist2), else 0."""
        self._per_query(N.lib.lbvh_within_distance, queries, "POINT_QUERY", flags, np.uint32, "queries")

    def k_closest_points(self, queries, k, out, found=None):
        """The k nearest triangles (1 <= k <= 32) of each point of `queries` (layouts.POINT_QUERY) into the DataBuffer `out`
        (layouts.CLOSEST_POINT, at least queries.size * k entries): row q = out[q * k : (q + 1) * k], nearest first, ties by the
        lower triangle index, padded with none-records {MAX_FLOAT, 0, 0, 0}.  `found` (uint32 DataBuffer, optional) receives the
        number of real records per row.  Asynchronous; read with out.get_data()[: queries.size * k].reshape(-1, k)."""
        k = int(k)
        if queries.dtype != L.POINT_QUERY or out.dtype != L.CLOSEST_POINT or out.size < queries.size * k or \
                (found is not None and (found.dtype != np.uint32 or found.size < queries.size)):
            raise ValueError("queries must be a DataBuffer of layouts.POINT_QUERY, out one of layouts.CLOSEST_POINT with k entries "
                             "per query, found one of uint32 with at least as many entries as queries, or None")
        if not 1 <= k <= N.K_CLOSEST_MAX:
            raise ValueError(f"k must be 1 .. {N.K_CLOSEST_MAX}")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_k_closest_points(self.ctx.handle, queries.device, queries.size, k, C.byref(s), out.device,
                                                             found.device if found is not None else None))

    def box_overlaps(self, boxes, offsets, tris=None):
        """Every triangle whose own box touches each box of the DataBuffer `boxes` (layouts.AABB), as a CSR list on the caller's
        buffers: `offsets` (uint64 DataBuffer, at least boxes.size + 1 entries) always complete; `tris` (uint32 DataBuffer, its size
        is the capacity) receives the ORIGINAL triangle indices, segment k = tris[offsets[k] : offsets[k + 1]], in no particular
        order.  tris=None counts only.  Nothing is written beyond tris.size; offsets[boxes.size] says what was needed.  Asynchronous."""
        self._overlaps(N.lib.lbvh_box_overlaps, boxes, L.AABB, offsets, tris)

    def gather_within_distance(self, queries, offsets, tris=None):
        """The same for points with radii (layouts.POINT_QUERY): every triangle within_distance would accept."""
        self._overlaps(N.lib.lbvh_gather_within_distance, queries, L.POINT_QUERY, offsets, tris)

    def _overlaps(self, fn, queries, dtype, offsets, tris):
        if queries.dtype != dtype or offsets.dtype != np.uint64 or offsets.size < queries.size + 1 or \
                (tris is not None and tris.dtype != np.uint32):
            raise ValueError(f"queries must be a DataBuffer of {dtype}, offsets one of uint64 with one entry more, tris one of uint32 or None")
        s = self.container.scene()
        N.check(self.ctx.handle, fn(self.ctx.handle, queries.device, queries.size, C.byref(s), offsets.device,
                                    tris.device if tris is not None else None, tris.size if tris is not None else 0))

    def overlaps(self, queries, min_capacity=1, device_sort=False):
        """Convenience: count -> one 8-byte download -> allocate -> fill.  `queries`: a DataBuffer of layouts.AABB (box form) or of
        layouts.POINT_QUERY (distance form).  Returns (offsets, tris): host arrays, uint64[queries.size + 1] and uint32[total].
        device_sort=True issues sort_index_segments before the download: every segment ascending."""
        return self._csr_lists(self.box_overlaps if queries.dtype == L.AABB else self.gather_within_distance, queries, min_capacity, device_sort)

    def _csr_lists(self, call, queries, min_capacity, device_sort, dtype=np.uint32, segment_sort=sort_index_segments):
        """count -> one 8-byte download -> allocate -> fill -> (device_sort: segment_sort on the device) -> (offsets, records of `dtype`)"""
        count = queries.size
        offsets = DataBuffer(self.ctx, count + 1, np.uint64)
        try:
            call(queries, offsets)
            last = np.zeros(1, dtype=np.uint64)
            N.check(self.ctx.handle, N.lib.lbvh_buffer_download(self.ctx.handle, last.ctypes.data_as(C.c_void_p),
                                                                C.c_void_p(offsets.device.value + 8 * count), 8))
            total = int(last[0])
            records = DataBuffer(self.ctx, max(total, int(min_capacity)), dtype)
            try:
                call(queries, offsets, records)
                if device_sort:
                    segment_sort(self.ctx, offsets, records, count)
                return offsets.get_data().copy(), records.get_data()[:total].copy()
            finally:
                records.dispose()
        finally:
            offsets.dispose()

    def triangle_intersections(self, queries, offsets, tris=None):
        """Every scene triangle each triangle of the DataBuffer `queries` (layouts.TRI_QUERY: a, skip, b, c) intersects — the narrow
        phase behind box_overlaps —, as a CSR list on the caller's buffers exactly as box_overlaps writes it: `offsets` (uint64
        DataBuffer, at least queries.size + 1 entries) always complete, `tris` (uint32 DataBuffer, its size is the capacity) the
        ORIGINAL triangle indices in no particular order; tris=None counts only.  skip = the original index of a scene triangle
        that is never reported (a mesh against itself), layouts.NULL for none.  Asynchronous."""
        self._overlaps(N.lib.lbvh_triangle_intersections, queries, L.TRI_QUERY, offsets, tris)

    def triangle_intersects_any(self, queries, flags):
        """1 into the uint32 DataBuffer `flags` for each triangle of `queries` that intersects any scene triangle, else 0."""
        self._per_query(N.lib.lbvh_triangle_intersects_any, queries, "TRI_QUERY", flags, np.uint32, "queries", "flags")

    def intersections(self, queries, min_capacity=1, device_sort=False):
        """Convenience, as overlaps(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.TRI_QUERY.
        Returns (offsets, tris): host arrays, uint64[queries.size + 1] and uint32[total].  device_sort=True issues
        sort_index_segments before the download: every segment ascending."""
        return self._csr_lists(self.triangle_intersections, queries, min_capacity, device_sort)

    def triangle_intersection_segments(self, queries, offsets, segments=None):
        """WHERE each triangle of the DataBuffer `queries` (layouts.TRI_QUERY) cuts every scene triangle it intersects:
        triangle_intersections with a layouts.TRI_SEGMENT record (the two ends p0, p1 of the shared segment, tri, and `edges`: which
        of the six edge tests passed and which gave each end; see segment_edges) in place of an index.  `offsets` (uint64
        DataBuffer, at least queries.size + 1 entries) receives the words triangle_intersections writes; `segments`
        (layouts.TRI_SEGMENT DataBuffer, its size is the capacity) the records, segment k = segments[offsets[k] : offsets[k + 1]],
        in no particular order; segments=None counts only.  Asynchronous."""
        if queries.dtype != L.TRI_QUERY or offsets.dtype != np.uint64 or offsets.size < queries.size + 1 or \
                (segments is not None and segments.dtype != L.TRI_SEGMENT):
            raise ValueError("queries must be a DataBuffer of layouts.TRI_QUERY, offsets one of uint64 with one entry more, segments one of "
                             "layouts.TRI_SEGMENT or None")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_triangle_intersection_segments(self.ctx.handle, queries.device, queries.size, C.byref(s), offsets.device,
                                                                           segments.device if segments is not None else None,
                                                                           segments.size if segments is not None else 0))

    def intersection_segments(self, queries, sort=False, min_capacity=1, device_sort=False):
        """Convenience, as intersections(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.TRI_QUERY.
        Returns (offsets, records): host arrays, uint64[queries.size + 1] and layouts.TRI_SEGMENT[total], every segment in the
        walk's order.  sort=True orders every segment by `tri` HERE, ON THE HOST (each triangle appears once per segment, so the
        order is total).  device_sort=True issues sort_record_segments before the download instead: the same arrays."""
        off, rec = self._csr_lists(self.triangle_intersection_segments, queries, min_capacity, device_sort, dtype=L.TRI_SEGMENT,
                                   segment_sort=_sort_records_by_dtype)
        if sort and not device_sort:
            segment = np.repeat(np.arange(queries.size), np.diff(off).astype(np.int64))
            rec = rec[np.lexsort((rec["tri"], segment))]
        return off, rec

    def capsule_overlaps(self, shapes, offsets, tris=None):
        """Every triangle each capsule of the DataBuffer `shapes` (layouts.CAPSULE: origin, radius, axis; see capsule_shapes)
        touches where it stands — the start overlap of capsule_cast without a direction —, as a CSR list on the caller's buffers
        exactly as box_overlaps writes it: `offsets` (uint64 DataBuffer, at least shapes.size + 1 entries) always complete, `tris`
        (uint32 DataBuffer, its size is the capacity) the ORIGINAL triangle indices in no particular order; tris=None counts only.
        Asynchronous."""
        self._overlaps(N.lib.lbvh_capsule_overlaps, shapes, L.CAPSULE, offsets, tris)

    def capsule_overlaps_any(self, shapes, flags):
        """1 into the uint32 DataBuffer `flags` for each capsule of `shapes` that touches any triangle, else 0."""
        self._per_query(N.lib.lbvh_capsule_overlaps_any, shapes, "CAPSULE", flags, np.uint32, "shapes", "flags")

    def obb_overlaps(self, shapes, offsets, tris=None):
        """The same for the oriented boxes of the DataBuffer `shapes` (layouts.OBB: centre and the half-axis vectors ax, ay, az; see
        obb_shapes): every triangle each box touches, the start overlap of box_cast without a direction.  Asynchronous."""
        self._overlaps(N.lib.lbvh_obb_overlaps, shapes, L.OBB, offsets, tris)

    def obb_overlaps_any(self, shapes, flags):
        """1 into the uint32 DataBuffer `flags` for each box of `shapes` that touches any triangle, else 0."""
        self._per_query(N.lib.lbvh_obb_overlaps_any, shapes, "OBB", flags, np.uint32, "shapes", "flags")

    def touching(self, shapes, min_capacity=1, device_sort=False):
        """Convenience, as intersections(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.CAPSULE or
        of layouts.OBB.  Returns (offsets, tris): host arrays, uint64[shapes.size + 1] and uint32[total].  device_sort=True issues
        sort_index_segments before the download: every segment ascending."""
        if shapes.dtype not in (L.CAPSULE, L.OBB):
            raise ValueError("shapes must be a DataBuffer of layouts.CAPSULE or layouts.OBB")
        return self._csr_lists(self.capsule_overlaps if shapes.dtype == L.CAPSULE else self.obb_overlaps, shapes, min_capacity, device_sort)

    def capsule_contacts(self, shapes, offsets, contacts=None):
        """How deep each capsule of the DataBuffer `shapes` (layouts.CAPSULE) is in every triangle it touches, and which way out:
        capsule_overlaps with a layouts.CONTACT record (depth, tri, the contact point's u, v on the triangle, the unit push-out
        normal, the contact point's parameter s on the axis) in place of an index.  `offsets` (uint64 DataBuffer, at least
        shapes.size + 1 entries) receives the words capsule_overlaps writes; `contacts` (layouts.CONTACT DataBuffer, its size is the
        capacity) the records, segment k = contacts[offsets[k] : offsets[k + 1]], in no particular order; contacts=None counts
        only.  Asynchronous."""
        if shapes.dtype != L.CAPSULE or offsets.dtype != np.uint64 or offsets.size < shapes.size + 1 or \
                (contacts is not None and contacts.dtype != L.CONTACT):
            raise ValueError("shapes must be a DataBuffer of layouts.CAPSULE, offsets one of uint64 with one entry more, contacts one of "
                             "layouts.CONTACT or None")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_capsule_contacts(self.ctx.handle, shapes.device, shapes.size, C.byref(s), offsets.device,
                                                             contacts.device if contacts is not None else None,
                                                             contacts.size if contacts is not None else 0))

    def capsule_deepest(self, shapes, out):
        """The deepest contact of each capsule of `shapes` (layouts.CAPSULE) into the DataBuffer `out` (layouts.CONTACT): the record
        with the greatest depth, ties to the lower triangle index; tri = layouts.NULL and zeros for a capsule that touches nothing.
        Asynchronous; read with out.get_data()."""
        self._per_query(N.lib.lbvh_capsule_deepest, shapes, "CAPSULE", out, L.CONTACT, "shapes")

    def segment_closest_points(self, queries, out):
        """Nearest triangle of each segment of the DataBuffer `queries` (layouts.SEGMENT_QUERY: origin, max_dist2, axis — the segment
        from origin to origin + axis; see segment_queries) into the DataBuffer `out` (layouts.SEGMENT_CLOSEST: dist2, tri, the nearest
        point (u, v) on the triangle, delta from it to the nearest point origin + axis*s of the segment), over the derived scene.  No
        triangle nearer than sqrt(max_dist2): dist2 = layouts.MAX_FLOAT and zeros.  Asynchronous; read with out.get_data()."""
        self._per_query(N.lib.lbvh_segment_closest_point, queries, "SEGMENT_QUERY", out, L.SEGMENT_CLOSEST, "queries")

    def segment_within_distance(self, queries, flags):
        """1 into the uint32 DataBuffer `flags` for each segment of `queries` with a triangle nearer than sqrt(max_dist2), else 0."""
        self._per_query(N.lib.lbvh_segment_within_distance, queries, "SEGMENT_QUERY", flags, np.uint32, "queries")

    def clearance(self, capsules):
        """Convenience: how far each capsule of `capsules` (a host array or a DataBuffer of layouts.CAPSULE) is from the mesh, by an
        unbounded segment_closest_points on its axis.  Returns (clearance, records): sqrt(dist2) - radius as a float32 host array
        (negative: the capsule is that deep in the nearest triangle; +inf where no triangle was found) and the layouts.SEGMENT_CLOSEST
        records.  Allocates, waits on the host; not part of the word-for-word contract of include/lbvh.h."""
        shapes = capsules.get_data() if isinstance(capsules, DataBuffer) else np.asarray(capsules)
        if shapes.dtype != L.CAPSULE:
            raise ValueError("capsules must be an array or a DataBuffer of layouts.CAPSULE")
        shapes = shapes.reshape(-1)
        n = len(shapes)
        queries = DataBuffer(self.ctx, max(n, 1), L.SEGMENT_QUERY)
        out = DataBuffer(self.ctx, max(n, 1), L.SEGMENT_CLOSEST)
        try:
            queries.local[:n] = segment_queries(shapes["origin"], shapes["axis"], np.inf)
            queries.local[n:]["max_dist2"] = 0                        # (the one spare query of an empty set is inactive)
            queries.sync()
            self.segment_closest_points(queries, out)
            records = out.get_data()[:n].copy()
        finally:
            queries.dispose()
            out.dispose()
        found = records["dist2"] != L.MAX_FLOAT
        with np.errstate(invalid="ignore"):
            gap = np.where(found, np.sqrt(records["dist2"]) - shapes["radius"], np.float32(np.inf)).astype(np.float32)
        return gap, records

    def triangle_closest_points(self, queries, out):
        """Nearest scene triangle of each triangle of the DataBuffer `queries` (layouts.TRI_DISTANCE_QUERY: a, skip, b, max_dist2, c;
        see tri_distance_queries) into the DataBuffer `out` (layouts.TRI_CLOSEST: dist2, tri, the edge test that gave it, s on that
        edge, delta from the scene triangle's nearest point to the query's; see tri_closest_witness), over the derived scene.  No
        triangle nearer than sqrt(max_dist2): dist2 = layouts.MAX_FLOAT and zeros.  Asynchronous; read with out.get_data()."""
        self._per_query(N.lib.lbvh_triangle_closest_point, queries, "TRI_DISTANCE_QUERY", out, L.TRI_CLOSEST, "queries")

    def triangle_within_distance(self, queries, flags):
        """1 into the uint32 DataBuffer `flags` for each triangle of `queries` with a scene triangle nearer than sqrt(max_dist2), else 0."""
        self._per_query(N.lib.lbvh_triangle_within_distance, queries, "TRI_DISTANCE_QUERY", flags, np.uint32, "queries", "flags")

    def mesh_distance(self, other_triangles, max_dist=np.inf):
        """Convenience: the least distance between the mesh `other_triangles` (an array of layouts.TRIANGLE, or a tuple (a, b, c) of
        (n, 3) vertex arrays) and this one, by one triangle_closest_points with max_dist2 = max_dist^2 on every triangle of it.
        Returns (distance, query_index, scene_tri, p_query, p_scene): the least record's sqrt(dist2), which triangle of
        `other_triangles` and which ORIGINAL triangle of this mesh are that near, and the nearest points on them
        (tri_closest_witness); (inf, -1, -1, None, None) where nothing is nearer than max_dist.  On equal dist2 the lower query
        index.  Allocates, waits on the host; not part of the word-for-word contract of include/lbvh.h."""
        q = tri_distance_queries_from_mesh(other_triangles, np.float32(max_dist) * np.float32(max_dist))
        n = len(q)
        queries = DataBuffer(self.ctx, max(n, 1), L.TRI_DISTANCE_QUERY)
        out = DataBuffer(self.ctx, max(n, 1), L.TRI_CLOSEST)
        try:
            queries.local[:n] = q
            queries.local[n:]["max_dist2"] = 0                        # (the one spare query of an empty set is inactive)
            queries.sync()
            self.triangle_closest_points(queries, out)
            records = out.get_data()[:n].copy()
        finally:
            queries.dispose()
            out.dispose()
        found = np.nonzero(records["dist2"] != L.MAX_FLOAT)[0]
        if len(found) == 0:
            return float("inf"), -1, -1, None, None
        k = int(found[np.argmin(records["dist2"][found])])
        tris = self.container.triangle_data.local[:self.container.triangles_length]
        p_query, p_scene = tri_closest_witness(q[k:k + 1], tris, records[k:k + 1])
        return float(np.sqrt(np.float64(records["dist2"][k]))), k, int(records["tri"][k]), p_query[0], p_scene[0]

    def triangle_gather_within_distance(self, queries, offsets, records=None):
        """EVERY scene triangle within sqrt(max_dist2) of each triangle of the DataBuffer `queries` (layouts.TRI_DISTANCE_QUERY), one
        layouts.TRI_CLOSEST record per pair — what triangle_closest_points would write were that triangle the only one —, as a CSR
        list on the caller's buffers: `offsets` (uint64 DataBuffer, at least queries.size + 1 entries) always complete; `records`
        (layouts.TRI_CLOSEST DataBuffer, its size is the capacity), segment k = records[offsets[k] : offsets[k + 1]], in no
        particular order; records=None counts only.  Asynchronous."""
        if queries.dtype != L.TRI_DISTANCE_QUERY or offsets.dtype != np.uint64 or offsets.size < queries.size + 1 or \
                (records is not None and records.dtype != L.TRI_CLOSEST):
            raise ValueError("queries must be a DataBuffer of layouts.TRI_DISTANCE_QUERY, offsets one of uint64 with one entry more, records "
                             "one of layouts.TRI_CLOSEST or None")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_triangle_gather_within_distance(self.ctx.handle, queries.device, queries.size, C.byref(s),
                                                                            offsets.device, records.device if records is not None else None,
                                                                            records.size if records is not None else 0))

    def proximity_pairs(self, other, max_dist, self_skip=False, sort=False, min_capacity=1, device_sort=False):
        """Convenience, as contacts(): count -> one 8-byte download -> allocate -> fill.  `other`: an array of
        layouts.TRI_DISTANCE_QUERY (taken as it is: max_dist and self_skip are not applied), or a mesh as mesh_distance takes it (an
        array of layouts.TRIANGLE or a tuple (a, b, c) of (n, 3) vertex arrays), every triangle of it with max_dist2 = max_dist^2 and,
        self_skip=True, skip = its own index (this mesh against itself; see unique_self_pairs).  Returns (offsets, records): host
        arrays, uint64[n + 1] and layouts.TRI_CLOSEST[total], every segment in the walk's order; sort=True orders every segment by
        (dist2, tri) HERE, ON THE HOST; device_sort=True issues sort_record_segments before the download instead: the same
        arrays.  Allocates, waits on the host."""
        if isinstance(other, np.ndarray) and other.dtype == L.TRI_DISTANCE_QUERY:
            q = other.reshape(-1)
        else:
            q = tri_distance_queries_from_mesh(other, np.float32(max_dist) * np.float32(max_dist), self_skip)
        n = len(q)
        if n == 0:
            return np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=L.TRI_CLOSEST)
        queries = DataBuffer(self.ctx, n, L.TRI_DISTANCE_QUERY)
        try:
            queries.local[:] = q
            queries.sync()
            off, rec = self._csr_lists(self.triangle_gather_within_distance, queries, min_capacity, device_sort, dtype=L.TRI_CLOSEST,
                                       segment_sort=_sort_records_by_dtype)
        finally:
            queries.dispose()
        if sort and not device_sort:
            segment = np.repeat(np.arange(n), np.diff(off).astype(np.int64))
            rec = rec[np.lexsort((rec["tri"], rec["dist2"], segment))]
        return off, rec

    def obb_contacts(self, shapes, offsets, contacts=None):
        """The same for the oriented boxes of the DataBuffer `shapes` (layouts.OBB): obb_overlaps with a layouts.BOX_CONTACT record
        (depth = the least push along normal that frees the box from the triangle, tri, axis = which of box_cast's thirteen axes
        gave it, back = the push along -normal, the unit push-out normal) in place of an index.  `offsets` receives the words
        obb_overlaps writes; `contacts` (layouts.BOX_CONTACT DataBuffer, its size is the capacity) the records, in no particular
        order inside a segment; contacts=None counts only.  Asynchronous."""
        if shapes.dtype != L.OBB or offsets.dtype != np.uint64 or offsets.size < shapes.size + 1 or \
                (contacts is not None and contacts.dtype != L.BOX_CONTACT):
            raise ValueError("shapes must be a DataBuffer of layouts.OBB, offsets one of uint64 with one entry more, contacts one of "
                             "layouts.BOX_CONTACT or None")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_obb_contacts(self.ctx.handle, shapes.device, shapes.size, C.byref(s), offsets.device,
                                                         contacts.device if contacts is not None else None,
                                                         contacts.size if contacts is not None else 0))

    def obb_deepest(self, shapes, out):
        """The deepest contact of each box of `shapes` (layouts.OBB) into the DataBuffer `out` (layouts.BOX_CONTACT): the record with
        the greatest depth, ties to the lower triangle index; tri = layouts.NULL and zeros for a box that touches nothing.
        Asynchronous; read with out.get_data()."""
        self._per_query(N.lib.lbvh_obb_deepest, shapes, "OBB", out, L.BOX_CONTACT, "shapes")

    def contacts(self, shapes, min_capacity=1, device_sort=False):
        """Convenience, as touching(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.CAPSULE or of
        layouts.OBB.  Returns (offsets, contacts): host arrays, uint64[shapes.size + 1] and layouts.CONTACT[total] (capsules) or
        layouts.BOX_CONTACT[total] (boxes), every segment in the walk's order.  device_sort=True issues sort_record_segments
        before the download: every segment deepest first, the lower triangle index first on equal depth — its first record is
        capsule_deepest's / obb_deepest's."""
        if shapes.dtype not in (L.CAPSULE, L.OBB):
            raise ValueError("shapes must be a DataBuffer of layouts.CAPSULE or layouts.OBB")
        if shapes.dtype == L.OBB:
            return self._csr_lists(self.obb_contacts, shapes, min_capacity, device_sort, dtype=L.BOX_CONTACT, segment_sort=_sort_records_by_dtype)
        return self._csr_lists(self.capsule_contacts, shapes, min_capacity, device_sort, dtype=L.CONTACT, segment_sort=_sort_records_by_dtype)

    def region_overlaps(self, regions, mode, offsets, tris=None):
        """Every triangle in each convex region of the DataBuffer `regions` (layouts.REGION: six planes {nx, ny, nz, d}, each keeping
        n . x + d >= 0; see frustum_planes, obb_planes, aabb_planes), as a CSR list on the caller's buffers exactly as box_overlaps
        writes it.  mode = layouts.REGION_TOUCHING: the triangles whose own box is not wholly outside any plane (the conservative
        frustum test); layouts.REGION_CONTAINED: those whose own box is wholly inside every plane.  tris=None counts only.
        Asynchronous."""
        if mode not in (L.REGION_TOUCHING, L.REGION_CONTAINED):
            raise ValueError("mode must be layouts.REGION_TOUCHING or layouts.REGION_CONTAINED")
        self._overlaps(lambda h, q, n, s, o, t, cap: N.lib.lbvh_region_overlaps(h, q, n, mode, s, o, t, cap), regions, L.REGION, offsets, tris)

    def region_overlaps_large(self, regions, mode, offsets, tris=None):
        """region_overlaps for few large regions (one camera frustum, a cascade, a marquee selection; at most
        _native.REGION_LARGE_MAX_COUNT of them): each region is spread over the device instead of over one lane
        (lbvh_region_overlaps_large).  The same offsets and, per segment, the same set of indices, in another order.  Asynchronous."""
        if mode not in (L.REGION_TOUCHING, L.REGION_CONTAINED):
            raise ValueError("mode must be layouts.REGION_TOUCHING or layouts.REGION_CONTAINED")
        if regions.size > N.REGION_LARGE_MAX_COUNT:
            raise ValueError(f"region_overlaps_large takes at most {N.REGION_LARGE_MAX_COUNT} regions")
        self._overlaps(lambda h, q, n, s, o, t, cap: N.lib.lbvh_region_overlaps_large(h, q, n, mode, s, o, t, cap), regions, L.REGION, offsets, tris)

    def plane_sections(self, planes, offsets, segments=None):
        """WHERE each plane of the DataBuffer `planes` (layouts.PLANE: n, d with n . x + d = 0; see host.planes) cuts the mesh: one
        layouts.PLANE_SEGMENT record per cut triangle (p0 and p1 on two of its edges, tri, and `edges`: which edges and the three
        sides; see host.section_edges), every plane spread over the device (lbvh_plane_sections; at most
        _native.PLANE_SECTIONS_MAX_COUNT planes).  `offsets` (uint64 DataBuffer, at least planes.size + 1 entries) is always
        complete; `segments` (layouts.PLANE_SEGMENT DataBuffer, its size is the capacity) receives the records, segment k =
        segments[offsets[k] : offsets[k + 1]], in no particular order; segments=None counts only.  Asynchronous."""
        if planes.dtype != L.PLANE or offsets.dtype != np.uint64 or offsets.size < planes.size + 1 or \
                (segments is not None and segments.dtype != L.PLANE_SEGMENT):
            raise ValueError("planes must be a DataBuffer of layouts.PLANE, offsets one of uint64 with one entry more, segments one of "
                             "layouts.PLANE_SEGMENT or None")
        if planes.size > N.PLANE_SECTIONS_MAX_COUNT:
            raise ValueError(f"plane_sections takes at most {N.PLANE_SECTIONS_MAX_COUNT} planes")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_plane_sections(self.ctx.handle, planes.device, planes.size, C.byref(s), offsets.device,
                                                           segments.device if segments is not None else None,
                                                           segments.size if segments is not None else 0))

    def cross_sections(self, planes, stitch=False, min_capacity=1, device_sort=False):
        """Convenience: count -> one 8-byte download -> allocate -> fill -> download, for layouts.PLANE records on the host (see
        host.planes) or a DataBuffer of them.  Returns (offsets, records): uint64[count + 1] and layouts.PLANE_SEGMENT[total],
        every segment ordered by `tri` on the host — or, device_sort=True, on the device before the download
        (sort_record_segments): the same arrays.  stitch=True returns instead a list with one (loops, chains) of
        host.stitch_sections per plane, stitched through the scene's own triangle records."""
        own = not isinstance(planes, DataBuffer)
        if own:
            host_planes = np.ascontiguousarray(planes, dtype=L.PLANE).reshape(-1)
            if len(host_planes) == 0:
                return [] if stitch else (np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=L.PLANE_SEGMENT))
            planes = DataBuffer(self.ctx, len(host_planes), L.PLANE)
            planes.local[:] = host_planes
            planes.sync()
        try:
            off, rec = self._csr_lists(self.plane_sections, planes, min_capacity, device_sort, dtype=L.PLANE_SEGMENT,
                                       segment_sort=_sort_records_by_dtype)
            if not device_sort:
                segment = np.repeat(np.arange(planes.size), np.diff(off).astype(np.int64))
                rec = rec[np.lexsort((rec["tri"], segment))]
        finally:
            if own:
                planes.dispose()
        if not stitch:
            return off, rec
        tris = self.container.triangle_data.local[:self.container.triangles_length]
        return [stitch_sections(rec[int(off[k]):int(off[k + 1])], tris) for k in range(len(off) - 1)]

    def region_overlaps_any(self, regions, mode, flags):
        """1 into the uint32 DataBuffer `flags` for each region of `regions` that has a candidate in `mode`, else 0."""
        if mode not in (L.REGION_TOUCHING, L.REGION_CONTAINED):
            raise ValueError("mode must be layouts.REGION_TOUCHING or layouts.REGION_CONTAINED")
        self._per_query(lambda h, q, n, s, f: N.lib.lbvh_region_overlaps_any(h, q, n, mode, s, f), regions, "REGION", flags, np.uint32, "regions", "flags")

    def in_regions(self, regions, mode=L.REGION_TOUCHING, min_capacity=1, device_sort=False, large=False):
        """Convenience, as overlaps(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.REGION.
        Returns (offsets, tris): host arrays, uint64[regions.size + 1] and uint32[total].  device_sort=True issues
        sort_index_segments before the download: every segment ascending.  large=True: through region_overlaps_large."""
        call = self.region_overlaps_large if large else self.region_overlaps
        return self._csr_lists(lambda q, o, t=None: call(q, mode, o, t), regions, min_capacity, device_sort)

    def count_hits(self, rays, counts):
        """The number of candidates of each ray of `rays` (layouts.RAY) in (t_min, t_max) into the uint32 DataBuffer `counts`: every
        triangle crossed counts, two at the same t count 2.  Asynchronous."""
        self._per_query(N.lib.lbvh_count_hits, rays, "RAY", counts, np.uint32, "rays")

    def trace_k_closest(self, rays, k, hits, found=None):
        """The first k hits (1 <= k <= 32) along each ray of `rays` (layouts.RAY) into the DataBuffer `hits` (layouts.HIT, at least
        rays.size * k entries): row q = hits[q * k : (q + 1) * k], nearest first, ties by the lower triangle index, padded with
        miss records {MAX_FLOAT, 0, 0, 0}.  `found` (uint32 DataBuffer, optional) receives the number of real records per row.
        Asynchronous; read with hits.get_data()[: rays.size * k].reshape(-1, k)."""
        k = int(k)
        if rays.dtype != L.RAY or hits.dtype != L.HIT or hits.size < rays.size * k or \
                (found is not None and (found.dtype != np.uint32 or found.size < rays.size)):
            raise ValueError("rays must be a DataBuffer of layouts.RAY, hits one of layouts.HIT with k entries per ray, found one of "
                             "uint32 with at least as many entries as rays, or None")
        if not 1 <= k <= N.K_CLOSEST_MAX:
            raise ValueError(f"k must be 1 .. {N.K_CLOSEST_MAX}")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_trace_k_closest(self.ctx.handle, rays.device, rays.size, k, C.byref(s), hits.device,
                                                            found.device if found is not None else None))

    def gather_hits(self, rays, offsets, hits=None):
        """Every hit along each ray of `rays` (layouts.RAY) as a CSR list on the caller's buffers: `offsets` (uint64 DataBuffer, at
        least rays.size + 1 entries) always complete; `hits` (layouts.HIT DataBuffer, its size is the capacity) receives the
        records, segment q = hits[offsets[q] : offsets[q + 1]], IN NO PARTICULAR ORDER (each record carries its t).  hits=None
        counts only.  Nothing is written beyond hits.size; offsets[rays.size] says what was needed.  Asynchronous."""
        if rays.dtype != L.RAY or offsets.dtype != np.uint64 or offsets.size < rays.size + 1 or \
                (hits is not None and hits.dtype != L.HIT):
            raise ValueError("rays must be a DataBuffer of layouts.RAY, offsets one of uint64 with one entry more, hits one of layouts.HIT or None")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_gather_hits(self.ctx.handle, rays.device, rays.size, C.byref(s), offsets.device,
                                                        hits.device if hits is not None else None, hits.size if hits is not None else 0))

    def all_hits(self, rays, sort=False, min_capacity=1, device_sort=False):
        """Convenience: count -> one 8-byte download -> allocate -> fill.  Returns (offsets, hits): host arrays, uint64[rays.size + 1]
        and layouts.HIT[total].  The library leaves a segment in the order of its walk; sort=True orders every segment by
        (t, tri) HERE, ON THE HOST (np.lexsort over the downloaded records — not a device sort).  device_sort=True issues
        sort_hit_segments before the download instead: the same order, made on the device."""
        off, rec = self._csr_lists(self.gather_hits, rays, min_capacity, device_sort, L.HIT, sort_hit_segments)
        if sort:
            segment = np.repeat(np.arange(rays.size), np.diff(off).astype(np.int64))
            rec = rec[np.lexsort((rec["tri"], rec["t"], segment))]
        return off, rec

    def sphere_cast_all(self, casts, offsets, hits=None):
        """EVERY triangle each moving sphere of `casts` (layouts.SPHERE_RAY) touches before t_max, as a CSR list on the caller's
        buffers exactly as gather_hits writes it: `offsets` (uint64 DataBuffer, at least casts.size + 1 entries) always complete;
        `hits` (layouts.HIT DataBuffer, its size is the capacity) receives the records sphere_cast would write were that triangle
        the first, segment q = hits[offsets[q] : offsets[q + 1]], IN NO PARTICULAR ORDER (each record carries its t).  hits=None
        counts only.  Nothing is written beyond hits.size; offsets[casts.size] says what was needed.  Asynchronous."""
        self._cast_all(N.lib.lbvh_sphere_cast_all, casts, "SPHERE_RAY", offsets, hits, "HIT")

    def capsule_cast_all(self, casts, offsets, hits=None):
        """The same for the moving capsules of `casts` (layouts.CAPSULE_RAY): capsule_cast's record of every triangle touched."""
        self._cast_all(N.lib.lbvh_capsule_cast_all, casts, "CAPSULE_RAY", offsets, hits, "HIT")

    def box_cast_all(self, casts, offsets, hits=None):
        """The same for the moving boxes of `casts` (layouts.BOX_RAY), `hits` a layouts.BOX_HIT DataBuffer: box_cast's record
        (t, tri, axis) of every triangle touched.  sort_hit_segments takes these records as they are."""
        self._cast_all(N.lib.lbvh_box_cast_all, casts, "BOX_RAY", offsets, hits, "BOX_HIT")

    def triangle_cast_all(self, casts, offsets, hits=None):
        """The same for the moving triangles of `casts` (layouts.TRI_RAY, as tri_casts makes them), `hits` a layouts.TRI_CAST_HIT
        DataBuffer: triangle_cast's record (t, tri, feature, w) of every triangle touched, `skip` never among them.
        sort_hit_segments takes these records as they are."""
        self._cast_all(N.lib.lbvh_triangle_cast_all, casts, "TRI_RAY", offsets, hits, "TRI_CAST_HIT")

    def mesh_sweep_all(self, other_triangles, direction, t_max, sort=True):
        """Convenience, the "all" twin of mesh_sweep: every pair of a triangle of the mesh `other_triangles` (layouts.TRIANGLE, or a
        tuple (a, b, c) of (n, 3) arrays) and a triangle of this mesh that touch while the other mesh moves along `direction` for
        0 <= t < t_max — one triangle_cast_all over one cast per moving triangle, count -> allocate -> fill.  Returns
        (moving, tri, t, feature, w): five arrays with one entry per pair, `moving` the index into other_triangles and the rest the
        layouts.TRI_CAST_HIT words.  sort=True orders the rows by (t, moving, tri), so row 0 is mesh_sweep's answer; sort=False
        leaves them grouped by moving triangle, each group in the order of the walk.  Blocking."""
        casts = tri_casts_from_mesh(other_triangles, direction, t_max)
        buf = DataBuffer(self.ctx, len(casts), L.TRI_RAY)
        try:
            buf.local[:] = casts
            buf.sync()
            off, rec = self.cast_all(buf)
        finally:
            buf.dispose()
        moving = np.repeat(np.arange(len(casts), dtype=np.int64), np.diff(off).astype(np.int64))
        if sort:
            order = np.lexsort((rec["tri"], moving, rec["t"]))
            moving, rec = moving[order], rec[order]
        return moving, rec["tri"].copy(), rec["t"].copy(), rec["feature"].copy(), rec["w"].copy()

    def _cast_all(self, fn, casts, layout, offsets, hits, record):
        if casts.dtype != getattr(L, layout) or offsets.dtype != np.uint64 or offsets.size < casts.size + 1 or \
                (hits is not None and hits.dtype != getattr(L, record)):
            raise ValueError(f"casts must be a DataBuffer of layouts.{layout}, offsets one of uint64 with one entry more, hits one of "
                             f"layouts.{record} or None")
        s = self.container.scene()
        N.check(self.ctx.handle, fn(self.ctx.handle, casts.device, casts.size, C.byref(s), offsets.device,
                                    hits.device if hits is not None else None, hits.size if hits is not None else 0))

    def cast_all(self, casts, sort=False, device_sort=False, min_capacity=1):
        """Convenience, as all_hits(): count -> one 8-byte download -> allocate -> fill, for a DataBuffer of layouts.SPHERE_RAY,
        layouts.CAPSULE_RAY, layouts.BOX_RAY or layouts.TRI_RAY.  Returns (offsets, records): host arrays, uint64[casts.size + 1] and
        layouts.HIT[total] (layouts.BOX_HIT[total] for boxes, layouts.TRI_CAST_HIT[total] for triangles).  sort=True orders every
        segment by (t, tri) on the host; device_sort=True issues sort_hit_segments before the download instead."""
        calls = {L.SPHERE_RAY: (self.sphere_cast_all, L.HIT), L.CAPSULE_RAY: (self.capsule_cast_all, L.HIT), L.BOX_RAY: (self.box_cast_all, L.BOX_HIT),
                 L.TRI_RAY: (self.triangle_cast_all, L.TRI_CAST_HIT)}
        if casts.dtype not in calls:
            raise ValueError("casts must be a DataBuffer of layouts.SPHERE_RAY, layouts.CAPSULE_RAY, layouts.BOX_RAY or layouts.TRI_RAY")
        call, record = calls[casts.dtype]
        off, rec = self._csr_lists(call, casts, min_capacity, device_sort, record, sort_hit_segments)
        if sort:
            segment = np.repeat(np.arange(casts.size), np.diff(off).astype(np.int64))
            rec = rec[np.lexsort((rec["tri"], rec["t"], segment))]
        return off, rec

    def point_crossings(self, queries, parity, dirs=None):
        """Bit j of the uint32 DataBuffer `parity` for each point of `queries` (layouts.POINT_QUERY; max_dist2 is not read): the
        parity of the number of triangles the ray from the point along dirs[j] crosses (dirs: up to 32 rows of x, y, z;
        default DEFAULT_DIRS).  inside(parity, len(dirs)) turns the words into inside / outside.  Asynchronous."""
        d = np.ascontiguousarray(DEFAULT_DIRS if dirs is None else dirs, dtype=np.float32).reshape(-1, 3)
        if queries.dtype != L.POINT_QUERY or parity.dtype != np.uint32 or parity.size < queries.size:
            raise ValueError("queries must be a DataBuffer of layouts.POINT_QUERY and parity one of uint32 with at least as many entries")
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_point_crossings(self.ctx.handle, queries.device, queries.size,
                                                            d.ctypes.data_as(C.POINTER(C.c_float)), len(d), C.byref(s), parity.device))

    def update(self, camera, rect=None, mode=L.TRACE_FAST, stats=False):
        """Enqueue one frame (or the sub-rectangle (x0, y0, x1, y1) of it).  Returns the device
        hit buffer; read it back with hits()."""
        cam = N.Camera.from_dict(camera)
        x0, y0, x1, y1 = rect if rect is not None else (0, 0, cam.screen_width, cam.screen_height)
        count = max((x1 - x0) * (y1 - y0), 1)
        if self._hits is None or self._hits.size < count:
            if self._hits is not None:
                self._hits.dispose()
            self._hits = DataBuffer(self.ctx, count, L.HIT)
        if stats and self._stats is None:
            self._stats = DataBuffer(self.ctx, 1, L.TRACE_STATS)
        self._rect = (x0, y0, x1, y1)
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_trace_primary(
            self.ctx.handle, C.byref(cam), x0, y0, x1, y1, C.byref(s), mode, self._hits.device,
            self._stats.device if stats else None))
        return self._hits

    def update_shard(self, camera, shard_index, shard_count, mode=L.TRACE_FAST, stats=False):
        """One launch tracing this GPU's share of the full frame: every shard_count-th group of 8
        adjacent tiles.  The hit buffer is full-frame sized; only the shard's pixels are written."""
        cam = N.Camera.from_dict(camera)
        count = cam.screen_width * cam.screen_height
        if self._hits is None or self._hits.size < count:
            if self._hits is not None:
                self._hits.dispose()
            self._hits = DataBuffer(self.ctx, count, L.HIT)
        if stats and self._stats is None:
            self._stats = DataBuffer(self.ctx, 1, L.TRACE_STATS)
        self._rect = (0, 0, cam.screen_width, cam.screen_height)
        s = self.container.scene()
        N.check(self.ctx.handle, N.lib.lbvh_trace_primary_shard(
            self.ctx.handle, C.byref(cam), shard_index, shard_count, C.byref(s), mode, self._hits.device,
            self._stats.device if stats else None))
        return self._hits

    def hits(self):
        x0, y0, x1, y1 = self._rect
        return self._hits.get_data()[: (x1 - x0) * (y1 - y0)].reshape(y1 - y0, x1 - x0).copy()

    def set_texture(self, rgba8):
        """_objectDrawer.SetTexture("_meshTexture", ...) (Assets/_Scripts/RaytracingMeshDrawer.cs:61):
        (h, w, 4) uint8, row 0 at v = 0."""
        tex = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert tex.ndim == 3 and tex.shape[2] == 4
        self._tex_shape = tex.shape
        self._tex = DataBuffer(self.ctx, tex.size // 4, np.uint32)
        self._tex.local[:] = tex.reshape(-1, 4).view(np.uint32).reshape(-1)
        self._tex.sync()

    def shade(self):
        """The shading tail of the Raytracing kernel over the last update()'s hit records -> RGBA16F."""
        x0, y0, x1, y1 = self._rect
        count = (x1 - x0) * (y1 - y0)
        if getattr(self, "_image", None) is None or self._image.size < count:
            self._image = DataBuffer(self.ctx, count, np.uint64)       # 4 halves per pixel
        N.check(self.ctx.handle, N.lib.lbvh_shade(
            self.ctx.handle, self._hits.device, count, self.container.triangle_data.device, self._tex.device,
            self._tex_shape[1], self._tex_shape[0], self._image.device))
        return self._image

    def on_render_image(self, src):
        """OnRenderImage (Assets/_Scripts/RaytracingMeshDrawer.cs:86-90): Graphics.Blit(src, dest, _imageComposerMaterial) —
        the shaded image laid over the camera's own rendering `src` ((h, w, 4) float16); returns dest as float16."""
        x0, y0, x1, y1 = self._rect
        count = (x1 - x0) * (y1 - y0)
        bg = np.ascontiguousarray(src, dtype=np.float16)
        assert bg.shape == (y1 - y0, x1 - x0, 4)
        buf = DataBuffer(self.ctx, count, np.uint64)
        buf.local[:] = bg.reshape(-1, 4).view(np.uint64).reshape(-1)
        buf.sync()
        N.check(self.ctx.handle, N.lib.lbvh_compose(self.ctx.handle, buf.device, self._image.device, count, buf.device))
        out = buf.get_data()[:count].view(np.float16).reshape(y1 - y0, x1 - x0, 4).copy()
        buf.dispose()
        return out

    def image(self):
        x0, y0, x1, y1 = self._rect
        n = (x1 - x0) * (y1 - y0)
        return self._image.get_data()[:n].view(np.float16).reshape(y1 - y0, x1 - x0, 4).copy()

    def stats(self):
        return self._stats.get_data()[0].copy()

    def on_destroy(self):                                            # OnDestroy :118-123
        if self.container:
            self.container.dispose()
        for b in (self._hits, self._stats):
            if b is not None:
                b.dispose()


class MultiGpuDrawer:
    """One frame from N GPUs driven by one process (twin of host/lbvh_host.hpp MultiGpuDrawer; BASELINE configs[2]): one
    Context + one replica of the scene per entry of `devices` (a device may repeat: logical ranks on one GPU), every build
    call enqueued round-robin, and update() = every context traces its share straight into ONE full-frame buffer on the
    first device (peer-mapped stores, no second pass) + the first context's stream waits for the others' completion events
    on the device.  The reference renders one image per Update() (Assets/_Scripts/RaytracingMeshDrawer.cs:76-89): this is
    where the N shares become that image."""

    def __init__(self, devices, triangles, capacity=None):
        self.contexts = [Context(d) for d in devices]
        self.drawers = [RaytracingMeshDrawer(c, triangles, capacity) for c in self.contexts]
        self.done = [c.sync_event() for c in self.contexts]
        self.consumed = self.contexts[0].sync_event()
        for c in self.contexts[1:]:
            c.peer_enable(devices[0])
        self.frame = None
        self._shape = None

    @property
    def owner(self):
        return self.contexts[0]

    def awake(self, fast=True):
        for d in self.drawers:                       # replicas: the same deterministic build on every GPU
            d.awake(fast=fast)
        return self

    def rebuild(self, fast=True):
        for d in self.drawers:
            d.rebuild(fast=fast)

    def update(self, camera, mode=L.TRACE_FAST):
        cam = N.Camera.from_dict(camera)
        count = cam.screen_width * cam.screen_height
        if self.frame is None or self.frame.size < count:
            self.sync()                              # nobody may still be writing the old buffer
            if self.frame is not None:
                self.frame.dispose()
            self.frame = DataBuffer(self.owner, count, L.HIT)
        self._shape = (cam.screen_height, cam.screen_width)
        n = len(self.contexts)
        self.owner.record(self.consumed)             # the owner's reads of the previous frame end here
        for c in self.contexts[1:]:
            c.wait_event(self.consumed)
        for r, (c, d) in enumerate(zip(self.contexts, self.drawers)):
            s = d.container.scene()
            N.check(c.handle, N.lib.lbvh_trace_primary_shard(c.handle, C.byref(cam), r, n, C.byref(s), mode, self.frame.device, None))
            if r:
                c.record(self.done[r])
        for r in range(1, n):
            self.owner.wait_event(self.done[r])      # the gather: a device-side wait, nothing is copied
        return self.frame

    def hits(self):
        h, w = self._shape
        return self.frame.get_data()[: h * w].reshape(h, w).copy()

    def sync(self):
        for c in self.contexts:
            c.sync()

    def on_destroy(self):
        self.sync()
        if self.frame is not None:
            self.frame.dispose()
        for d in self.drawers:
            d.on_destroy()
        for c, e in zip(self.contexts, self.done):
            c.destroy_event(e)
        self.owner.destroy_event(self.consumed)
        for c in self.contexts:
            c.close()


class MultiGpuSorter:
    """ComputeBufferSorter over N contexts of one process (twin of host/lbvh_host.hpp MultiGpuSorter; BASELINE configs[3]): one
    Context per entry of `devices` (a device may repeat: logical ranks on one GPU) and one lbvh_sort_pairs_sharded call per
    sort — the key-range sharded sort whose multi-process twin is sharded_sort.ShardedSorter.  Block i lives on context i; the
    result is context q's slice of the globally sorted sequence, or (replicate) the whole sequence on every context."""

    def __init__(self, devices):
        self.contexts = [Context(d) for d in devices]
        self._inputs = [None] * len(self.contexts)       # per context: (keys, values) DataBuffers, grown on demand
        self._outputs = [None] * len(self.contexts)

    def sort_device(self, keys, values, counts, out_keys, out_values, capacities, replicate=False):
        """The C call on device pointers (one of each per context; ints or c_void_p).  Asynchronous apart from its one host
        wait; the inputs come back locally sorted.  Returns the slice lengths."""
        n = len(self.contexts)
        arr = lambda t, xs: (t * n)(*[x.value if isinstance(x, C.c_void_p) else x for x in xs])    # noqa: E731
        ctxs = (C.c_void_p * n)(*[c.handle.value for c in self.contexts])
        out_counts = (C.c_uint32 * n)()
        N.check(self.contexts[0].handle, N.lib.lbvh_sort_pairs_sharded(
            ctxs, n, arr(C.c_void_p, keys), arr(C.c_void_p, values), arr(C.c_uint32, counts), arr(C.c_void_p, out_keys),
            arr(C.c_void_p, out_values), arr(C.c_uint32, capacities), out_counts, N.SORT_SHARDED_REPLICATE if replicate else 0))
        return list(out_counts)

    def _buffers(self, slots, i, size):
        if slots[i] is None or slots[i][0].size < size:
            if slots[i] is not None:
                for b in slots[i]:
                    b.dispose()
            slots[i] = (DataBuffer(self.contexts[i], max(size, 1), np.uint32), DataBuffer(self.contexts[i], max(size, 1), np.uint32))
        return slots[i]

    def sort(self, blocks, replicate=False):
        """blocks: one (keys, values) pair of u32 host arrays per context.  Returns ([(keys, values)] per context, counts):
        context q's slice of the sorted sequence (replicate: the whole sequence), as host arrays."""
        assert len(blocks) == len(self.contexts)
        blocks = [(np.ascontiguousarray(k, dtype=np.uint32), np.ascontiguousarray(v, dtype=np.uint32)) for k, v in blocks]
        total = sum(len(k) for k, _ in blocks)
        ins, outs = [], []
        for i, (k, v) in enumerate(blocks):
            assert len(k) == len(v)
            bk, bv = self._buffers(self._inputs, i, len(k))
            bk.local[: len(k)] = k
            bv.local[: len(v)] = v
            bk.sync()
            bv.sync()
            ins.append((bk, bv))
            outs.append(self._buffers(self._outputs, i, total))       # any slice may need all N pairs
        counts = self.sort_device([b[0].device for b in ins], [b[1].device for b in ins], [len(k) for k, _ in blocks],
                                  [o[0].device for o in outs], [o[1].device for o in outs], [o[0].size for o in outs],
                                  replicate=replicate)
        res = []
        for q, (ok, ov) in enumerate(outs):
            m = total if replicate else counts[q]
            res.append((ok.get_data()[:m].copy(), ov.get_data()[:m].copy()))
        return res, counts

    def sync(self):
        for c in self.contexts:
            c.sync()

    def close(self):
        for c in self.contexts:
            if c.handle:
                c.sync()
        for slots in (self._inputs, self._outputs):
            for pair in slots:
                if pair is not None:
                    for b in pair:
                        b.dispose()
        self._inputs = [None] * len(self.contexts)
        self._outputs = [None] * len(self.contexts)
        for c in self.contexts:
            c.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DynamicPathTracer:
    """SURVEY 8(f) rank 3 / BASELINE configs[4] (extension, no reference counterpart): per frame the rigid bodies
    are rotated (lbvh_animate), the whole LBVH is rebuilt on the same buffers (RaytracingMeshDrawer.rebuild), primary
    rays go through the packet kernel and `bounces` diffuse bounces through lbvh_trace_rays / lbvh_path_scatter."""

    def __init__(self, ctx, rest_triangles, body_ids, body_centres, t_min=1e-3, albedo=0.7, seed=1):
        self.ctx = ctx
        self.drawer = RaytracingMeshDrawer(ctx, rest_triangles).awake()
        n = self.drawer.container.triangles_length
        self.rest = DataBuffer(ctx, n, L.TRIANGLE)
        self.rest.local[:] = np.ascontiguousarray(rest_triangles, dtype=L.TRIANGLE)
        self.rest.sync()
        self.body = DataBuffer(ctx, n, np.uint32)
        self.body.local[:] = np.ascontiguousarray(body_ids, dtype=np.uint32)
        self.body.sync()
        ctr = np.ascontiguousarray(body_centres, dtype=np.float32).reshape(-1, 4)
        self.centres = DataBuffer(ctx, ctr.size, np.float32)
        self.centres.local[:] = ctr.reshape(-1)
        self.centres.sync()
        self.t_min, self.albedo, self.seed = float(t_min), float(albedo), int(seed)
        self.states = self.hits = self.image_buf = None

    def animate(self, angle, fused=True):
        """the bodies turned to `angle` and the whole LBVH rebuilt: lbvh_animate_build_scene (one call; fused=False: lbvh_animate +
        the rebuild as two — same results)"""
        c = self.drawer.container
        cs, sn = float(np.float32(np.cos(angle))), float(np.float32(np.sin(angle)))
        if not fused:
            N.check(self.ctx.handle, N.lib.lbvh_animate(
                self.ctx.handle, self.rest.device, c.triangles_length, self.body.device, self.centres.device, cs, sn, c.triangle_data.device))
            self.drawer.rebuild(fast=True)
            return
        f3 = C.POINTER(C.c_float)
        N.check(self.ctx.handle, N.lib.lbvh_animate_build_scene(
            self.ctx.handle, self.rest.device, self.body.device, self.centres.device, cs, sn, c.triangle_data.device, c.triangles_length,
            c.capacity, c.box_min.ctypes.data_as(f3), c.box_max.ctypes.data_as(f3), c.keys.device, c.triangle_index.device,
            c.triangle_aabb.device, c.bvh_internal_node.device, c.bvh_leaf_node.device, c.bvh_data.device,
            L.BUILD_RESET_NODES | L.BUILD_FAST_SCENE))

    def render(self, camera, bounces=4):
        cam = N.Camera.from_dict(camera)
        count = cam.screen_width * cam.screen_height
        if self.states is None or self.states.size < count:
            self.states = DataBuffer(self.ctx, count, L.PATH_STATE)
            self.hits = DataBuffer(self.ctx, count, L.HIT)
            self.image_buf = DataBuffer(self.ctx, count, np.uint64)
        h = self.ctx.handle
        s = self.drawer.container.scene()
        # primary rays: the coherent packet kernel — BEFORE the path states are initialised: 132 MB of state stores right
        # in front of it push the scene out of the caches (the frame's primary trace 0.274 -> 0.253 ms)
        N.check(h, N.lib.lbvh_trace_primary(h, C.byref(cam), 0, 0, cam.screen_width, cam.screen_height, C.byref(s),
                                            L.TRACE_FAST, self.hits.device, None))
        # bounce b = scatter at the hits of segment b + trace of segment b + 1 (one call); the first one also makes the path
        # states from the camera (lbvh_path_first_bounce = lbvh_path_begin + bounce 0); the last bounce only scatters
        if bounces == 0:
            N.check(h, N.lib.lbvh_path_begin(h, C.byref(cam), self.states.device))
        else:
            N.check(h, N.lib.lbvh_path_first_bounce(h, C.byref(cam), C.byref(s), self.states.device, self.hits.device, self.seed,
                                                    self.albedo, self.t_min))
        for b in range(1, bounces):
            N.check(h, N.lib.lbvh_path_bounce(h, C.byref(s), self.states.device, self.hits.device, count, b, self.seed,
                                              self.albedo, self.t_min))
        N.check(h, N.lib.lbvh_path_scatter(h, C.byref(s), self.hits.device, count, bounces, self.seed, self.albedo,
                                           self.states.device))
        N.check(h, N.lib.lbvh_path_resolve(h, self.states.device, count, self.image_buf.device))
        self._shape = (cam.screen_height, cam.screen_width)
        return self.image_buf

    def image(self):
        n = self._shape[0] * self._shape[1]
        return self.image_buf.get_data()[:n].view(np.float16).reshape(self._shape + (4,)).copy()
