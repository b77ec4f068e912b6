"""Buffer element layouts of the hot path as numpy dtypes.

Bit-for-bit the reference's structs (Assets/_Shaders/Constants.cginc:9-54,
Assets/_Scripts/SceneDataTypes.cs:4-89) and include/lbvh.h.
"""
import numpy as np

AABB = np.dtype([("min", "<f4", 3), ("_dummy0", "<f4"), ("max", "<f4", 3), ("_dummy1", "<f4")])
TRIANGLE = np.dtype([
    ("a", "<f4", 3), ("_dummy0", "<f4"),
    ("b", "<f4", 3), ("_dummy1", "<f4"),
    ("c", "<f4", 3), ("_dummy2", "<f4"),
    ("a_uv", "<f4", 2), ("b_uv", "<f4", 2), ("c_uv", "<f4", 2), ("_dummy3", "<f4", 2),
    ("a_normal", "<f4", 3), ("_dummy4", "<f4"),
    ("b_normal", "<f4", 3), ("_dummy5", "<f4"),
    ("c_normal", "<f4", 3), ("_dummy6", "<f4"),
])
INTERNAL_NODE = np.dtype([
    ("leftNode", "<u4"), ("leftNodeType", "<u4"), ("rightNode", "<u4"), ("rightNodeType", "<u4"),
    ("parent", "<u4"), ("index", "<u4"),
])
LEAF_NODE = np.dtype([("parent", "<u4"), ("index", "<u4")])
HIT = np.dtype([("t", "<f4"), ("tri", "<u4"), ("u", "<f4"), ("v", "<f4")])
TRACE_STATS = np.dtype([("pops", "<u8"), ("box_hits", "<u8"), ("leaf_tests", "<u8"),
                        ("tri_tests", "<u8"), ("hits", "<u8")])

BUILD_FAST_SCENE, BUILD_RESET_NODES = 1, 2      # lbvh_build_scene flags

RAY_STATS = np.dtype([("rays", "<u8"), ("node_fetches", "<u8"), ("triangle_tests", "<u8")])
PATH_STATE = np.dtype([("origin", "<f4", 3), ("alive", "<u4"), ("dir", "<f4", 3), ("pad0", "<f4"),
                       ("throughput", "<f4", 3), ("pad1", "<f4"), ("radiance", "<f4", 3), ("alpha", "<f4")])
assert PATH_STATE.itemsize == 64
# lbvh_trace_closest / lbvh_trace_occluded: a ray of the caller's own, active iff t_min < t_max
RAY = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4")])
assert RAY.itemsize == 32
# lbvh_sphere_cast / lbvh_sphere_cast_any: lbvh_ray with the sphere's radius where t_min is
SPHERE_RAY = np.dtype([("origin", "<f4", 3), ("radius", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4")])
assert SPHERE_RAY.itemsize == 32
# lbvh_capsule_cast / lbvh_capsule_cast_any: the sphere's record and the axis (the other end is origin + axis)
CAPSULE_RAY = np.dtype([("origin", "<f4", 3), ("radius", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4"), ("axis", "<f4", 3), ("_pad", "<u4")])
assert CAPSULE_RAY.itemsize == 48
# lbvh_box_cast / lbvh_box_cast_any: a moving box { centre + s0*ax + s1*ay + s2*az : |s_i| <= 1 } (three half-axis vectors; the pads
# are not read) and its record; axis = the separating axis that gave the time, BOX_AXIS_START = overlapping at the start
BOX_RAY = np.dtype([("centre", "<f4", 3), ("t_max", "<f4"), ("dir", "<f4", 3), ("_pad0", "<u4"), ("ax", "<f4", 3), ("_pad1", "<u4"),
                    ("ay", "<f4", 3), ("_pad2", "<u4"), ("az", "<f4", 3), ("_pad3", "<u4")])
BOX_HIT = np.dtype([("t", "<f4"), ("tri", "<u4"), ("axis", "<u4"), ("_zero", "<u4")])
assert BOX_RAY.itemsize == 80 and BOX_HIT.itemsize == 16
BOX_AXIS_START = 13
# lbvh_closest_point_query / lbvh_within_distance: a point with its squared search radius (active iff max_dist2 > 0), and the answer
POINT_QUERY = np.dtype([("p", "<f4", 3), ("max_dist2", "<f4")])
CLOSEST_POINT = np.dtype([("dist2", "<f4"), ("tri", "<u4"), ("u", "<f4"), ("v", "<f4")])
assert POINT_QUERY.itemsize == 16 and CLOSEST_POINT.itemsize == 16
# lbvh_triangle_intersections / lbvh_triangle_intersects_any: a query triangle; skip = the ORIGINAL index of a scene triangle that is
# never a candidate (NULL below, LBVH_NULL: none)
TRI_QUERY = np.dtype([("a", "<f4", 3), ("skip", "<u4"), ("b", "<f4", 3), ("_pad0", "<u4"), ("c", "<f4", 3), ("_pad1", "<u4")])
assert TRI_QUERY.itemsize == 48
# lbvh_triangle_cast / lbvh_triangle_cast_any: a triangle moving along dir without turning (the pads are not read) and its record;
# feature = which pair gave the time (0 - 2 a moving vertex on the scene face, 3 - 5 a scene vertex on the moving face, 6 + 3m + n
# moving edge m on scene edge n, w the position on that scene edge), TRI_CAST_START | j = the triangles intersect at the start
TRI_RAY = np.dtype([("a", "<f4", 3), ("skip", "<u4"), ("b", "<f4", 3), ("t_max", "<f4"), ("c", "<f4", 3), ("_pad0", "<u4"),
                    ("dir", "<f4", 3), ("_pad1", "<u4")])
TRI_CAST_HIT = np.dtype([("t", "<f4"), ("tri", "<u4"), ("feature", "<u4"), ("w", "<f4")])
assert TRI_RAY.itemsize == 64 and TRI_CAST_HIT.itemsize == 16
TRI_CAST_START = 16
# lbvh_triangle_intersection_segments: where a query triangle cuts scene triangle `tri` — the two ends p0, p1 and `edges`: bits 0 .. 5
# which of the six edge tests passed, bits 8 .. 10 the test that gave p0, bits 12 .. 14 the one that gave p1 (host.segment_edges)
TRI_SEGMENT = np.dtype([("p0", "<f4", 3), ("tri", "<u4"), ("p1", "<f4", 3), ("edges", "<u4")])
assert TRI_SEGMENT.itemsize == 32
# lbvh_plane_sections: a plane n . x + d = 0, and where it cuts scene triangle `tri` — p0 the crossing on the edge that leaves the
# positive side, p1 the one on the edge that returns to it, and `edges`: bits 0 .. 2 the two crossing edges (v0-v1, v1-v2, v2-v0),
# bits 8 .. 9 the edge that gave p0, bits 12 .. 13 the one that gave p1, bits 16 .. 18 the sides of v0, v1, v2 (host.section_edges)
PLANE = np.dtype([("n", "<f4", 3), ("d", "<f4")])
PLANE_SEGMENT = np.dtype([("p0", "<f4", 3), ("tri", "<u4"), ("p1", "<f4", 3), ("edges", "<u4")])
assert PLANE.itemsize == 16 and PLANE_SEGMENT.itemsize == 32
# lbvh_capsule_overlaps / lbvh_obb_overlaps and their _any forms: a capsule (the segment origin .. origin + axis and the radius) and
# an oriented box { centre + s0*ax + s1*ay + s2*az : |s_i| <= 1 } where they stand — CAPSULE_RAY and BOX_RAY without the motion;
# the pads are not read
CAPSULE = np.dtype([("origin", "<f4", 3), ("radius", "<f4"), ("axis", "<f4", 3), ("_pad", "<u4")])
OBB = np.dtype([("centre", "<f4", 3), ("_pad0", "<u4"), ("ax", "<f4", 3), ("_pad1", "<u4"), ("ay", "<f4", 3), ("_pad2", "<u4"),
                ("az", "<f4", 3), ("_pad3", "<u4")])
assert CAPSULE.itemsize == 32 and OBB.itemsize == 64
# lbvh_capsule_contacts / lbvh_capsule_deepest: one contact of a capsule with a triangle — depth = radius - distance of the axis from
# the triangle, (u, v) the contact point on the triangle, normal the unit push-out direction, s the contact point on the axis; the
# none-record of lbvh_capsule_deepest has tri = NULL below and zeros elsewhere
CONTACT = np.dtype([("depth", "<f4"), ("tri", "<u4"), ("u", "<f4"), ("v", "<f4"), ("normal", "<f4", 3), ("s", "<f4")])
assert CONTACT.itemsize == 32
# lbvh_segment_closest_point / lbvh_segment_within_distance: the segment origin .. origin + axis with its squared search radius (CAPSULE
# with the bound in place of the radius; active iff max_dist2 > 0), and the answer: dist2 of the segment from triangle `tri`, (u, v) the
# nearest point on the triangle, delta from it to the nearest point of the segment, origin + axis*s; the none-record is
# {MAX_FLOAT, 0, 0, 0, (0, 0, 0), 0}
SEGMENT_QUERY = np.dtype([("origin", "<f4", 3), ("max_dist2", "<f4"), ("axis", "<f4", 3), ("_pad", "<u4")])
SEGMENT_CLOSEST = np.dtype([("dist2", "<f4"), ("tri", "<u4"), ("u", "<f4"), ("v", "<f4"), ("delta", "<f4", 3), ("s", "<f4")])
assert SEGMENT_QUERY.itemsize == 32 and SEGMENT_CLOSEST.itemsize == 32
# lbvh_triangle_closest_point / lbvh_triangle_within_distance: TRI_QUERY with a squared search radius (active iff max_dist2 > 0 and all
# nine coordinates are finite), and the answer: dist2 of the query triangle from triangle `tri`, given by edge test `edge` & 7 (0 .. 2:
# the query's edges from a, b, c against the scene triangle; 3 .. 5: the scene triangle's edges v0-v1, v0-v2, v1-v2 against the query;
# | 8: that edge pierces), s the nearest point's parameter on that edge, delta from the scene triangle's nearest point to the query's;
# the none-record is {MAX_FLOAT, 0, 0, 0, (0, 0, 0), 0}
TRI_DISTANCE_QUERY = np.dtype([("a", "<f4", 3), ("skip", "<u4"), ("b", "<f4", 3), ("max_dist2", "<f4"), ("c", "<f4", 3), ("_pad", "<u4")])
TRI_CLOSEST = np.dtype([("dist2", "<f4"), ("tri", "<u4"), ("edge", "<u4"), ("s", "<f4"), ("delta", "<f4", 3), ("_zero", "<u4")])
assert TRI_DISTANCE_QUERY.itemsize == 48 and TRI_CLOSEST.itemsize == 32
# lbvh_obb_contacts / lbvh_obb_deepest: one contact of an oriented box with a triangle — depth = the least push along normal that
# separates them, axis the j of the box cast's thirteen axes that gave it (BOX_AXIS_START: none counted), back the push along
# -normal on the same axis; the none-record of lbvh_obb_deepest has tri = NULL below and zeros elsewhere
BOX_CONTACT = np.dtype([("depth", "<f4"), ("tri", "<u4"), ("axis", "<u4"), ("back", "<f4"), ("normal", "<f4", 3), ("_zero", "<u4")])
assert BOX_CONTACT.itemsize == 32
# lbvh_region_overlaps / lbvh_region_overlaps_any: six planes {nx, ny, nz, d}, each keeping n . x + d >= 0; the two modes
REGION = np.dtype([("plane", "<f4", (6, 4))])
assert REGION.itemsize == 96
REGION_TOUCHING, REGION_CONTAINED = 0, 1

assert AABB.itemsize == 32          # Assets/_Scripts/MeshBufferContainer.cs:103
assert TRIANGLE.itemsize == 128     # Assets/_Scripts/MeshBufferContainer.cs:98
assert INTERNAL_NODE.itemsize == 24
assert LEAF_NODE.itemsize == 8
assert HIT.itemsize == 16

INTERNAL = 0                         # Assets/_Shaders/Constants.cginc:17
LEAF = 1                             # Assets/_Shaders/Constants.cginc:18
NULL = 0xFFFFFFFF                    # NullLeaf words, Assets/_Scripts/SceneDataTypes.cs:63-71
MAX_FLOAT = np.float32(2139095040.0)  # (float)0x7F7FFFFF, Assets/_Shaders/Constants.cginc:7

TRACE_REFERENCE = 0
TRACE_FAST = 1
TRACE_FAST_EXACT = 2      # TRACE_FAST + rays that meet an exact t tie re-traced by the reference's walk: == TRACE_REFERENCE, every word

# Scene box the reference hard-wires for Morton normalisation
# (Assets/_Scripts/MeshBufferContainer.cs:9-15)
SCENE_BOX_MIN = np.array([-125.0, -125.0, -125.0], dtype=np.float32)
SCENE_BOX_MAX = np.array([125.0, 125.0, 125.0], dtype=np.float32)
