"""numpy restatement of TriangleMesh.set_pose (srt_pose_colliders, csrc/rt_pose.h) and the helpers the mesh-pose
tests share: the 12 numbers of a pose, the posed vertices and vertex normals by the documented rule, a mesh
primitive built from explicit vertex arrays (so that the oracle, `collider_record` and an ordinary upload see
exactly the restated vertices), the scene restated with such meshes, and the bindings of the host check
harness's pose functions (rt_hostcheck.cpp hc_pose_triangles / hc_bvh_refit / hc_pose_nearest)."""
import copy
import ctypes

import numpy as np

from sightpy import _native as N
from sightpy import vec3
from sightpy._lower import collider_record, lower_scene
from sightpy.geometry.primitive import Primitive
from sightpy.geometry.triangle import Triangle_Collider
from sightpy.geometry.triangle_mesh import TriangleMesh

IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
NODE_DTYPE = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<i4", (4,)), ("count", "<i4", (4,))])
BVH_EMPTY = -(2 ** 31)


def rotation(theta_deg, axis):
    """Rodrigues' rotation matrix about `axis` (any length)."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    t = np.deg2rad(theta_deg)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def pose_numbers(R, center, t=(0.0, 0.0, 0.0)):
    """R row-major then T = center - R center + t (what set_pose hands to the device)."""
    R = np.asarray(R, dtype=np.float64)
    c = np.asarray(center, dtype=np.float64)
    return np.concatenate([R.reshape(-1), c - R @ c + np.asarray(t, dtype=np.float64)])


def rotate_rows(V, pose):
    """(..., 3): ((R[k][0] x + R[k][1] y) + R[k][2] z) per component k, in this order."""
    R = np.asarray(pose)[:9].reshape(3, 3)
    x, y, z = V[..., 0], V[..., 1], V[..., 2]
    return np.stack([(R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z for k in range(3)], axis=-1)


def posed_vertices(V, pose):
    """The rule of srt_pose_colliders for vertices V (..., 3)."""
    return rotate_rows(V, pose) + np.asarray(pose)[9:]


def mesh_arrays(mesh):
    """(vertices (n, 3, 3), vertex normals (n, 3, 3) or None, uvs (n, 3, 2) or None) of a mesh's Python colliders."""
    cl = mesh.collider_list
    V = np.array([[[p.x, p.y, p.z] for p in (c.p1, c.p2, c.p3)] for c in cl], dtype=np.float64)
    Nn = None if cl[0].normals is None else np.array([[[n.x, n.y, n.z] for n in c.normals] for c in cl], dtype=np.float64)
    UV = None if cl[0].uvs is None else np.array([c.uvs for c in cl], dtype=np.float64)
    return V, Nn, UV


class ExplicitMesh(Primitive):
    """A mesh primitive from explicit arrays: vertices (n, 3, 3), raw vertex normals (n, 3, 3) or None
    (Triangle_Collider normalises them), uvs (n, 3, 2) or None.  It takes its other fields from `like` without
    touching that primitive's material."""

    def __init__(self, like, V, normals=None, uvs=None):
        self.center, self.material, self.shadow = like.center, like.material, like.shadow
        self.max_ray_depth, self.mc = like.max_ray_depth, like.mc
        self.collider_list = []
        for k in range(len(V)):
            nn = None if normals is None else tuple(vec3(*(float(v) for v in normals[k, i])) for i in range(3))
            uv = None if uvs is None else tuple((float(uvs[k, i, 0]), float(uvs[k, i, 1])) for i in range(3))
            p = [vec3(*(float(v) for v in V[k, i])) for i in range(3)]
            self.collider_list.append(Triangle_Collider(assigned_primitive=self, p1=p[0], p2=p[1], p3=p[2],
                                                        normals=nn, uvs=uv))


def restated_mesh(mesh, pose=None):
    """ExplicitMesh of `mesh` under `pose` (default: the mesh's own; None: its rest pose) by the rule above."""
    pose = mesh.pose if pose is None else pose
    V, Nn, UV = mesh_arrays(mesh)
    if pose is not None:
        V = posed_vertices(V, pose)
        Nn = None if Nn is None else rotate_rows(Nn, pose)
    return ExplicitMesh(mesh, V, Nn, UV)


def restated_scene(scene):
    """A copy of `scene` in which every TriangleMesh is an ExplicitMesh of its posed vertices: what an ordinary
    lowering, upload and the oracle see as the posed scene."""
    out = copy.copy(scene)
    out._history = None
    shadowed = {id(c) for c in scene.shadowed_collider_list}
    out.scene_primitives, out.collider_list, out.shadowed_collider_list = [], [], []
    for prim in scene.scene_primitives:
        p2 = restated_mesh(prim) if isinstance(prim, TriangleMesh) else prim
        out.scene_primitives.append(p2)
        out.collider_list += p2.collider_list
        if prim.collider_list and id(prim.collider_list[0]) in shadowed:
            out.shadowed_collider_list += p2.collider_list
    return out


def records(colliders):
    """collider_record of each collider, as one table."""
    out = np.zeros(len(colliders), dtype=N.COLLIDER_DTYPE)
    for k, c in enumerate(colliders):
        out[k] = collider_record(c)
    return out


# ---- the host check harness ---------------------------------------------------------------------------
def _lib():
    import hostcheck as HC

    lib = HC.lib()
    lib.hc_pose_triangles.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_pose_triangles.restype = None
    lib.hc_bvh_refit.argtypes = [ctypes.POINTER(N.SceneDesc), ctypes.c_int] + [ctypes.c_void_p] * 4 + \
                                [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_pose_nearest.argtypes = [ctypes.POINTER(N.SceneDesc), ctypes.c_int] + [ctypes.c_void_p] * 5 + \
                                   [ctypes.c_int64] + [ctypes.c_void_p] * 3
    return lib


def hc_pose_triangles(recs, pose):
    recs = np.ascontiguousarray(recs)
    pose = np.ascontiguousarray(pose, dtype=np.float64)
    out = np.zeros_like(recs)
    _lib().hc_pose_triangles(N.ptr(recs), len(recs), N.ptr(pose), N.ptr(out))
    return out


def _ranges(ranges):
    first = np.array([r[0] for r in ranges], dtype=np.int32)
    count = np.array([r[1] for r in ranges], dtype=np.int32)
    poses = np.ascontiguousarray([r[2] for r in ranges], dtype=np.float64).reshape(-1, 12)
    return first, count, poses


def hc_bvh_refit(scene, ranges):
    """(nodes (NODE_DTYPE), leaf slots' collider indices, the posed collider table, bvh_bound) of the scene's BVH
    after posing `ranges` [(first, count, pose), ...] and refitting on the host; no ranges: the built tree."""
    L = lower_scene(scene)
    d = L.desc()
    first, count, poses = _ranges(ranges)
    lib = _lib()
    args = (ctypes.byref(d), len(first), N.ptr(first) if len(first) else None, N.ptr(count) if len(first) else None,
            N.ptr(poses) if len(first) else None)
    n = lib.hc_bvh_refit(*args, None, 0, None, 0, None, None)
    nodes = np.zeros(n, dtype=NODE_DTYPE)
    tri = np.full(len(L.colliders), -1, dtype=np.int32)
    posed = np.zeros_like(L.colliders)
    bound = ctypes.c_float(0.0)
    lib.hc_bvh_refit(*args, N.ptr(nodes) if n else None, n, N.ptr(tri), len(tri), N.ptr(posed), ctypes.byref(bound))
    return nodes, tri, posed, float(bound.value)


def hc_pose_nearest(scene, ranges, O, D):
    """hostcheck.nearest on the scene with `ranges` posed (through the refitted BVH, or with HC.set_bvh(0) the
    linear loop over the posed table): (t, collider id, orientation)."""
    L = lower_scene(scene)
    d = L.desc()
    first, count, poses = _ranges(ranges)
    O = np.ascontiguousarray(O, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = O.shape[1]
    t, ids, orient = np.empty(n), np.empty(n, np.int32), np.empty(n)
    _lib().hc_pose_nearest(ctypes.byref(d), len(first), N.ptr(first), N.ptr(count), N.ptr(poses), N.ptr(O), N.ptr(D),
                           n, N.ptr(t), N.ptr(ids), N.ptr(orient))
    return t, ids, orient
