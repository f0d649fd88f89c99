"""Helpers the mesh-deformation tests share (TriangleMesh.set_vertices -> srt_deform_colliders, csrc/rt_deform.h).
The reference throughout is existing code: an OBJ file holding the deformed vertices (written with %r, so the floats
round-trip; every other record of the source file copied), loaded by TriangleMesh with the same flags, lowered by
`collider_record`, uploaded in the ordinary way and rendered by the oracle.  Also the two deformations of the tests,
and the bindings of the host check harness's functions (rt_hostcheck.cpp hc_deform_triangles / hc_deform_refit /
hc_deform_nearest)."""
import ctypes

import numpy as np

import mesh_pose_ref as MP
from sightpy import _native as N
from sightpy._lower import lower_scene
from sightpy.geometry.triangle_mesh import TriangleMesh


def twist(P, deg_per_unit=60.0, scale=(1.3, 0.8, 1.1)):
    """No pose can express it: every vertex turned about the y axis by an angle proportional to its y, then scaled
    along x / y / z."""
    P = np.asarray(P, dtype=np.float64)
    a = np.deg2rad(deg_per_unit) * P[:, 1]
    x = np.cos(a) * P[:, 0] + np.sin(a) * P[:, 2]
    z = -np.sin(a) * P[:, 0] + np.cos(a) * P[:, 2]
    return np.stack([x, P[:, 1], z], axis=1) * np.asarray(scale, dtype=np.float64)


def bulge(P, amount=0.35):
    """A second, different deformation: vertices pushed outward by a wave along x, and sheared."""
    P = np.asarray(P, dtype=np.float64)
    out = P * (1.0 + amount * np.sin(7.0 * P[:, :1] + 0.5))
    out[:, 0] += 0.4 * P[:, 1]
    return out


def write_deformed_obj(src, dst, P):
    """`src` with its k-th `v` record replaced by P[k]; returns dst."""
    k = 0
    with open(src) as fi, open(dst, "w") as fo:
        for line in fi.read().split("\n"):
            tok = line.split()
            if tok and tok[0] == "v":
                fo.write("v %r %r %r\n" % tuple(float(x) for x in P[k]))
                k += 1
            elif tok:
                fo.write(line + "\n")
    assert k == len(P)
    return dst


def mesh_of(sc, k=0):
    return [p for p in sc.scene_primitives if isinstance(p, TriangleMesh)][k]


def mesh_range(sc, k=0):
    """(first, count) of the k-th mesh in the scene's collider list."""
    m = mesh_of(sc, k)
    first = next(i for i, c in enumerate(sc.collider_list) if c is m.collider_list[0])
    return first, len(m.collider_list)


def center_of(mesh):
    return np.array([mesh.center.x, mesh.center.y, mesh.center.z], dtype=np.float64)


# ---- the host check harness ---------------------------------------------------------------------------
def _lib():
    import hostcheck as HC

    lib = HC.lib()
    P = ctypes.c_void_p
    mesh = [ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P]  # first, count, n_verts, corner, recompute, center, P
    ranges = [ctypes.c_int, P, P, P]
    lib.hc_deform_triangles.argtypes = [P] + mesh[1:] + [P]
    lib.hc_deform_refit.argtypes = [ctypes.POINTER(N.SceneDesc)] + mesh + ranges + [P, ctypes.c_int, P, ctypes.c_int, P, P]
    lib.hc_deform_nearest.argtypes = [ctypes.POINTER(N.SceneDesc)] + mesh + ranges + [P, P, ctypes.c_int64, P, P, P]
    return lib


def _mesh_args(mesh, P, first=None):
    corners = np.ascontiguousarray(mesh.corners, dtype=np.int32)
    flags = np.ascontiguousarray(mesh._recompute, dtype=np.uint8)
    center = center_of(mesh)
    P = np.ascontiguousarray(P, dtype=np.float64)
    keep = (corners, flags, center, P)
    head = () if first is None else (first,)
    return head + (len(corners), len(P), N.ptr(corners), N.ptr(flags), N.ptr(center), N.ptr(P)), keep


def _range_args(ranges):
    if not ranges:
        return (0, None, None, None), ()
    first, count, poses = MP._ranges(ranges)
    return (len(first), N.ptr(first), N.ptr(count), N.ptr(poses)), (first, count, poses)


def hc_deform_triangles(mesh, rest, P, corners=None):
    """The records `rest` of `mesh` under the vertex array P, as k_deform_triangles writes them (None: the harness
    refused a corner index); `corners` replaces the mesh's corner table."""
    rest = np.ascontiguousarray(rest)
    out = np.zeros_like(rest)
    args, keep = _mesh_args(mesh, P)
    if corners is not None:
        corners = np.ascontiguousarray(corners, dtype=np.int32)
        args = (args[0], args[1], N.ptr(corners)) + args[3:]
    rc = _lib().hc_deform_triangles(N.ptr(rest), *args, N.ptr(out))
    return out if rc == 0 else None


def hc_deform_refit(scene, k, P, ranges=()):
    """(nodes, leaf slots' collider indices, the collider table, bvh_bound) of the scene's BVH after deforming its
    k-th mesh to P, refitting, and posing `ranges` [(first, count, pose), ...] from the deformed table."""
    L = lower_scene(scene)
    d = L.desc()
    mesh = mesh_of(scene, k)
    margs, keep = _mesh_args(mesh, P, first=mesh_range(scene, k)[0])
    rargs, keep2 = _range_args(ranges)
    lib = _lib()
    n = lib.hc_deform_refit(ctypes.byref(d), *margs, *rargs, None, 0, None, 0, None, None)
    assert n >= 0
    nodes = np.zeros(n, dtype=MP.NODE_DTYPE)
    tri = np.full(len(L.colliders), -1, dtype=np.int32)
    table = np.zeros_like(L.colliders)
    bound = ctypes.c_float(0.0)
    lib.hc_deform_refit(ctypes.byref(d), *margs, *rargs, N.ptr(nodes) if n else None, n, N.ptr(tri), len(tri),
                        N.ptr(table), ctypes.byref(bound))
    return nodes, tri, table, float(bound.value)


def hc_deform_nearest(scene, k, P, O, D, ranges=()):
    """hostcheck.nearest on the scene with its k-th mesh deformed to P and `ranges` posed (through the refitted
    BVH, or with HC.set_bvh(0) the linear loop over the rewritten table): (t, collider id, orientation)."""
    L = lower_scene(scene)
    d = L.desc()
    mesh = mesh_of(scene, k)
    margs, keep = _mesh_args(mesh, P, first=mesh_range(scene, k)[0])
    rargs, keep2 = _range_args(ranges)
    O = np.ascontiguousarray(O, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    n = O.shape[1]
    t, ids, orient = np.empty(n), np.empty(n, np.int32), np.empty(n)
    rc = _lib().hc_deform_nearest(ctypes.byref(d), *margs, *rargs, N.ptr(O), N.ptr(D), n, N.ptr(t), N.ptr(ids),
                                  N.ptr(orient))
    assert rc == 0
    return t, ids, orient
