"""Expected values for triangles with per-vertex normals / texture coordinates (tests/test_vattr.py,
tests/test_gpu_vattr.py): the interpolation restated in numpy, wrapped around the oracle's
module-level `collider_normal` / `collider_uv` for the length of one test (the oracle's shaders call
them by global name, so render_linear / trace_linear / shade_linear then shade smooth, textured
triangles with the reference's own material code); the OBJ files and scenes of those tests.

The interpolation at a point P of the triangle, float64, in this order:
    b2 = dot(n31, P - p1) / d2,  d2 = dot(n31, p2 - p1)
    b3 = dot(n12, P - p2) / d3,  d3 = dot(n12, p3 - p2)
    b1 = (1.0 - b2) - b3
    normal = normalize(n1*b1 + n2*b2 + n3*b3), the face normal if that sum is exactly zero
    u = u1*b1 + u2*b2 + u3*b3, v likewise
"""
import ctypes

import numpy as np

import sightpy_oracle as O
import scenes
from sightpy import Scene, Sphere, Plane, Glossy, TriangleMesh, image, rgb, vec3
from sightpy import _native as N
from sightpy._lower import collider_record

_ORIG = {"normal": O.collider_normal, "uv": O.collider_uv}


def bary(c, P):
    """(b1, b2, b3) of the points P (3, n) on Triangle_Collider c."""
    d2 = c.n31.dot(c.p2 - c.p1)
    d3 = c.n12.dot(c.p3 - c.p2)
    b2 = O.dot(O.col3(c.n31), P - O.col3(c.p1)) / d2
    b3 = O.dot(O.col3(c.n12), P - O.col3(c.p2)) / d3
    b1 = (1.0 - b2) - b3
    return b1, b2, b3


def interp_normal(c, P):
    b1, b2, b3 = bary(c, P)
    n1, n2, n3 = (O.col3(n) for n in c.normals)
    s = n1 * b1 + n2 * b2 + n3 * b3
    zero = (s[0] == 0.0) & (s[1] == 0.0) & (s[2] == 0.0)
    return np.where(zero, O.col3(c.normal), O.normalize(s))


def interp_uv(c, P):
    b1, b2, b3 = bary(c, P)
    (u1, v1), (u2, v2), (u3, v3) = c.uvs
    return u1 * b1 + u2 * b2 + u3 * b3, v1 * b1 + v2 * b2 + v3 * b3


def collider_normal(c, P):
    if O._kind(c) == "Triangle_Collider" and getattr(c, "normals", None) is not None:
        return interp_normal(c, P)
    return _ORIG["normal"](c, P)


def collider_uv(c, P):
    if O._kind(c) == "Triangle_Collider" and getattr(c, "uvs", None) is not None:
        return interp_uv(c, P)
    return _ORIG["uv"](c, P)


def patch(monkeypatch):
    """Wrap the oracle's collider_normal / collider_uv until the test ends."""
    monkeypatch.setattr(O, "collider_normal", collider_normal)
    monkeypatch.setattr(O, "collider_uv", collider_uv)


# ---- OBJ files ------------------------------------------------------------------------------------
def _read_obj(path):
    V, F = [], []
    for line in open(path):
        tok = line.split()
        if tok and tok[0] == "v":
            V.append([float(x) for x in tok[1:4]])
        elif tok and tok[0] == "f":
            F.append([int(t.split("/")[0]) - 1 for t in tok[1:4]])
    return np.array(V), F


def spherical_uv(V):
    """sphere.py:58-64's coordinates of the unit directions of V (n, 3)."""
    M = V / np.linalg.norm(V, axis=1, keepdims=True)
    return (np.arctan2(M[:, 2], M[:, 0]) + np.pi) / (2 * np.pi), (np.arcsin(M[:, 1]) + np.pi / 2) / np.pi


def write_smooth_icosphere_obj(path, subdiv, radius=0.5):
    """scenes.write_icosphere_obj's icosphere with `vn` = the unit vertex positions and `vt` = their
    spherical coordinates, faces written 'v/vt/vn'.  Returns (vertices (n, 3), faces)."""
    scenes.write_icosphere_obj(path, subdiv=subdiv, radius=radius, slash_format=False)
    V, F = _read_obj(path)
    u, v = spherical_uv(V)
    with open(path, "w") as fh:
        for p in V:
            fh.write("v %.17g %.17g %.17g\n" % tuple(p))
        for p in V / np.linalg.norm(V, axis=1, keepdims=True):
            fh.write("vn %.17g %.17g %.17g\n" % tuple(p))
        for a, b in zip(u, v):
            fh.write("vt %.17g %.17g\n" % (a, b))
        for a, b, c in F:
            fh.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a + 1, a + 1, a + 1, b + 1, b + 1, b + 1, c + 1, c + 1, c + 1))
    return V, F


def write_tetrahedron_obj(path, radius=0.5):
    """Four triangles (below the BVH threshold of 8: the linear triangle loop), `vn` = the unit vertex
    positions, `vt` = their spherical coordinates."""
    V = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    V = radius * V / np.linalg.norm(V, axis=1, keepdims=True)
    F = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    u, v = spherical_uv(V)
    with open(path, "w") as fh:
        for p in V:
            fh.write("v %.17g %.17g %.17g\n" % tuple(p))
        for p in V / np.linalg.norm(V, axis=1, keepdims=True):
            fh.write("vn %.17g %.17g %.17g\n" % tuple(p))
        for a, b in zip(u, v):
            fh.write("vt %.17g %.17g\n" % (a, b))
        for a, b, c in F:
            fh.write("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a + 1, a + 1, a + 1, b + 1, b + 1, b + 1, c + 1, c + 1, c + 1))
    return V, F


# ---- scenes ---------------------------------------------------------------------------------------
def checker():
    return Glossy(diff_color=image("checkered_floor.png", repeat=4.0), n=vec3(1.5 + 0.2j, 1.5 + 0.2j, 1.5 + 0.2j),
                  roughness=0.2, spec_coeff=0.4, diff_coeff=0.8)


def mesh_scene(obj_path, width=64, height=48, depth=3, center=(0.35, 0.05, -1.0), material=None, smooth=True,
               texcoords=False, extra=None):
    """scenes.mesh_scene (the same spheres, floor, light, camera and sky box) whose TriangleMesh takes
    `smooth` / `texcoords` and another material; `extra` adds one more primitive before the floor."""
    red = Glossy(diff_color=rgb(0.6, 0.1, 0.1), n=vec3(1.5 + 0.2j, 1.5 + 0.2j, 1.5 + 0.2j), roughness=0.2,
                 spec_coeff=0.4, diff_coeff=0.8)
    gold = Glossy(diff_color=rgb(1.0, 0.572, 0.184), n=vec3(0.15 + 3.58j, 0.4 + 2.37j, 1.54 + 1.91j),
                  roughness=0.0, spec_coeff=0.2, diff_coeff=0.8)
    floor = Glossy(diff_color=image("checkered_floor.png", repeat=20.0), n=vec3(1.2 + 0.3j, 1.2 + 0.3j, 1.1 + 0.3j),
                   roughness=0.2, spec_coeff=0.3, diff_coeff=0.9)
    sc = Scene(ambient_color=rgb(0.05, 0.05, 0.05))
    sc.add_Camera(look_from=vec3(0.3, 0.6, 1.8), look_at=vec3(0.0, 0.0, -1.0), screen_width=width,
                  screen_height=height)
    sc.add_DirectionalLight(Ldir=vec3(0.52, 0.45, -0.5), color=rgb(0.5, 0.5, 0.5))
    sc.add(Sphere(material=gold, center=vec3(-0.8, 0.0, -1.2), radius=0.45, max_ray_depth=depth))
    sc.add(TriangleMesh(obj_path, center=vec3(*center), material=red if material is None else material,
                        max_ray_depth=depth, smooth=smooth, texcoords=texcoords))
    if extra is not None:
        sc.add(extra)
    sc.add(Plane(material=floor, center=vec3(0, -0.5, -2.0), width=40.0, height=40.0, u_axis=vec3(1.0, 0, 0),
                 v_axis=vec3(0, 0, -1.0), max_ray_depth=depth))
    sc.add_Background("stormydays.png")
    return sc


def mesh_colliders(sc):
    return [c for c in sc.collider_list if type(c).__name__ == "Triangle_Collider"]


# ---- the texel-boundary rule of the textured frames -------------------------------------------------
def _texel_index(tex, u, v):
    h, w = tex.img.shape[0], tex.img.shape[1]
    return (v * h * tex.repeat).astype(int) % h, (u * w * tex.repeat).astype(int) % w


def _nudge(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


def texel_boundary_pixels(sc, jit, ulps=8):
    """Pixels (bool, npix) where a sample's primary ray hits a textured triangle so close to a texel
    boundary that the texel index (texture.py:32-39 truncates) changes when u or v moves by +-`ulps`
    ulp: these may be left out of a frame comparison.  Needs the patched oracle."""
    npix = sc.camera.screen_width * sc.camera.screen_height
    out = np.zeros(npix, dtype=bool)
    for s in range(jit.shape[0]):
        Oa, Da = O.primary_rays(sc.camera, jit[s])
        near, ids = O.hit_ids(sc, Oa, Da)
        for ci in np.unique(ids[ids >= 0]):
            c = sc.collider_list[ci]
            tex = getattr(c.assigned_primitive.material, "diff_texture", None)
            if O._kind(c) != "Triangle_Collider" or getattr(c, "uvs", None) is None or not isinstance(tex, image):
                continue
            sel = ids == ci
            P = Oa[:, sel] + Da[:, sel] * near[sel]
            u, v = O.collider_uv(c, P)
            r0, c0 = _texel_index(tex, u, v)
            moved = np.zeros(u.shape, dtype=bool)
            for k in (-ulps, ulps):
                r1, _ = _texel_index(tex, u, _nudge(v, k))
                _, c1 = _texel_index(tex, _nudge(u, k), v)
                moved |= (r1 != r0) | (c1 != c0)
            out[np.flatnonzero(sel)[moved]] = True
    return out


# ---- the host check harness' k_collider_surface ------------------------------------------------------
def hostcheck_surface(collider, P, normal=True, uv=True):
    """Collider.get_Normal (3, n) and get_uv (2, n) at P (3, n) through the CPU build of the device
    functions (rt_hostcheck.cpp hc_collider_surface)."""
    import hostcheck as HC

    lib = HC.lib()
    lib.hc_collider_surface.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                        ctypes.c_void_p]
    rec = np.ascontiguousarray(collider_record(collider)).reshape(1)
    P = np.ascontiguousarray(P, dtype=np.float64)
    n = P.shape[1]
    Nout = np.empty((3, n)) if normal else None
    uvout = np.empty((2, n)) if uv else None
    rc = lib.hc_collider_surface(N.ptr(rec), N.ptr(P), n, N.ptr(Nout), N.ptr(uvout))
    if rc:
        raise RuntimeError(lib.hc_last_error().decode())
    return Nout, uvout
