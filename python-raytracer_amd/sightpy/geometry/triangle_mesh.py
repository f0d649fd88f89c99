"""OBJ triangle mesh (reference `geometry/triangle_mesh.py:12-43`).

The reference constructor raises NameError (`colliders` undefined, :40), and its header notes the
missing bounding volume hierarchy (:7-9).  This version builds one `Triangle_Collider` per face
(vertex indices from 'f' records, 1-based, '/'-separated), which is what the reference intends.
On the device the Triangle colliders of a scene with 8 or more of them are intersected through a
BVH built when the scene is uploaded (csrc/rt_bvh.h, traversal `bvh_nearest` / `bvh_shadow` in
csrc/rt_device.h), with the same nearest / first-index / tie results as the linear loop over
`scene.collider_list`.

`smooth=True` shades with interpolated vertex normals: the file's `vn` records where all three
corners of a face name one (`v//vn`, `v/vt/vn`), else the area-weighted vertex normals (the
normalised sum of the unnormalised face cross products over the faces sharing the `v` index; the
face normal where that sum is zero).  `texcoords=True` gives every triangle the `vt` coordinates its
corners name (`v/vt`, `v/vt/vn`), so image textures can be applied; a face without them is a
ValueError.  With the defaults the `vn` / `vt` records and indices are ignored, as before.

`set_pose(R, t)` moves the mesh rigidly on the device (no reference counterpart): the collider records and the
BVH's boxes are recomputed there from a resident copy of the rest pose (srt_pose_colliders, csrc/rt_pose.h),
while the Python colliders below keep the rest pose.  `rotate()` still rewrites the Python colliders, which costs
a full lowering and upload of the mesh.

`set_vertices(P)` changes the mesh's shape on the device (no reference counterpart either): the mesh keeps the
file's `v` records and its faces' corner indices, and srt_deform_colliders (csrc/rt_deform.h) recomputes every
triangle's record, the area-weighted vertex normals of a smooth mesh and the BVH's boxes from the new positions,
24 bytes per vertex and frame.  The Python colliders keep the loaded shape here too.
"""
import numpy as np

from ..utils.vector3 import vec3
from .primitive import Primitive
from .triangle import Triangle_Collider

__all__ = ["TriangleMesh"]


def _corner(tok):
    """'v', 'v/vt', 'v//vn' or 'v/vt/vn' -> 0-based (v, vt or None, vn or None)."""
    parts = tok.split("/")
    vt = int(parts[1]) - 1 if len(parts) > 1 and parts[1] else None
    vn = int(parts[2]) - 1 if len(parts) > 2 and parts[2] else None
    return int(parts[0]) - 1, vt, vn


def _vertex_normals(verts, faces):
    """Area-weighted vertex normals in float64: per `v` index the sum, in file order, of the
    unnormalised cross products (p2 - p1) x (p3 - p1) of the faces that name it; unnormalised."""
    P = np.array([[v.x, v.y, v.z] for v in verts], dtype=np.float64).reshape(-1, 3)
    acc = np.zeros_like(P)
    for corners in faces:
        a, b, c = (k[0] for k in corners)
        n = np.cross(P[b] - P[a], P[c] - P[a])
        for i in (a, b, c):
            acc[i] += n
    return acc


class TriangleMesh(Primitive):
    def __init__(self, file_name, center, material, max_ray_depth=5, shadow=True, smooth=False, texcoords=False):
        super().__init__(center, material, max_ray_depth, shadow=shadow)
        verts, norms, texs, faces, records = [], [], [], [], []
        with open(file_name, "r") as f:
            for line in f.read().split("\n"):
                tok = line.split()
                if not tok:
                    continue
                if tok[0] == "v":
                    verts.append(vec3(float(tok[1]), float(tok[2]), float(tok[3])))
                elif tok[0] == "vn":
                    norms.append(vec3(float(tok[1]), float(tok[2]), float(tok[3])))
                elif tok[0] == "vt":
                    texs.append((float(tok[1]), float(tok[2])))
                elif tok[0] == "f":
                    faces.append([_corner(t) for t in tok[1:4]])
                    records.append(" ".join(tok))
        vnorm = _vertex_normals(verts, faces) if smooth else None
        recompute = []
        for k, corners in enumerate(faces):
            a, b, c = (v for v, _, _ in corners)
            p1, p2, p3 = verts[a] + center, verts[b] + center, verts[c] + center
            normals = uvs = None
            if smooth:
                if all(vn is not None and 0 <= vn < len(norms) for _, _, vn in corners):
                    normals = tuple(norms[vn] for _, _, vn in corners)
                    recompute.append((0, 0, 0))
                else:
                    recompute.append((1, 1, 1))
                    face_n = ((p2 - p1).cross(p3 - p1)).normalize()  # (Triangle_Collider.normal) for a zero sum
                    normals = tuple(vec3(*vnorm[i]) if np.any(vnorm[i] != 0.0) else face_n for i in (a, b, c))
            if texcoords:
                if not all(vt is not None and 0 <= vt < len(texs) for _, vt, _ in corners):
                    raise ValueError("%s: face %d ('%s') names no vt record on every corner (texcoords=True)"
                                     % (file_name, k + 1, records[k]))
                uvs = tuple(texs[vt] for _, vt, _ in corners)
            self.collider_list += [
                Triangle_Collider(assigned_primitive=self, p1=p1, p2=p2, p3=p3, normals=normals, uvs=uvs)
            ]
        # device posing (set_pose): the 12 numbers of the current pose or None, whether the mesh has ever been
        # posed, the lowered records of its colliders (filled by _lower.lower_scene), and a counter of
        # invalidate() calls (temporal motion: a mesh invalidated between two frames has no pose pair)
        self._pose = None
        self._device_posed = False
        self._record_cache = None
        self._epoch = 0
        # device deformation (set_vertices): the file's `v` records (n_v, 3) and the faces' corner indices
        # (n_f, 3), negative ones as the index Python's list indexing read; per corner whether its normal came
        # from _vertex_normals (and is recomputed on the device); the current vertex array or None (the loaded
        # shape); a counter of the arrays set; whether rotate() has turned the colliders away from the file's frame
        # (set_vertices is then refused)
        n_v = len(verts)
        self._file_verts = np.array([[v.x, v.y, v.z] for v in verts], dtype=np.float64).reshape(-1, 3)
        self._corners = np.array([[a if a >= 0 else a + n_v for a, _, _ in corners] for corners in faces],
                                 dtype=np.int32).reshape(-1, 3)
        self._recompute = (np.array(recompute, dtype=np.uint8).reshape(-1, 3) if smooth
                           else np.zeros((len(faces), 3), dtype=np.uint8))
        self._verts_cur = None
        self._vert_version = 0
        self._turned = False

    def set_pose(self, R, t=(0.0, 0.0, 0.0)):
        """Pose the mesh rigidly on the device: a point x_rest of the mesh as it was loaded (or last rotate()d,
        the rest pose) is rendered at R (x_rest - center) + center + t.  `R`: a 3 x 3 rotation (ValueError unless
        R R^T = I within 1e-9 and det R > 0), `t`: three numbers.  Poses are absolute, not cumulative.

        The Python colliders keep the rest pose: only the device's collider records and BVH boxes are
        recomputed (srt_pose_colliders), from R and T = center - R center + t, computed here once in float64.
        From the first call on the mesh is device-posed: the scene lowering takes its records from a cache
        kept on the mesh, so a frame in which only poses changed lowers, hashes, builds and uploads nothing
        for it.  Direct edits of a device-posed mesh's colliders (or of `center`) are therefore not seen until
        invalidate() is called; rotate() calls it.  Scenes with user Collider / Material / texture / Light
        subclasses and renders on several GPUs read the Python colliders and refuse a posed mesh
        (NotImplementedError)."""
        R = np.array(R, dtype=np.float64)
        t = np.array(t, dtype=np.float64).reshape(-1)
        if R.shape != (3, 3) or t.shape != (3,):
            raise ValueError("set_pose: R must be 3 x 3 and t three numbers, not %r and %r" % (R.shape, t.shape))
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError("set_pose: R and t must be finite")
        if np.abs(R @ R.T - np.eye(3)).max() > 1e-9 or np.linalg.det(R) <= 0.0:
            raise ValueError("set_pose: R is not a rotation (R R^T = I within 1e-9 and det R > 0)")
        c = np.array([self.center.x, self.center.y, self.center.z], dtype=np.float64)
        self._pose = np.concatenate([R.reshape(-1), c - R @ c + t])
        self._device_posed = True

    def reset_pose(self):
        """Back to the rest pose (the mesh stays device-posed: its records stay cached)."""
        self._pose = None

    @property
    def pose(self):
        """The 12 numbers handed to the device, R row-major then T, or None in the rest pose."""
        return None if self._pose is None else self._pose.copy()

    def invalidate(self):
        """Drop the cached records after the colliders were edited: the next lowering reads them again.  A
        deformation (set_vertices) is dropped with them: the next frame uploads the Python colliders."""
        self._record_cache = None
        self._epoch += 1
        if self._verts_cur is not None:
            self._verts_cur = None
            self._vert_version += 1

    def rotate(self, θ, u):
        super().rotate(θ, u)
        self.invalidate()
        self._turned = True

    # ---- deformation on the device ----
    @property
    def file_vertices(self):
        """(n_v, 3) float64: the file's `v` records (a copy)."""
        return self._file_verts.copy()

    @property
    def corners(self):
        """(n_f, 3) int32: the vertex index of every face's corners p1, p2, p3 (a copy)."""
        return self._corners.copy()

    def set_vertices(self, P):
        """Deform the mesh on the device: `P`, an (n_v, 3) array of finite float64 values (ValueError otherwise),
        gives every `v` record of the file a new position, in the file's frame and absolute (not cumulative).
        Vertex i is rendered at P[i] + center componentwise, as the constructor places verts[i] + center -- and
        under a pose at pose(P[i] + center): set_pose, reset_pose, set_vertices and reset_vertices can be called
        in any order.

        The device recomputes from `P` every field of each triangle's record exactly as Triangle_Collider computes
        it (srt_deform_colliders) and refits the BVH's boxes; its topology stays the loaded shape's, so a large
        deformation loosens it (rewrite the colliders and invalidate() to rebuild).  With `smooth=True` the corners
        whose normals the constructor took from the area-weighted vertex normals get them recomputed from `P`
        without center: per vertex the sum, in file order and once per corner naming it, of the unnormalised
        (P[b] - P[a]) x (P[c] - P[a]), normalised; the new face normal where the sum is exactly zero.  Corners of
        faces that took the file's `vn` records keep those normals, whatever the new shape.  Texture coordinates
        stay.

        The Python colliders keep the loaded shape, as under set_pose, and the mesh becomes device-posed: a frame
        in which only vertices changed lowers, hashes, builds and uploads nothing for it.  rotate() and
        invalidate() drop the deformation, and after rotate() the mesh refuses set_vertices (NotImplementedError):
        its colliders, and the `vn` normals among them, have left the file's frame that `P` is given in -- turn a
        deformed mesh with set_pose.  Scenes with user Collider / Material / texture / Light subclasses and renders
        on several GPUs refuse a deformed mesh (NotImplementedError)."""
        if self._turned:
            raise NotImplementedError("set_vertices after rotate(): the colliders have left the file's frame; "
                                      "turn a deformed mesh with set_pose")
        P = np.array(P, dtype=np.float64)
        if P.shape != self._file_verts.shape:
            raise ValueError("set_vertices: P must be %r, one row per `v` record of the file, not %r"
                             % (self._file_verts.shape, P.shape))
        if not np.isfinite(P).all():
            raise ValueError("set_vertices: P must be finite")
        self._verts_cur = np.ascontiguousarray(P)
        self._vert_version += 1
        self._device_posed = True

    def reset_vertices(self):
        """Back to the file's positions, through the device; nothing to do for a mesh that is not deformed."""
        if self._verts_cur is not None:
            self.set_vertices(self._file_verts)

    @property
    def vertices(self):
        """The (n_v, 3) array last given to set_vertices (a copy), or None in the loaded shape."""
        return None if self._verts_cur is None else self._verts_cur.copy()

    def deformed_vertices(self):
        """(n_f, 3, 3) float64: the vertices the device renders, P[corner] + center componentwise and then the
        pose's rule (posed_vertices); without a deformation, posed_vertices()."""
        if self._verts_cur is None:
            return self.posed_vertices()
        c = np.array([self.center.x, self.center.y, self.center.z], dtype=np.float64)
        return self._posed(self._verts_cur[self._corners] + c)

    def rest_vertices(self):
        """(n, 3, 3) float64: p1, p2, p3 of every triangle as the Python colliders hold them."""
        return np.array([[[p.x, p.y, p.z] for p in (c.p1, c.p2, c.p3)] for c in self.collider_list],
                        dtype=np.float64).reshape(-1, 3, 3)

    def posed_vertices(self):
        """(n, 3, 3) float64: the vertices the device renders, x'_k = ((R[k][0] x + R[k][1] y) + R[k][2] z)
        + T[k] in exactly this order (the rule of srt_pose_colliders); the rest vertices without a pose."""
        return self._posed(self.rest_vertices())

    def _posed(self, V):
        if self._pose is None:
            return V
        R, T = self._pose[:9].reshape(3, 3), self._pose[9:]
        x, y, z = V[..., 0], V[..., 1], V[..., 2]
        return np.stack([((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + T[k] for k in range(3)], axis=-1)
