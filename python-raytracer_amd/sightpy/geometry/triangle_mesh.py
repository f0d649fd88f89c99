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
        for k, corners in enumerate(faces):
            a, b, c = (v for v, _, _ in corners)
            p1, p2, p3 = verts[a] + center, verts[b] + center, verts[c] + center
            normals = uvs = None
            if smooth:
                if all(vn is not None and 0 <= vn < len(norms) for _, _, vn in corners):
                    normals = tuple(norms[vn] for _, _, vn in corners)
                else:
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
