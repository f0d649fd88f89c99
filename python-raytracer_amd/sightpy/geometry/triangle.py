"""Triangle primitive (reference `geometry/triangle.py:8-86`).

The reference `Triangle.__init__` passes `assigned_primitive=` to a collider whose constructor
takes `assigned_surface` (triangle.py:12 vs :20) and so raises TypeError; the collider works when
built directly.  Here both spellings are accepted so the primitive is usable; the collider's
intersection is the reference's (plane through the centroid + three edge half-spaces).
`get_uv` is undefined in the reference (uses unset pu/pv/w/h), so textured triangles are rejected
at scene lowering unless they carry their own texture coordinates.

Per-vertex attributes (this package's addition): `normals=(n1, n2, n3)` and
`uvs=((u1, v1), (u2, v2), (u3, v3))` are interpolated at the hit point P with the barycentric
weights b2 = dot(n31, P - p1) / dot(n31, p2 - p1), b3 = dot(n12, P - p2) / dot(n12, p3 - p2),
b1 = (1 - b2) - b3 (device: `triangle_bary` in csrc/rt_device.h).  The hit orientation, and so the
side the children start on, still comes from the geometric face.
"""
from .primitive import Primitive
from .collider import Collider

__all__ = ["Triangle", "Triangle_Collider"]


class Triangle(Primitive):
    def __init__(self, center, material, p1, p2, p3, max_ray_depth=5, shadow=True, normals=None, uvs=None):
        super().__init__(center, material, max_ray_depth, shadow=shadow)
        self.collider_list += [Triangle_Collider(assigned_primitive=self, p1=p1, p2=p2, p3=p3, normals=normals,
                                                 uvs=uvs)]


class Triangle_Collider(Collider):
    """Device: `rt_triangle_hit`."""

    def __init__(self, assigned_surface=None, p1=None, p2=None, p3=None, assigned_primitive=None, normals=None,
                 uvs=None):
        self.assigned_primitive = assigned_primitive if assigned_primitive is not None else assigned_surface
        self.p1 = p1
        self.p2 = p2
        self.p3 = p3
        self.normal = ((self.p2 - self.p1).cross(self.p3 - self.p1)).normalize()
        self.centroid = (self.p1 + self.p2 + self.p3) / 3
        self.center = self.centroid
        self.n31 = (self.p3 - self.p1).cross(self.normal)
        self.n12 = (self.p1 - self.p2).cross(self.normal)
        self.n23 = (self.p2 - self.p3).cross(self.normal)
        # per-vertex attributes: unit normals at p1, p2, p3 and (u, v) pairs, or None (the face normal,
        # no texture coordinates)
        if normals is not None:
            if len(normals) != 3:
                raise ValueError("normals: three vec3 values (n1, n2, n3)")
            normals = tuple(n.normalize() for n in normals)
        if uvs is not None:
            if len(uvs) != 3 or any(len(t) != 2 for t in uvs):
                raise ValueError("uvs: three (u, v) pairs")
            uvs = tuple((float(u), float(v)) for u, v in uvs)
        self.normals = normals
        self.uvs = uvs

    def bary_denominators(self):
        """(d2, d3) of the barycentric weights: dot(n31, p2 - p1), dot(n12, p3 - p2)."""
        return self.n31.dot(self.p2 - self.p1), self.n12.dot(self.p3 - self.p2)

    def rotate(self, M, center):
        self.p1 = center + (self.p1 - center).matmul(M)
        self.p2 = center + (self.p2 - center).matmul(M)
        self.p3 = center + (self.p3 - center).matmul(M)
        self.n31 = self.n31.matmul(M)
        self.n12 = self.n12.matmul(M)
        self.n23 = self.n23.matmul(M)
        self.normal = self.normal.matmul(M)
        if self.normals is not None:
            self.normals = tuple(n.matmul(M) for n in self.normals)
        self.centroid = center + (self.centroid - center).matmul(M)

    def get_uv(self, hit):
        if self.uvs is None:
            # triangle.py:79-83 reads pu/pv/w/h, which a Triangle_Collider never has
            raise NotImplementedError("Triangle uv is undefined in the reference (triangle.py:79-83)")
        return super().get_uv(hit)
