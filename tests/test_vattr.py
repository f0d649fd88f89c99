"""Smooth-shaded, textured triangle meshes on the CPU: the OBJ loader's `vn` / `vt` records, the
lowered per-vertex attributes, and the kernels' interpolation (rt_device.h, compiled by g++ into the
host harness) against the numpy restatement in tests/vattr_ref.py and the oracle shading with it.
The GPU versions are in test_gpu_vattr.py."""
import numpy as np
import pytest

import hostcheck as HC
import scenes
import sightpy_oracle as O
import vattr_ref as VR
from sightpy import _native as N
from sightpy._lower import lower_scene, collider_record

RTOL, ATOL = 1e-5, 1e-12


def _a(v):
    return np.array([float(v.x), float(v.y), float(v.z)])


def _glossy():
    from sightpy import Glossy, rgb, vec3

    return Glossy(diff_color=rgb(0.5, 0.5, 0.5), roughness=0.2, spec_coeff=0.3, diff_coeff=0.8, n=vec3(1.5, 1.5, 1.5))


@pytest.fixture(scope="module")
def ico1(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vattr") / "ico1.obj")
    VR.write_smooth_icosphere_obj(p, 1)
    return p


@pytest.fixture(scope="module")
def tetra(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vattr") / "tetra.obj")
    VR.write_tetrahedron_obj(p, radius=0.7)
    return p


# ---- 1. loader ------------------------------------------------------------------------------------
FORMS_OBJ = """# a square pyramid: every face form
v 0 1 0
v -1 0 1
v 1 0 1
v 1 0 -1
v -1 0 -1
vn 0 1 0
vn -1 0.5 1
vn 1 0.5 1
vn 3 0 -4
vt 0.5 1.0
vt 0.0 0.0
vt 1.0 0.0
vt 0.25 0.75
f 1/1/1 2/2/2 3/3/3
f 1//1 3//3 4//4
f 1/1 4/3 5/4
f 1 5 2
"""


def test_loader_parses_vn_vt_and_every_face_form(tmp_path):
    from sightpy import TriangleMesh, vec3

    path = tmp_path / "forms.obj"
    path.write_text(FORMS_OBJ)
    V = np.array([[0, 1, 0], [-1, 0, 1], [1, 0, 1], [1, 0, -1], [-1, 0, -1]], dtype=np.float64)
    VN = np.array([[0, 1, 0], [-1, 0.5, 1], [1, 0.5, 1], [3, 0, -4]], dtype=np.float64)
    VT = [(0.5, 1.0), (0.0, 0.0), (1.0, 0.0), (0.25, 0.75)]
    F = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1)]
    m = TriangleMesh(str(path), center=vec3(0.0, 0.0, 0.0), material=_glossy(), smooth=True)
    assert len(m.collider_list) == 4 and all(c.uvs is None for c in m.collider_list)

    def unit(v):  # vec3.normalize
        return v * (1.0 / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))

    # the faces whose corners all name a vn record: those normals, normalised
    for c, idx in zip(m.collider_list[:2], [(0, 1, 2), (0, 2, 3)]):
        for n, k in zip(c.normals, idx):
            assert np.array_equal(_a(n), unit(VN[k]))
    # v/vt and v: the area-weighted vertex normals, summed over the faces in file order
    acc = np.zeros((5, 3))
    for a, b, c in F:
        n = np.cross(V[b] - V[a], V[c] - V[a])
        for i in (a, b, c):
            acc[i] += n
    for c, idx in zip(m.collider_list[2:], F[2:]):
        for n, k in zip(c.normals, idx):
            assert np.array_equal(_a(n), unit(acc[k]))
    # texcoords: only on the faces that name them
    with pytest.raises(ValueError, match="face 2"):
        TriangleMesh(str(path), center=vec3(0.0, 0.0, 0.0), material=_glossy(), texcoords=True)
    two = tmp_path / "two.obj"
    two.write_text("\n".join(l for l in FORMS_OBJ.split("\n") if not l.startswith("f ") or "//" not in l and l != "f 1 5 2"))
    m = TriangleMesh(str(two), center=vec3(0.0, 0.0, 0.0), material=_glossy(), texcoords=True)
    assert [c.uvs for c in m.collider_list] == [(VT[0], VT[1], VT[2]), (VT[0], VT[2], VT[3])]
    assert all(c.normals is None for c in m.collider_list)
    # a vertex whose face cross products cancel takes the face normal
    flat = tmp_path / "cancel.obj"
    flat.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 3 2\n")
    m = TriangleMesh(str(flat), center=vec3(0.0, 0.0, 0.0), material=_glossy(), smooth=True)
    for c in m.collider_list:
        for n in c.normals:
            assert np.array_equal(_a(n), _a(c.normal))


def test_default_mesh_lowers_as_before(tmp_path):
    """smooth / texcoords default to off: the lowered collider table of scenes.mesh_scene equals the one
    with both spelled out, no record carries a flag or a value in the attribute slots."""
    path = str(tmp_path / "ico.obj")
    scenes.write_icosphere_obj(path, subdiv=1)
    a = lower_scene(scenes.mesh_scene(path)).colliders
    b = lower_scene(VR.mesh_scene(path, smooth=False, texcoords=False)).colliders
    assert np.array_equal(a, b)
    tri = a[a["type"] == N.TRIANGLE]
    assert len(tri) == 80 and not np.any(tri["flags"] & (N.CF_VNORMAL | N.CF_VUV)) and not np.any(tri["p"][:, 24:])
    s = lower_scene(VR.mesh_scene(path, smooth=True)).colliders
    assert np.all(s[s["type"] == N.TRIANGLE]["flags"] & N.CF_VNORMAL)
    assert np.array_equal(s["p"][:, :24], a["p"][:, :24])


def test_triangle_keywords_and_get_uv_refusal():
    from sightpy import Triangle, vec3
    from sightpy.ray import Hit

    p = (vec3(0.0, 0.0, 0.0), vec3(1.0, 0.0, 0.0), vec3(0.0, 1.0, 0.0))
    plain = Triangle(vec3(0.0, 0.0, 0.0), _glossy(), *p)
    assert plain.collider_list[0].normals is None and plain.collider_list[0].uvs is None
    with pytest.raises(NotImplementedError):
        plain.collider_list[0].get_uv(Hit(1.0, 1.0, None, plain.collider_list[0], plain))
    t = Triangle(vec3(0.0, 0.0, 0.0), _glossy(), *p, normals=(vec3(0.0, 0.0, 2.0), vec3(1.0, 0.0, 1.0), vec3(0.0, 3.0, 0.0)),
                 uvs=((0, 0), (1, 0), (0, 1)))
    c = t.collider_list[0]
    assert np.array_equal(_a(c.normals[0]), [0.0, 0.0, 1.0]) and np.array_equal(_a(c.normals[2]), [0.0, 1.0, 0.0])
    rec = collider_record(c)
    assert int(rec["flags"]) == N.CF_VNORMAL | N.CF_VUV
    assert np.array_equal(rec["p"][33:39], [0, 0, 1, 0, 0, 1])
    assert rec["p"][39] == c.n31.dot(c.p2 - c.p1) and rec["p"][40] == c.n12.dot(c.p3 - c.p2)


# ---- 2. rotation ----------------------------------------------------------------------------------
def test_rotate_turns_the_vertex_normals(ico1):
    from sightpy import TriangleMesh, vec3
    from sightpy.geometry.primitive import rotation_matrix

    m = TriangleMesh(ico1, center=vec3(0.2, 0.0, -1.0), material=_glossy(), smooth=True)
    before = [[n for n in c.normals] for c in m.collider_list]
    m.rotate(θ=35, u=vec3(0.3, 1.0, 0.2))
    M = rotation_matrix(35, vec3(0.3, 1.0, 0.2))
    for c, ns in zip(m.collider_list, before):
        p = collider_record(c)["p"]
        assert np.array_equal(p[24:33], np.concatenate([_a(n.matmul(M)) for n in ns]))
        assert np.array_equal(p[3:6], _a(c.normal))
        assert p[39] == c.n31.dot(c.p2 - c.p1)
    # the rotated mesh is still a sphere: the rotated normals are the unit vertex positions
    c = m.collider_list[5]
    np.testing.assert_allclose(_a(c.normals[0]), _a(c.p1 - m.center) / 0.5, rtol=0, atol=1e-14)


# ---- 3. what the interpolation buys -------------------------------------------------------------------
def _ring(center, n=512, radius=3.0):
    """n rays from a tilted circle around `center`, each aimed at it."""
    a = (np.arange(n) + 0.25) * (2 * np.pi / n)
    e1 = np.array([1.0, 0.2, 0.1]) / np.linalg.norm([1.0, 0.2, 0.1])
    e2 = np.cross(e1, [0.3, 1.0, -0.4])
    e2 /= np.linalg.norm(e2)
    Oa = center[:, None] + radius * (e1[:, None] * np.cos(a) + e2[:, None] * np.sin(a))
    Da = center[:, None] - Oa
    return np.ascontiguousarray(Oa), np.ascontiguousarray(Da / np.linalg.norm(Da, axis=0))


def _angles(Nn, T):
    return np.degrees(np.arccos(np.clip(O.dot(Nn, T), -1.0, 1.0)))


def test_icosphere_interpolated_normals_are_closer_to_the_sphere(tmp_path):
    """320-face icosphere (subdivision 2, vn = the unit vertex positions), a ring of 512 rays through
    its centre: the device functions' normals equal the numpy restatement bit for bit, and their
    largest angle to the true sphere normal is under half the face normals' largest.

    Measured with the numpy restatement: flat max 10.07 deg (mean 4.81), smooth max 1.5e-6 deg (mean
    2.5e-7), ratio 1.5e-7; the smooth normal is closer than the face normal at 512 of 512 hits.  (With
    vn = the unit vertex positions the interpolated sum is (P - centre) / radius, the sphere's own normal
    direction at the facet point, so what is left is rounding and the arccos near 1.)"""
    path = str(tmp_path / "ico2.obj")
    VR.write_smooth_icosphere_obj(path, 2)
    center = np.array([0.35, 0.05, -1.0])
    from sightpy import Scene, TriangleMesh, vec3

    sc = Scene()  # the mesh alone: every ray of the ring meets it first
    sc.add(TriangleMesh(path, center=vec3(*center), material=_glossy(), smooth=True))
    Oa, Da = _ring(center)
    t, ids, _ = HC.nearest(sc, Oa, Da)
    near, ref_ids = O.hit_ids(sc, Oa, Da)
    assert np.array_equal(ids, ref_ids) and np.array_equal(t, near)
    tri = np.array([type(sc.collider_list[i]).__name__ == "Triangle_Collider" for i in ids])
    assert tri.all()
    P = Oa + Da * t
    true = (P - center[:, None]) / np.linalg.norm(P - center[:, None], axis=0)
    smooth, flat = np.empty((3, 512)), np.empty((3, 512))
    for ci in np.unique(ids):
        c, sel = sc.collider_list[ci], ids == ci
        want = VR.interp_normal(c, P[:, sel])
        got, _ = VR.hostcheck_surface(c, P[:, sel], uv=False)
        assert np.array_equal(got, want)
        smooth[:, sel] = want
        flat[:, sel] = O.col3(c.normal)
    a_s, a_f = _angles(smooth, true), _angles(flat, true)
    print("flat max %.4g mean %.4g  smooth max %.3g mean %.3g  ratio %.3g  closer at %d of %d" % (
        a_f.max(), a_f.mean(), a_s.max(), a_s.mean(), a_s.max() / a_f.max(), (a_s < a_f).sum(), len(a_s)))
    assert np.all(a_s < a_f)
    assert a_s.max() < 0.5 * a_f.max()


# ---- 4. frames: oracle against the host check ---------------------------------------------------------
def _frames(sc, jit):
    """hostcheck frames with and without the BVH, the same bit for bit"""
    out = []
    for on in (0, 1):
        HC.set_bvh(on)
        try:
            out.append(HC.render(sc, jit))
        finally:
            HC.set_bvh(1)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    return out[1]


@pytest.mark.parametrize("mesh", ["ico1", "tetra"])
def test_smooth_frames_match_the_patched_oracle(mesh, ico1, tetra, monkeypatch):
    """64x48, depth 3, 2 spp: the 80-face icosphere (through the BVH) and the four-triangle
    tetrahedron (the linear triangle loop), each with set_bvh(0) and set_bvh(1)."""
    VR.patch(monkeypatch)
    sc = VR.mesh_scene(ico1 if mesh == "ico1" else tetra, 64, 48, 3, smooth=True)
    assert (HC.bvh_nodes(sc) > 0) == (mesh == "ico1")
    np.random.seed(5)
    jit = sc.camera.draw_jitter(2)
    rgb, u8, hits, st = _frames(sc, jit)
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(hits, ids)
    assert st["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    np.testing.assert_allclose(rgb, ref, rtol=RTOL, atol=ATOL)
    on_mesh = np.isin(hits, [i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Triangle_Collider"])
    assert on_mesh.mean() > 0.02
    # and the smooth frame is not the flat one
    flat = HC.render(VR.mesh_scene(ico1 if mesh == "ico1" else tetra, 64, 48, 3, smooth=False), jit)[0]
    assert not np.allclose(flat, rgb, rtol=1e-3, atol=1e-6)


# ---- 5. textured mesh -----------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["ico1", "tetra"])
def test_textured_frames_match_the_patched_oracle(mesh, ico1, tetra, monkeypatch):
    """As the smooth frames, with texcoords=True and a Glossy whose diff_color is the checkered image
    (repeat 4) over the vertices' spherical coordinates.  A pixel whose primary hit lies within 8 ulp
    of a texel boundary (texel selection truncates) may be left out, at most 0.5 % of them.

    Measured: the rule leaves out 0 of 3072 pixels in either scene (0.0 %)."""
    VR.patch(monkeypatch)
    sc = VR.mesh_scene(ico1 if mesh == "ico1" else tetra, 64, 48, 3, smooth=True, texcoords=True, material=VR.checker())
    np.random.seed(5)
    jit = sc.camera.draw_jitter(2)
    skip = VR.texel_boundary_pixels(sc, jit)
    print("texel-boundary pixels: %d of %d (%.3f %%)" % (skip.sum(), skip.size, 100.0 * skip.mean()))
    assert skip.mean() <= 0.005
    rgb, u8, hits, st = _frames(sc, jit)
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(hits, ids)
    np.testing.assert_allclose(rgb[:, ~skip], ref[:, ~skip], rtol=RTOL, atol=ATOL)
    plain = HC.render(VR.mesh_scene(ico1 if mesh == "ico1" else tetra, 64, 48, 3, smooth=True), jit)[0]
    assert not np.allclose(plain, rgb, rtol=1e-3, atol=1e-6)


def test_uv_of_flagged_triangles_through_the_device_functions(ico1):
    sc = VR.mesh_scene(ico1, smooth=True, texcoords=True, material=VR.checker())
    rng = np.random.default_rng(3)
    for c in VR.mesh_colliders(sc)[::9]:
        w = rng.dirichlet([1.0, 1.0, 1.0], size=64).T
        w[:, :3] = np.eye(3)  # the vertices themselves
        P = O.col3(c.p1) * w[0] + O.col3(c.p2) * w[1] + O.col3(c.p3) * w[2]
        Nn, uv = VR.hostcheck_surface(c, P)
        assert np.array_equal(Nn, VR.interp_normal(c, P))
        u, v = VR.interp_uv(c, P)
        assert np.array_equal(uv[0], u) and np.array_equal(uv[1], v)
        np.testing.assert_allclose(uv[:, :3], np.array(c.uvs).T, rtol=0, atol=1e-14)
    flat = VR.mesh_colliders(VR.mesh_scene(ico1, smooth=False))[0]
    with pytest.raises(RuntimeError, match="uv is undefined"):
        VR.hostcheck_surface(flat, np.zeros((3, 1)))


def test_lowering_refusals_that_stay(ico1):
    """A normal map on a triangle (no inverse_basis_matrix) and a thin film stay refused with texture
    coordinates too; an image texture on a triangle without them stays refused."""
    from sightpy import ThinFilmInterference

    nm = VR.checker()
    nm.set_normalmap("floor.jpg", repeat=4.0)
    with pytest.raises(NotImplementedError):
        lower_scene(VR.mesh_scene(ico1, smooth=True, texcoords=True, material=nm))
    with pytest.raises(NotImplementedError):
        lower_scene(VR.mesh_scene(ico1, smooth=True, texcoords=True, material=ThinFilmInterference(thickness=330, noise=60.0)))
    with pytest.raises(NotImplementedError):
        lower_scene(VR.mesh_scene(ico1, smooth=True, texcoords=False, material=VR.checker()))
    lower_scene(VR.mesh_scene(ico1, smooth=False, texcoords=True, material=VR.checker()))
