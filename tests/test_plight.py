"""PositionalLight / SpotLight without a GPU: the Python classes, their lowering, and the shader
(rt_device.h shade_glossy under MAT_PLIGHT, compiled for the CPU by the host check harness) against
the numpy restatement of tests/plight_ref.py.  Hit ids exact, linear RGB within 1e-5 relative; no pixel
is left out of a comparison.  The device frames are in test_gpu_plight.py."""
import numpy as np
import pytest

import hostcheck as HC
import plight_ref as PR
import sightpy_oracle as O
from sightpy import Glossy, PointLight, PositionalLight, Scene, SpotLight, rgb, vec3
from sightpy import _hybrid, _native as N
from sightpy._lower import lower_scene

RTOL, ATOL = 1e-5, 1e-12


def _jitter(sc, spp, seed=5):
    np.random.seed(seed)
    return np.ascontiguousarray(sc.camera.draw_jitter(spp))


def _check(sc, spp, monkeypatch):
    """hostcheck.render of `sc` against the patched oracle; returns the restatement's records."""
    PR.patch(monkeypatch)
    jit = _jitter(sc, spp)
    (ref, ids, counts), rec = PR.recorded(lambda: O.render_linear(sc, jit))
    rgb_, _, hits, st = HC.render(sc, jit)
    assert np.array_equal(hits, ids)
    assert st["rays_per_depth"][:len(counts["depth"])] == [counts["depth"][d] for d in sorted(counts["depth"])]
    assert st["shadow_rays"] == counts["shadow"]  # one shadow test per light per Glossy hit
    np.testing.assert_allclose(rgb_, ref, rtol=RTOL, atol=ATOL)
    return rec, rgb_


# ---- 1. the Python classes and their lowering ---------------------------------------------------------
def _batch():
    rng = np.random.default_rng(2)
    M = rng.uniform(-2.0, 2.0, size=(3, 64))
    Nn = rng.normal(size=(3, 64))
    Nn /= np.sqrt((Nn * Nn).sum(0))
    return M, Nn


def test_positional_light_methods_on_a_batch():
    M, Nn = _batch()
    pos, col = np.array([0.3, 1.5, -0.7]), np.array([0.9, 0.8, 0.6])
    lt = PositionalLight(vec3(*pos), rgb(*col), intensity=7.0)
    d = pos[:, None] - M
    dist = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    L = d * (1.0 / dist)
    NdotL = np.maximum(Nn[0] * L[0] + Nn[1] * L[1] + Nn[2] * L[2], 0.0)
    Mv = vec3(*M)
    assert np.array_equal(lt.get_distance(Mv), dist)
    gl = lt.get_L(Mv)
    assert np.array_equal([gl.x, gl.y, gl.z], L)
    irr = lt.get_irradiance(dist, NdotL)
    assert np.array_equal([irr.x, irr.y, irr.z], col[:, None] * NdotL / dist ** 2.0 * 7.0)
    assert PositionalLight(vec3(0, 0, 0), rgb(1, 1, 1)).intensity == 100.0


def test_spot_light_methods_on_a_batch():
    M, Nn = _batch()
    pos, col, axis = np.array([0.3, 1.5, -0.7]), np.array([0.9, 0.8, 0.6]), np.array([0.2, -1.0, 0.1])
    lt = SpotLight(vec3(*pos), vec3(*axis), rgb(*col), 25.0, 50.0, intensity=3.0)
    a = axis * (1.0 / np.sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]))
    assert np.array_equal([lt.axis.x, lt.axis.y, lt.axis.z], a)
    ci, co = np.cos(np.radians(25.0)), np.cos(np.radians(50.0))
    assert (lt.cos_inner, lt.cos_outer) == (ci, co)
    Mv = vec3(*M)
    dist = lt.get_distance(Mv)
    Lv = lt.get_L(Mv)
    L = np.array([Lv.x, Lv.y, Lv.z])
    NdotL = np.maximum(Nn[0] * L[0] + Nn[1] * L[1] + Nn[2] * L[2], 0.0)
    mL = L * -1.0
    c = mL[0] * a[0] + mL[1] * a[1] + mL[2] * a[2]
    s = np.clip((c - co) / (ci - co), 0.0, 1.0)
    assert (s == 0.0).any() and (s == 1.0).any() and ((s > 0.0) & (s < 1.0)).any()
    irr = lt.get_irradiance(dist, NdotL, Lv)
    assert np.array_equal([irr.x, irr.y, irr.z], col[:, None] * NdotL / dist ** 2.0 * 3.0 * (s * s * (3.0 - 2.0 * s)))


@pytest.mark.parametrize("inner, outer", [(30.0, 30.0), (40.0, 30.0), (10.0, 95.0), (-5.0, 30.0)])
def test_spot_light_constructor_validates_the_cone(inner, outer):
    with pytest.raises(ValueError):
        SpotLight(vec3(0, 1, 0), vec3(0, -1, 0), rgb(1, 1, 1), inner, outer)


def test_spot_light_constructor_refuses_a_zero_direction():
    with pytest.raises(ValueError):
        SpotLight(vec3(0, 1, 0), vec3(0, 0, 0), rgb(1, 1, 1), 10.0, 20.0)
    SpotLight(vec3(0, 1, 0), vec3(0, -2, 0), rgb(1, 1, 1), 10.0, 90.0)  # outer_deg = 90 is allowed


def test_lowering_of_positional_and_spot_lights():
    sc = PR.room()
    L = lower_scene(sc)
    assert N.LIGHT_DTYPE.itemsize == 128 and N.LIGHT_POSITIONAL == 3 and N.ABI_VERSION == 7
    assert list(L.lights["type"]) == [N.LIGHT_DIRECTIONAL, N.LIGHT_POSITIONAL]
    # the records srt_upload_scene receives: Lowered keeps them as the common part and the extension rows
    assert L.lights.dtype == N.LIGHT_BASE_DTYPE and L.light_ext.shape == (2, N.LIGHT_EXT)
    table = L.light_table()
    assert table.dtype == N.LIGHT_DTYPE and len(table) == L.desc().n_lights == 2
    r = table[1]
    assert list(r["pos"]) == list(PR.LIGHT_POS) and list(r["color"]) == [0.9, 0.8, 0.6]
    assert r["intensity"] == 1.0 and r["flags"] == 0
    assert not L.light_local[1].any() and L.light_local[0].any()  # the cuboid's row of the directional light only
    sp = lower_scene(PR.spot_room()).light_table()[1]
    lt = PR.spot_room().Light_list[1]
    assert sp["type"] == N.LIGHT_POSITIONAL and sp["flags"] == N.LF_SPOT and sp["intensity"] == 4.0
    assert list(sp["axis"]) == [lt.axis.x, lt.axis.y, lt.axis.z]
    assert (sp["cos_inner"], sp["cos_outer"]) == (lt.cos_inner, lt.cos_outer)
    assert abs(np.dot(sp["axis"], sp["axis"]) - 1.0) < 1e-15


def test_scene_key_changes_when_the_light_moves():
    sc = PR.room()
    a = lower_scene(sc)
    assert a.signature() == lower_scene(sc).signature()
    sc.Light_list[1].pos = vec3(0.2, 0.0, -3.0)
    b = lower_scene(sc)
    assert b.signature() != a.signature()
    assert b.texel_key == a.texel_key and np.array_equal(b.colliders, a.colliders)  # the light table only
    sc.Light_list[1].intensity = 2.0
    assert lower_scene(sc).signature() != b.signature()
    sp = PR.spot_room()
    c = lower_scene(sp).signature()
    sp.Light_list[1].cos_outer = float(np.cos(np.radians(40.0)))
    assert lower_scene(sp).signature() != c


def test_point_light_still_raises_name_error():
    sc = Scene()
    sc.add_PointLight(vec3(0, 1, 0), rgb(1, 1, 1))
    lt = sc.Light_list[0]
    assert type(lt) is PointLight and not isinstance(lt, PositionalLight)
    with pytest.raises(NameError):
        lt.get_L()
    sc2 = PR.room()
    sc2.Light_list[1] = PointLight(vec3(*PR.LIGHT_POS), rgb(0.9, 0.8, 0.6))
    assert lower_scene(sc2).lights[1]["type"] == N.LIGHT_POINT
    with pytest.raises(RuntimeError, match="PointLight"):  # SRT_ERR_NAME at the first Glossy hit
        HC.render(sc2, _jitter(sc2, 1))


def test_subclass_overriding_a_method_is_a_user_light():
    class Flicker(PositionalLight):
        def get_L(self, M):
            return PositionalLight.get_L(self, M)

    class Plain(SpotLight):
        pass

    assert _hybrid.device_light(PositionalLight(vec3(0, 1, 0), rgb(1, 1, 1)))
    assert _hybrid.device_light(Plain(vec3(0, 1, 0), vec3(0, -1, 0), rgb(1, 1, 1), 10.0, 20.0))
    lt = Flicker(vec3(0, 1, 0), rgb(1, 1, 1))
    assert not _hybrid.device_light(lt)
    sc = PR.room()
    sc.Light_list[1] = lt
    with pytest.raises(NotImplementedError, match="per-ray light direction"):  # the per-ray refusal
        lower_scene(sc)


def test_positional_light_with_a_user_texture_is_refused():
    from sightpy import Sphere
    from sightpy.textures.texture import texture

    class Stripes(texture):
        def __init__(self):
            pass

        def get_color(self, hit):
            return rgb(0.5, 0.5, 0.5)

    mat = Glossy(diff_color=rgb(0.5, 0.5, 0.5), n=vec3(1.5 + 0j, 1.5 + 0j, 1.5 + 0j), roughness=0.2, spec_coeff=0.3,
                 diff_coeff=0.8)
    mat.diff_texture = Stripes()
    sc = PR.room(extra=Sphere(material=mat, center=vec3(0.1, 0.9, -2.0), radius=0.2, max_ray_depth=3))
    assert _hybrid.needs_inputs(sc)
    with pytest.raises(NotImplementedError, match="per-hit inputs"):
        lower_scene(sc)


def test_positional_light_with_a_smooth_mesh_is_refused(tmp_path):
    """No kernel variant holds both MAT_PLIGHT and the per-vertex triangle attributes; a flat mesh is fine."""
    import vattr_ref as VR
    from sightpy import TriangleMesh

    p = str(tmp_path / "tetra.obj")
    VR.write_tetrahedron_obj(p)
    _, blue, _ = PR._materials()
    smooth = TriangleMesh(p, center=vec3(0.1, 0.2, -2.6), material=blue, max_ray_depth=3, smooth=True)
    with pytest.raises(NotImplementedError, match="smooth or textured TriangleMesh"):
        lower_scene(PR.room(extra=smooth))
    flat = TriangleMesh(p, center=vec3(0.1, 0.2, -2.6), material=blue, max_ray_depth=3)
    lower_scene(PR.room(extra=flat))


# ---- 2. the room: lit, shadowed, and occluders beyond the light ----------------------------------------
def test_room_under_a_positional_light(monkeypatch):
    rec, _ = _check(PR.room(48, 36, 3), 2, monkeypatch)
    dist, near, see, ndl = (PR.cat(rec, k) for k in ("dist", "nearest", "seelight", "NdotL"))
    assert (see & (ndl > 0.0)).any()  # lit hits
    assert (near < dist).any() and not see[near < dist].any()  # shadowed hits
    beyond = (near < O.FARAWAY) & (near >= dist)
    assert beyond.any() and see[beyond].all()  # an occluder beyond the light does not shadow


# ---- 3. the spot light's cone edge on the floor -----------------------------------------------------
def test_room_under_a_spot_light(monkeypatch):
    rec, _ = _check(PR.spot_room(48, 36, 3), 2, monkeypatch)
    s = PR.cat(rec, "s")
    assert (s == 0.0).any() and (s == 1.0).any() and ((s > 0.0) & (s < 1.0)).any()


# ---- 4. a mesh that shadows the floor, through the BVH and the linear loop -----------------------------
@pytest.fixture(scope="module")
def split_tetra(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("plight") / "split_tetra.obj")
    assert PR.write_split_tetrahedron_obj(p) == 12
    return p


def test_mesh_shadows_the_floor_with_and_without_the_bvh(split_tetra, monkeypatch):
    sc = PR.mesh_room(split_tetra, 48, 36, 3)
    assert HC.bvh_nodes(sc) > 0
    tri = [i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Triangle_Collider"]
    assert len(tri) == 12
    try:
        HC.set_bvh(1)
        rec, with_bvh = _check(sc, 2, monkeypatch)
        HC.set_bvh(0)
        _, linear = _check(sc, 2, monkeypatch)
    finally:
        HC.set_bvh(1)
    assert np.array_equal(with_bvh, linear)
    # floor hits the mesh shadows: the nearest shadow caster of a shadowed floor hit is a mesh triangle
    jit = _jitter(sc, 2)
    floor = next(i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Plane_Collider")
    lt = sc.Light_list[1]
    shadowed = 0
    for s in range(2):
        Oa, Da = O.primary_rays(sc.camera, jit[s])
        near, ids = O.hit_ids(sc, Oa, Da)
        sel = ids == floor
        P = Oa[:, sel] + Da[:, sel] * near[sel]
        d = O.col3(lt.pos) - P
        dist = np.sqrt(O.dot(d, d))
        L = d * (1.0 / dist)
        tmesh = np.min([O.intersect(sc.collider_list[i], P + O.col3(vec3(0.0, 1e-6, 0.0)), L)[0] for i in tri], axis=0)
        shadowed += int((tmesh < dist).sum())
    assert shadowed > 10


# ---- 5. the 33rd light: past the seelight mask ----------------------------------------------------------
def test_positional_light_at_index_32(monkeypatch):
    sc = PR.many_lights_room(16, 12, 3)
    rec, _ = _check(sc, 1, monkeypatch)
    dist, near = PR.cat(rec, "dist"), PR.cat(rec, "nearest")
    assert (near < dist).any() and (near >= dist).any()


# ---- 6. irradiance beyond the fixed-point range ---------------------------------------------------------
def test_light_just_above_the_floor(monkeypatch):
    sc = PR.near_floor_room(_jitter(PR.room(16, 12, 3), 1), 16, 12, 3)
    rec, rgb_ = _check(sc, 1, monkeypatch)
    assert abs(PR.cat(rec, "dist").min() - 0.02) < 1e-6
    assert PR.cat(rec, "lv").max() >= 2.0 ** 17  # the irradiance itself is beyond the fixed-point range
    # ... and so is a pixel of the frame: |r| + |g| + |b| of a term at 2^17, or a pixel's magnitude at
    # 2^16, is what makes the device render the frame again with float64 sums
    assert rgb_.sum(axis=0).max() >= 2.0 ** 17
