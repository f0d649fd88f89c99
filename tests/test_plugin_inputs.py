"""User texture and Light subclasses on the CPU (reference plugin points textures/texture.py:14-16 and
lights.py:12-22, used at glossy.py:30,38-44): which textures and lights the device tables hold, that
a scene with a user one is rendered by the host-driven recursion, how it lowers (SRT_MF_HIT_ALBEDO,
SRT_LIGHT_USER), and what stays refused.  The device frames are in test_gpu_plugin_inputs.py."""
import numpy as np
import pytest

import plugin_scenes as PS
import scenes
import user_classes as U
from sightpy import _hybrid, _native as N, rgb, vec3
from sightpy._lower import lower_scene
from sightpy.lights import DirectionalLight, Light, PointLight
from sightpy.textures.texture import image, solid_color, texture


def test_device_texture_classifies():
    class Keeps(solid_color):
        pass

    class Overrides(solid_color):
        def get_color(self, hit):
            return self.color

    class KeepsImage(image):
        pass

    class OverridesImage(image):
        def get_color(self, hit):
            return super().get_color(hit)

    class Own(texture):
        def get_color(self, hit):
            return rgb(1.0, 0.0, 0.0)

    img = image("checkered_floor.png")
    assert _hybrid.device_texture(solid_color(rgb(1, 1, 1))) and _hybrid.device_texture(img)
    assert _hybrid.device_texture(Keeps(rgb(1, 1, 1)))
    keeps = KeepsImage.__new__(KeepsImage)
    over = OverridesImage.__new__(OverridesImage)
    assert _hybrid.device_texture(keeps) and not _hybrid.device_texture(over)
    assert not _hybrid.device_texture(Overrides(rgb(1, 1, 1)))
    assert not _hybrid.device_texture(Own())
    C = PS.classes()
    assert not _hybrid.device_texture(C.Bands(rgb(1, 1, 1), rgb(0, 0, 0)))


def test_device_light_classifies():
    class Keeps(DirectionalLight):
        pass

    class Dimmed(DirectionalLight):
        def get_irradiance(self, dist_light, NdotL):
            return self.color * NdotL * 0.5

    class Near(PointLight):
        def get_distance(self, M):
            return 1.0

    d = vec3(0.0, 1.0, 0.0)
    assert _hybrid.device_light(DirectionalLight(d, rgb(1, 1, 1)))
    assert _hybrid.device_light(PointLight(d, rgb(1, 1, 1)))
    assert _hybrid.device_light(Keeps(d, rgb(1, 1, 1)))
    assert not _hybrid.device_light(Dimmed(d, rgb(1, 1, 1)))
    assert not _hybrid.device_light(Near(d, rgb(1, 1, 1)))
    assert not _hybrid.device_light(Light(d, rgb(1, 1, 1)))
    assert not _hybrid.device_light(PS.falloff())
    assert not _hybrid.device_light(PS.classes().PlainDirectional(d, rgb(1, 1, 1)))


@pytest.mark.parametrize("kind", PS.KINDS)
def test_plugin_scenes_are_hybrid(kind):
    sc = PS.scene(kind, 16, 12)
    assert _hybrid.is_hybrid(sc)
    # the colliders and materials are all the device's: only the texture / the light is the user's
    assert all(_hybrid.on_device(c) for c in sc.collider_list)


def test_builtin_scene_is_not_hybrid():
    assert not _hybrid.is_hybrid(scenes.example1(16, 12))


def test_user_textures_lower_with_the_flag():
    sc = PS.scene("texture", 16, 12)
    L = lower_scene(sc)
    assert L.device_index == list(range(len(sc.collider_list)))
    mats = [L.materials[L.colliders["material"][i]] for i in range(len(sc.collider_list))]
    flagged = [bool(m["flags"] & N.MF_HIT_ALBEDO) for m in mats]
    # gold sphere (Bands), blue sphere (solid), lamp (Checker3D), floor (Checker3D), sky box sides
    assert flagged[:4] == [True, False, True, True] and not any(flagged[4:])
    assert [int(m["type"]) for m in mats[:4]] == [N.GLOSSY, N.GLOSSY, N.EMISSIVE, N.GLOSSY]
    for m in (mats[0], mats[2], mats[3]):
        assert m["tex"] == -1 and not m["p"][0:3].any()
    assert mats[0]["p"][3] == 0.8 and mats[3]["p"][3] == 0.9  # diff_coeff: applied on the device
    assert (L.lights["type"] == N.LIGHT_DIRECTIONAL).all()
    # the built-in scene's materials carry no such flag
    assert not (lower_scene(scenes.example1(16, 12)).materials["flags"] & N.MF_HIT_ALBEDO).any()


def test_user_light_lowers_with_its_direction():
    sc = PS.scene("light", 16, 12)
    L = lower_scene(sc)
    assert L.lights["type"].tolist() == [N.LIGHT_DIRECTIONAL, N.LIGHT_USER]
    Ld = sc.Light_list[1].get_L()
    assert L.lights["dir"][1].tolist() == [Ld.x, Ld.y, Ld.z]
    assert not L.lights["color"][1].any()
    assert not (L.materials["flags"] & N.MF_HIT_ALBEDO).any()


def test_user_light_local_rows_for_cuboids():
    from sightpy import Cuboid, Glossy
    from sightpy.geometry.cuboid import Cuboid_Collider

    sc = PS.scene("light", 16, 12)
    cb = Cuboid(material=Glossy(diff_color=rgb(0.5, 0.5, 0.5), roughness=0.2, spec_coeff=0.3, diff_coeff=0.8,
                                n=vec3(1.5, 1.5, 1.5)), center=vec3(0.0, 0.0, -2.0), width=0.4, height=0.4, length=0.4)
    cb.rotate(θ=30, u=vec3(0, 1, 0))
    sc.add(cb)
    L = lower_scene(sc)
    j = [i for i, c in enumerate(sc.collider_list) if isinstance(c, Cuboid_Collider) and c.assigned_primitive is cb][0]
    Ld = sc.Light_list[1].get_L().matmul(sc.collider_list[j].basis_matrix)
    assert L.light_local[1, j].tolist() == [float(Ld.x), float(Ld.y), float(Ld.z)]


def test_light_added_after_the_first_call_is_noticed():
    sc = scenes.example1(16, 12)
    assert not _hybrid.is_hybrid(sc)
    sc.Light_list += [PS.falloff()]
    assert _hybrid.is_hybrid(sc)
    assert lower_scene(sc).lights["type"].tolist() == [N.LIGHT_DIRECTIONAL, N.LIGHT_USER]
    sc.Light_list.pop()
    assert not _hybrid.is_hybrid(sc)


def test_per_ray_light_direction_is_refused():
    class Fan(Light):
        def get_L(self):
            return vec3(np.zeros(4), np.ones(4), np.zeros(4))

        def get_distance(self, M):
            return 1.0

        def get_irradiance(self, dist_light, NdotL):
            return self.color * NdotL

    sc = scenes.example1(16, 12)
    sc.Light_list += [Fan(vec3(0, 1, 0), rgb(1, 1, 1))]
    assert _hybrid.is_hybrid(sc)
    with pytest.raises(NotImplementedError, match="per-ray light direction"):
        lower_scene(sc)


def test_user_texture_on_a_triangle_lowers():
    from sightpy import Glossy
    from sightpy.geometry.triangle import Triangle

    C = PS.classes()
    sc = scenes.example1(16, 12)
    mat = Glossy(diff_color=C.Checker3D(rgb(1, 1, 1), rgb(0, 0, 0)), roughness=0.2, spec_coeff=0.3, diff_coeff=0.8,
                 n=vec3(1.5, 1.5, 1.5))
    sc.add(Triangle(center=vec3(0, 0, -2.0), material=mat, p1=vec3(-0.5, 0, -2.0), p2=vec3(0.5, 0, -2.0),
                    p3=vec3(0, 0.7, -2.0)))
    assert _hybrid.is_hybrid(sc)
    L = lower_scene(sc)
    assert L.materials["flags"][L.colliders["material"][-1]] & N.MF_HIT_ALBEDO


def test_both_refusals_remain():
    with pytest.raises(NotImplementedError, match="casts shadows"):
        _hybrid.is_hybrid(U.scene("collider_shadow"))
    from sightpy import Glossy

    sc = U.scene("collider")
    sc.collider_list[1].assigned_primitive.material = Glossy(diff_color=rgb(1, 1, 1), roughness=0.2, spec_coeff=0.3,
                                                             diff_coeff=0.8, n=vec3(1.5, 1.5, 1.5))
    sc._hybrid_key = None
    with pytest.raises(NotImplementedError, match="built-in material"):
        _hybrid.is_hybrid(sc)
    # ... and with a user texture or a user light in the same scene
    sc = U.scene("collider_shadow")
    sc.Light_list += [PS.falloff()]
    with pytest.raises(NotImplementedError, match="casts shadows"):
        _hybrid.is_hybrid(sc)
    sc = U.scene("collider")
    C = PS.classes()
    sc.collider_list[1].assigned_primitive.material = Glossy(diff_color=C.Checker3D(rgb(1, 1, 1), rgb(0, 0, 0)),
                                                             roughness=0.2, spec_coeff=0.3, diff_coeff=0.8,
                                                             n=vec3(1.5, 1.5, 1.5))
    with pytest.raises(NotImplementedError, match="built-in material"):
        _hybrid.is_hybrid(sc)
