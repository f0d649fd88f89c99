"""The denoiser without a GPU: the per-pixel functions of csrc/rt_denoise.h (compiled for the CPU,
tests/denoise_host.py) against the restatement in tests/denoise_ref.py -- the first-hit guide images on
four scenes, the a-trous filter for levels 0..5 on the cornell fixture and on small random frames --,
what the filter buys on the fixture, and Scene.render's argument checks.  Hit ids exact, floats within
rtol 1e-5 / atol 1e-12."""
import numpy as np
import pytest

import denoise_host as DH
import denoise_ref as DR
import scenes
import vattr_ref as VR
from conftest import golden

from denoise_ref import LEVELS, SHAPES, close, random_frame, same_aovs


# ---- 1. first-hit guide images ------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("example1", (64, 48)), ("cornell", (24, 24)), ("features", (48, 36))])
def test_hostcheck_aovs_match_the_restatement(name, size):
    sc = getattr(scenes, name)(*size)
    ref = DR.aovs(sc)
    got = DH.aovs(sc)
    same_aovs(got, ref)
    kinds = {type(sc.collider_list[i].assigned_primitive.material).__name__ for i in np.unique(ref["hit_id"]) if i >= 0}
    want = {"example1": {"Glossy", "SkyBox_Material"}, "cornell": {"Diffuse", "Refractive"},
            "features": {"Glossy", "Refractive", "Emissive", "SkyBox_Material"}}[name]
    assert want <= kinds, kinds  # the frame shows what the case is about
    if name == "cornell":  # (its rotated cuboid too)
        assert any(type(sc.collider_list[i]).__name__ == "Cuboid_Collider" for i in np.unique(ref["hit_id"]))


def test_hostcheck_aovs_ignore_the_normal_map():
    """features' floor is normal-mapped: the guide holds the plane's own normal there."""
    sc = scenes.features(48, 36)
    got = DH.aovs(sc)
    floor = next(i for i, c in enumerate(sc.collider_list)
                 if getattr(c.assigned_primitive.material, "normalmap", None) is not None)
    sel = got["hit_id"] == floor
    assert sel.sum() > 100
    n = sc.collider_list[floor].normal
    assert np.array_equal(np.abs(got["normal"][:, sel]), np.abs(np.array([[n.x], [n.y], [n.z]]) * np.ones(sel.sum())))


def test_hostcheck_aovs_smooth_textured_mesh_through_the_bvh(tmp_path, monkeypatch):
    import hostcheck as HC

    p = str(tmp_path / "ico1.obj")
    VR.write_smooth_icosphere_obj(p, 1)
    sc = VR.mesh_scene(p, 64, 48, 3, smooth=True, texcoords=True, material=VR.checker())
    assert HC.bvh_nodes(sc) > 0
    VR.patch(monkeypatch)
    ref = DR.aovs(sc)
    got = DH.aovs(sc)
    j = np.stack([np.full(64 * 48, 0.5), np.full(64 * 48, 0.5), np.zeros(64 * 48), np.zeros(64 * 48)])[None]
    same_aovs(got, ref, skip=VR.texel_boundary_pixels(sc, j))
    tri = np.array([type(sc.collider_list[i]).__name__ == "Triangle_Collider" if i >= 0 else False for i in ref["hit_id"]])
    assert tri.sum() > 50
    # interpolated normals: not the face normals, and textured albedo: more than one colour
    face = np.array([[sc.collider_list[i].normal.x, sc.collider_list[i].normal.y, sc.collider_list[i].normal.z]
                     for i in ref["hit_id"][tri]]).T
    assert np.abs(np.abs(got["normal"][:, tri]) - np.abs(face)).max() > 1e-3
    assert len(np.unique(got["albedo"][:, tri], axis=1).T) > 1


# ---- 2. the filter --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    g = golden("denoise_cornell_64x64")
    W, H = int(g["width"]), int(g["height"])
    return {"noisy": g["noisy"], "ref": g["ref"], "W": W, "H": H, "guides": DR.aovs(scenes.cornell(W, H))}


@pytest.fixture(scope="module")
def fixture_filtered(fixture):
    """The restatement's result per level on the fixture, computed once."""
    return {l: DR.atrous(fixture["noisy"], fixture["guides"], fixture["W"], fixture["H"], levels=l) for l in LEVELS}


@pytest.mark.parametrize("levels", LEVELS)
def test_hostcheck_denoise_matches_the_restatement_on_the_fixture(fixture, fixture_filtered, levels):
    got, _ = DH.denoise(fixture["noisy"], fixture["guides"], fixture["W"], fixture["H"], levels=levels)
    close(got, fixture_filtered[levels])
    if levels == 0:
        assert np.array_equal(got, fixture["noisy"])
    else:
        assert np.abs(got - fixture["noisy"]).max() > 1e-3


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_hostcheck_denoise_matches_the_restatement_on_random_frames(shape, levels):
    W, H = shape
    rgb, guides, bg = random_frame(W, H, 10 * W + H)
    got, _ = DH.denoise(rgb, guides, W, H, levels=levels, sigma_color=0.6, sigma_normal=0.3, sigma_albedo=0.2,
                        sigma_plane=0.05)
    ref = DR.atrous(rgb, guides, W, H, levels=levels, sigma_color=0.6, sigma_normal=0.3, sigma_albedo=0.2,
                    sigma_plane=0.05)
    close(got, ref)
    assert np.array_equal(got[:, bg], rgb[:, bg])  # background pixels pass through
    if W > 1 and levels > 0:
        assert np.abs(got - rgb).max() > 1e-3


@pytest.mark.parametrize("levels", LEVELS)
def test_hostcheck_denoise_non_finite_pixels(levels):
    W, H = 70, 9
    rgb, guides, bg = random_frame(W, H, 3)
    a, b = 2 * W + 5, 6 * W + 66
    assert not bg[a] and not bg[b]
    rgb[1, a] = np.inf
    rgb[2, b] = np.nan
    got, _ = DH.denoise(rgb, guides, W, H, levels=levels)
    close(got, DR.atrous(rgb, guides, W, H, levels=levels))
    for p in (a, b):
        assert np.array_equal(got[:, p], rgb[:, p], equal_nan=True)
    others = np.ones(W * H, dtype=bool)
    others[[a, b]] = False
    assert np.isfinite(got[:, others]).all()


def test_hostcheck_denoise_resolves_as_the_render_does(fixture):
    import sightpy_oracle as O

    W, H = fixture["W"], fixture["H"]
    got, u8 = DH.denoise(fixture["noisy"], fixture["guides"], W, H, levels=2)
    want = O.srgb_u8(got, H, W)
    assert np.abs(u8.astype(int) - want.astype(int)).max() <= 1
    _, u8x = DH.denoise(fixture["noisy"], fixture["guides"], W, H, levels=2, rgbx=True)
    assert np.array_equal(u8x[..., :3], u8) and (u8x[..., 3] == 255).all()


@pytest.mark.parametrize("bad", [{"levels": 9}, {"levels": -1}, {"sigma_color": 0.0}, {"sigma_plane": -1.0}])
def test_hostcheck_denoise_refuses_bad_arguments(bad):
    rgb, guides, _ = random_frame(5, 3, 1)
    with pytest.raises(ValueError):
        DH.denoise(rgb, guides, 5, 3, **bad)


def test_filter_reduces_the_error_of_the_noisy_fixture(fixture):
    """E(a) = mean((f(a) - f(ref))^2), f(x) = x / (1 + x): with levels = 3 and the default sigmas the
    filtered 2-sample frame is at most 0.75 of the unfiltered frame's error against the 64-sample frame
    (which itself carries 1/32 of the noisy frame's variance)."""
    W, H = fixture["W"], fixture["H"]
    e0 = DR.tonemapped_error(fixture["noisy"], fixture["ref"])
    ratios = {}
    for levels in (2, 3, 4):
        ratios[levels] = DR.tonemapped_error(DR.atrous(fixture["noisy"], fixture["guides"], W, H, levels=levels),
                                             fixture["ref"]) / e0
    print("E(filtered) / E(noisy) by levels:", ratios)
    assert ratios[3] <= 0.75
    host = DR.tonemapped_error(DH.denoise(fixture["noisy"], fixture["guides"], W, H, levels=3)[0], fixture["ref"]) / e0
    assert host <= 0.75


# ---- 3. Scene.render's argument -------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [{"levels": 9}, {"nope": 1}, {"levels": 2.5}, {"sigma_color": 0}, "yes"])
def test_render_refuses_a_bad_denoise_argument_before_any_launch(spec, monkeypatch):
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(2, denoise=spec)


def test_denoise_params_defaults_and_overrides():
    from sightpy import _backend as B

    assert B.denoise_params(False) is None and B.denoise_params(None) is None
    assert B.denoise_params(True) == DR.DEFAULTS
    assert B.denoise_params({"levels": 2, "sigma_plane": 0.5}) == dict(DR.DEFAULTS, levels=2, sigma_plane=0.5)


def test_hybrid_scene_refuses_denoise_and_aovs(monkeypatch):
    import plugin_scenes
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    sc = plugin_scenes.scene("texture", 16, 12)
    with pytest.raises(NotImplementedError):
        sc.render(1, denoise=True)
    with pytest.raises(NotImplementedError):
        sc.get_aovs()
