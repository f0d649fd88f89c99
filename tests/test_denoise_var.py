"""The half-frame denoiser without a GPU: hc_denoise_var (srt_denoise_var's per-pixel functions of
csrc/rt_denoise.h compiled for the CPU, tests/denoise_var_host.py) against the restatement in
tests/denoise_var_ref.py on the shapes and levels of tests/test_denoise.py, what the variance buys on a
synthetic frame and on the cornell fixture, and Scene.render's new keys.  Floats within rtol 1e-5 / atol 1e-12."""
import numpy as np
import pytest

import denoise_host as DH
import denoise_ref as DR
import denoise_var_host as VH
import denoise_var_ref as VR
import scenes
from conftest import golden

from denoise_ref import LEVELS, SHAPES, close


# ---- a. both flags off: srt_denoise of the mean ------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_hostcheck_no_flags_equals_denoise_of_the_mean(shape, levels):
    W, H = shape
    A, B, guides, _ = VR.random_halves(W, H, 10 * W + H)
    got, _, u8 = VH.denoise_var(A, B, 2, 2, guides, W, H, levels=levels, **VR.SIGMAS)
    kw = {k: v for k, v in VR.SIGMAS.items() if k != "sigma_lum"}
    want, want_u8 = DH.denoise((A + B) / 2, guides, W, H, levels=levels, **kw)
    assert np.array_equal(got, want) and np.array_equal(u8, want_u8)
    # (unequal scaling of the halves: the mean as the definition writes it)
    got3, _, u83 = VH.denoise_var(A, B, 3, 3, guides, W, H, levels=levels, **VR.SIGMAS)
    want3, want3_u8 = DH.denoise(VR.mean_of_halves(A, B, 3, 3), guides, W, H, levels=levels, **kw)
    assert np.array_equal(got3, want3) and np.array_equal(u83, want3_u8)


# ---- b. the other three combinations against the restatement ----------------------------------------------
@pytest.mark.parametrize("mode", VR.MODES)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_hostcheck_modes_match_the_restatement(shape, levels, mode):
    W, H = shape
    variance, demodulate = mode
    A, B, guides, bg = VR.random_halves(W, H, 10 * W + H)
    got, var, _ = VH.denoise_var(A, B, 2, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels,
                                 **VR.SIGMAS)
    ref, ref_var = VR.denoise_var(A, B, 2, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels,
                                  **VR.SIGMAS)
    close(got, ref)
    c = VR.mean_of_halves(A, B, 2, 2)
    assert np.array_equal(got[:, bg], c[:, bg])  # background pixels: c itself
    if variance:
        close(var, ref_var)
        assert not var[bg].any() and (var >= 0.0).all()
    if W > 1 and levels > 0:
        assert np.abs(got - c).max() > 1e-3


# ---- c. unequal halves and awkward pixels ------------------------------------------------------------------
@pytest.mark.parametrize("mode", VR.MODES)
@pytest.mark.parametrize("levels", (0, 1, 3, 5))
def test_hostcheck_unequal_halves_and_awkward_pixels(levels, mode):
    W, H = 70, 9
    variance, demodulate = mode
    A, B, guides, bg, pix = VR.awkward_halves()
    got, var, _ = VH.denoise_var(A, B, 1, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels)
    ref, ref_var = VR.denoise_var(A, B, 1, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels)
    close(got, ref)
    c = VR.mean_of_halves(A, B, 1, 2)
    for p in (pix["inf"], pix["nan"]):  # copied through: c itself, not c / d * d
        assert np.array_equal(got[:, p], c[:, p], equal_nan=True) and not np.isfinite(c[:, p]).all()
    assert np.array_equal(got[:, bg], c[:, bg])
    others = np.ones(W * H, dtype=bool)
    others[[pix["inf"], pix["nan"]]] = False
    assert np.isfinite(got[:, others]).all()  # the zero albedo channel included (the 1e-3 clamp)
    if variance:
        close(var, ref_var)
        assert var[pix["inf"]] == 0.0 and var[pix["nan"]] == 0.0 and not var[bg].any()
        assert np.isfinite(var).all()


def test_hostcheck_zero_albedo_channel_is_clamped():
    """levels = 0 with demodulate: c / d * d, d = max(albedo, 1e-3): within two roundings of c and finite."""
    W, H = 70, 9
    A, B, guides, bg, pix = VR.awkward_halves()
    got, _, _ = VH.denoise_var(A, B, 1, 2, guides, W, H, demodulate=True, levels=0)
    c = VR.mean_of_halves(A, B, 1, 2)
    p = pix["zero"]
    assert np.isfinite(got[:, p]).all()
    np.testing.assert_allclose(got[:, p], c[:, p], rtol=4e-16)


# ---- d. adaptivity -------------------------------------------------------------------------------------------
def test_hostcheck_variance_spares_a_clean_step_and_filters_noise():
    VR.check_adaptivity(lambda A, B, g, W, H: VH.denoise_var(A, B, 1, 1, g, W, H, variance=True, levels=3)[0],
                        lambda c, g, W, H: DH.denoise(c, g, W, H)[0])


# ---- e. arguments ----------------------------------------------------------------------------------------------
BAD = [dict(ka=0), dict(kb=-1), dict(levels=9), dict(levels=-1), dict(sigma_normal=0.0), dict(sigma_albedo=-1.0),
       dict(sigma_plane=0.0), dict(variance=True, sigma_lum=0.0), dict(variance=False, sigma_color=0.0)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_hostcheck_refuses_bad_arguments(bad):
    A, B, guides, _ = VR.random_halves(5, 3, 1)
    kw = dict(bad)
    ka, kb = kw.pop("ka", 1), kw.pop("kb", 1)
    with pytest.raises(ValueError):
        VH.denoise_var(A, B, ka, kb, guides, 5, 3, **kw)


def test_hostcheck_a_sigma_not_in_use_may_be_anything():
    A, B, guides, _ = VR.random_halves(5, 3, 1)
    VH.denoise_var(A, B, 1, 1, guides, 5, 3, variance=True, sigma_color=0.0)
    VH.denoise_var(A, B, 1, 1, guides, 5, 3, variance=False, sigma_lum=-1.0)


def test_hostcheck_resolves_as_the_render_does():
    import sightpy_oracle as O

    W, H = 70, 9
    A, B, guides, _ = VR.random_halves(W, H, 4)
    got, _, u8 = VH.denoise_var(A, B, 2, 2, guides, W, H, variance=True, demodulate=True, levels=2)
    assert np.abs(u8.astype(int) - O.srgb_u8(got, H, W).astype(int)).max() <= 1
    _, _, u8x = VH.denoise_var(A, B, 2, 2, guides, W, H, variance=True, demodulate=True, levels=2, rgbx=True)
    assert np.array_equal(u8x[..., :3], u8) and (u8x[..., 3] == 255).all()


# ---- g. quality on the fixture -----------------------------------------------------------------------------
# E(filtered) / E(unfiltered mean of the halves) on the cornell fixture by the restatement, on the CPU, levels
# 2 / 3 / 4:   variance + demodulate, sigma_lum 1.0:  0.7031 / 0.7926 / 0.8300
#              srt_denoise's filter on the same mean:  0.5530 / 0.6913 / 0.8536
RATIO_LEVELS_3 = 0.792649567829418


def test_variance_mode_on_the_cornell_fixture():
    g, g0 = golden("denoise_var_cornell_64x64"), golden("denoise_cornell_64x64")
    W, H = int(g["width"]), int(g["height"])
    guides = DR.aovs(scenes.cornell(W, H))
    new, old = VR.fixture_error_ratios(g, g0, guides)
    print("E(filtered) / E(mean) by levels: variance + demodulate", new, "srt_denoise's filter", old)
    assert new[3] <= RATIO_LEVELS_3 * 1.05
    ka, kb = int(g["spp_a"]), int(g["spp_b"])
    host = VH.denoise_var(g["half_a"], g["half_b"], ka, kb, guides, W, H, variance=True, demodulate=True, levels=3)[0]
    e0 = DR.tonemapped_error(VR.mean_of_halves(g["half_a"], g["half_b"], ka, kb), g0["ref"])
    assert DR.tonemapped_error(host, g0["ref"]) / e0 <= RATIO_LEVELS_3 * 1.05


# ---- Scene.render's new keys -----------------------------------------------------------------------------------
def test_denoise_params_new_keys():
    from sightpy import _backend as B

    assert B.denoise_params({"levels": 2}) == dict(DR.DEFAULTS, levels=2)  # today's path: today's parameters
    assert B.denoise_params({"sigma_lum": 2.0}) == DR.DEFAULTS             # (neither flag on)
    assert B.denoise_params({"variance": False, "demodulate": False}) == DR.DEFAULTS
    assert B.denoise_params({"variance": True}) == dict(VR.DEFAULTS, variance=True, demodulate=False)
    assert B.denoise_params({"demodulate": True, "sigma_lum": 2, "levels": 3}) == dict(
        VR.DEFAULTS, variance=False, demodulate=True, sigma_lum=2.0, levels=3)


@pytest.mark.parametrize("spec", [{"variance": 1}, {"demodulate": "yes"}, {"variance": True, "sigma_lum": 0},
                                  {"variance": True, "nope": 1}, {"variance": True, "levels": 9}])
def test_render_refuses_bad_new_keys_before_any_launch(spec, monkeypatch):
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(2, denoise=spec)


@pytest.mark.parametrize("spec", [{"variance": True}, {"demodulate": True}])
def test_render_half_frames_need_two_samples(spec, monkeypatch):
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(1, denoise=spec)


def test_render_half_frames_refuse_several_gpus_and_hybrid_scenes(monkeypatch):
    import plugin_scenes
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(NotImplementedError):
        plugin_scenes.scene("texture", 16, 12).render(2, denoise={"variance": True})
    monkeypatch.setenv("SIGHTPY_DEVICES", "0,1")
    with pytest.raises(NotImplementedError):
        scenes.cornell(24, 24).render(2, denoise={"demodulate": True})
