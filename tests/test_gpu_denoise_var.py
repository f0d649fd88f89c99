"""The half-frame denoiser on the device: srt_denoise_var (k_dn_prepare, k_atrous<true>, k_dn_finish) against
the restatement in tests/denoise_var_ref.py on the shapes of tests/test_denoise_var.py, its arguments and
pointers, and Scene.render(denoise={"variance": ..., "demodulate": ...}) end to end.  Floats within rtol 1e-5 /
atol 1e-12."""
import ctypes

import numpy as np
import pytest

import denoise_ref as DR
import denoise_var_host as VH
import denoise_var_ref as VR
import scenes
import sightpy_oracle as O
from conftest import golden
from denoise_ref import LEVELS, SHAPES, close

pytestmark = pytest.mark.gpu


def _backend():
    from sightpy import _backend

    return _backend


def _report(what, got, ref):
    """The largest deviation from the restatement, for the record (-s shows it)."""
    sel = np.isfinite(ref) & (ref != 0.0)
    if sel.any():
        d = np.abs(got[sel] - ref[sel])
        print("deviation", what, "rel %.3g abs %.3g" % (float((d / np.abs(ref[sel])).max()), float(d.max())))


# ---- a. both flags off: srt_denoise of the mean ------------------------------------------------------------
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_no_flags_equals_denoise_of_the_mean(shape, levels):
    B = _backend()
    W, H = shape
    A, Bh, guides, _ = VR.random_halves(W, H, 10 * W + H)
    got, _, u8 = B.denoise_var(A, Bh, 2, 2, guides, W, H, levels=levels, **VR.SIGMAS)
    kw = {k: v for k, v in VR.SIGMAS.items() if k != "sigma_lum"}
    want, want_u8 = B.denoise((A + Bh) / 2, guides, W, H, levels=levels, **kw)
    assert np.array_equal(got, want) and np.array_equal(u8, want_u8)


# ---- b. the other three combinations against the restatement ----------------------------------------------
@pytest.mark.parametrize("mode", VR.MODES)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_modes_match_the_restatement(shape, levels, mode):
    B = _backend()
    W, H = shape
    variance, demodulate = mode
    A, Bh, guides, bg = VR.random_halves(W, H, 10 * W + H)
    ms = []
    got, var, u8 = B.denoise_var(A, Bh, 2, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels,
                                 want_variance=variance, timings=ms, **VR.SIGMAS)
    ref, ref_var = VR.denoise_var(A, Bh, 2, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels,
                                  **VR.SIGMAS)
    close(got, ref)
    _report("rgb %dx%d levels %d mode %s" % (W, H, levels, mode), got, ref)
    c = VR.mean_of_halves(A, Bh, 2, 2)
    assert np.array_equal(got[:, bg], c[:, bg])
    if variance:
        close(var, ref_var)
        _report("variance %dx%d levels %d mode %s" % (W, H, levels, mode), var, ref_var)
        assert not var[bg].any()
    assert len(ms) == levels + 2 and all(v > 0.0 for v in ms)  # each level, the chain, the prepare kernel
    assert np.abs(u8.astype(int) - O.srgb_u8(got, H, W).astype(int)).max() <= 1


# ---- c. unequal halves and awkward pixels ------------------------------------------------------------------
@pytest.mark.parametrize("mode", VR.MODES)
@pytest.mark.parametrize("levels", (0, 1, 3, 5))
def test_gpu_unequal_halves_and_awkward_pixels(levels, mode):
    B = _backend()
    W, H = 70, 9
    variance, demodulate = mode
    A, Bh, guides, bg, pix = VR.awkward_halves()
    got, var, _ = B.denoise_var(A, Bh, 1, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels,
                                want_variance=variance)
    ref, ref_var = VR.denoise_var(A, Bh, 1, 2, guides, W, H, variance=variance, demodulate=demodulate, levels=levels)
    close(got, ref)
    c = VR.mean_of_halves(A, Bh, 1, 2)
    for p in (pix["inf"], pix["nan"]):
        assert np.array_equal(got[:, p], c[:, p], equal_nan=True)
    assert np.array_equal(got[:, bg], c[:, bg])
    others = np.ones(W * H, dtype=bool)
    others[[pix["inf"], pix["nan"]]] = False
    assert np.isfinite(got[:, others]).all()
    if variance:
        close(var, ref_var)
        assert var[pix["inf"]] == 0.0 and var[pix["nan"]] == 0.0 and not var[bg].any() and np.isfinite(var).all()


# ---- d. adaptivity -------------------------------------------------------------------------------------------
def test_gpu_variance_spares_a_clean_step_and_filters_noise():
    B = _backend()
    VR.check_adaptivity(lambda A, Bh, g, W, H: B.denoise_var(A, Bh, 1, 1, g, W, H, variance=True, levels=3)[0],
                        lambda c, g, W, H: B.denoise(c, g, W, H)[0])


def test_gpu_variance_mode_on_the_cornell_fixture():
    """E(filtered) / E(mean) at levels 3 within 1.05 of the restatement's CPU figure (tests/test_denoise_var.py)."""
    B = _backend()
    g, g0 = golden("denoise_var_cornell_64x64"), golden("denoise_cornell_64x64")
    W, H = int(g["width"]), int(g["height"])
    ka, kb = int(g["spp_a"]), int(g["spp_b"])
    guides = DR.aovs(scenes.cornell(W, H))
    got = B.denoise_var(g["half_a"], g["half_b"], ka, kb, guides, W, H, variance=True, demodulate=True, levels=3)[0]
    e0 = DR.tonemapped_error(VR.mean_of_halves(g["half_a"], g["half_b"], ka, kb), g0["ref"])
    ratio = DR.tonemapped_error(got, g0["ref"]) / e0
    print("E(filtered) / E(mean), levels 3, on the device:", ratio)
    assert ratio <= 0.792649567829418 * 1.05


# ---- e. arguments and pointers ---------------------------------------------------------------------------------
def _args(A, Bh, guides, W, H, keep, **kw):
    from sightpy import _native as N

    a = N.DenoiseVarArgs()
    VH.fill_args(a, keep, A, Bh, kw.pop("ka", 1), kw.pop("kb", 1), guides, kw.pop("levels", 2),
                 kw.pop("variance", True), kw.pop("demodulate", True), False, kw)
    out = np.empty((3, W * H))
    keep.append(out)
    a.out_rgb = N.ptr(out)
    return a


BAD = [dict(ka=0), dict(kb=-3), dict(levels=9), dict(levels=-1), dict(sigma_normal=0.0), dict(sigma_albedo=-1.0),
       dict(sigma_plane=0.0), dict(variance=True, sigma_lum=0.0), dict(variance=False, sigma_color=-1.0),
       dict(null="rgb_a"), dict(null="rgb_b"), dict(null="normal"), dict(null="albedo"), dict(null="position"),
       dict(null="depth"), dict(null="out_rgb"), dict(variance=False, with_variance_out=True), dict(flags=16)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_gpu_denoise_var_refuses_bad_arguments(bad):
    from sightpy import _native as N

    lib, ctx = _backend().context()
    A, Bh, guides, _ = VR.random_halves(5, 3, 1)
    kw = dict(bad)
    null, var_out, flags = kw.pop("null", None), kw.pop("with_variance_out", False), kw.pop("flags", 0)
    keep = []
    a = _args(A, Bh, guides, 5, 3, keep, **kw)
    if null:
        setattr(a, null, None)  # (out_rgb: no output at all)
    if var_out:
        v = np.empty(15)
        keep.append(v)
        a.out_variance = N.ptr(v)
    a.flags |= flags
    assert lib.srt_denoise_var(ctx, 5, 3, ctypes.byref(a)) == N.ERR_ARG
    assert b"srt_denoise_var" in lib.srt_last_error()


def test_gpu_denoise_var_refuses_a_bad_size_and_takes_unused_sigmas():
    from sightpy import _native as N

    lib, ctx = _backend().context()
    A, Bh, guides, _ = VR.random_halves(5, 3, 1)
    keep = []
    a = _args(A, Bh, guides, 5, 3, keep)
    assert lib.srt_denoise_var(ctx, 0, 3, ctypes.byref(a)) == N.ERR_ARG
    assert lib.srt_denoise_var(ctx, 5, -1, ctypes.byref(a)) == N.ERR_ARG
    a = _args(A, Bh, guides, 5, 3, keep, variance=True, sigma_color=0.0)  # sigma_color is not in use
    N.check(lib, lib.srt_denoise_var(ctx, 5, 3, ctypes.byref(a)))
    a = _args(A, Bh, guides, 5, 3, keep, variance=False, sigma_lum=0.0)
    N.check(lib, lib.srt_denoise_var(ctx, 5, 3, ctypes.byref(a)))


def test_gpu_denoise_var_device_pointers_equal_host_pointers():
    """Device arrays are used in place and device outputs written in place: the same bits as from host arrays,
    the variance and the 4-byte image included."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    W, H = 70, 9
    n = W * H
    A, Bh, guides, _ = VR.random_halves(W, H, 5)
    kw = dict(variance=True, demodulate=True, levels=3)
    want, want_var, want_u8 = B.denoise_var(A, Bh, 2, 1, guides, W, H, want_variance=True, rgbx=True, **kw)
    with B.DeviceArrays() as pool:
        dev = {}
        for k, v in (("a", A), ("b", Bh), ("normal", guides["normal"]), ("albedo", guides["albedo"]),
                     ("position", guides["position"]), ("depth", guides["depth"])):
            v = np.ascontiguousarray(v)
            dev[k] = pool.alloc(v.nbytes)
            N.check(lib, lib.srt_memcpy(ctx, dev[k], N.ptr(v), v.nbytes))
        # through the wrapper (device inputs, host outputs)
        got, got_var, got_u8 = B.denoise_var(dev["a"], dev["b"], 2, 1, dev, W, H, want_variance=True, rgbx=True, **kw)
        assert np.array_equal(got, want) and np.array_equal(got_var, want_var) and np.array_equal(got_u8, want_u8)
        # and with device outputs
        a = N.DenoiseVarArgs()
        a.rgb_a, a.rgb_b = dev["a"].value, dev["b"].value
        for k in ("normal", "albedo", "position", "depth"):
            setattr(a, k, dev[k].value)
        a.spp_a, a.spp_b, a.levels = 2, 1, 3
        a.flags = N.DENOISE_RGBX | N.DENOISE_VARIANCE | N.DENOISE_DEMODULATE
        for k in ("sigma_color", "sigma_lum", "sigma_normal", "sigma_albedo", "sigma_plane"):
            setattr(a, k, VR.DEFAULTS[k])
        d_out, d_var, d_u8 = pool.doubles(3 * n), pool.doubles(n), pool.alloc(4 * n)
        a.out_rgb, a.out_variance, a.out_srgb8 = d_out.value, d_var.value, d_u8.value
        N.check(lib, lib.srt_denoise_var(ctx, W, H, ctypes.byref(a)))
        assert np.array_equal(pool.fetch(d_out, (3, n)), want)
        assert np.array_equal(pool.fetch(d_var, (n,)), want_var)
        assert np.array_equal(pool.fetch(d_u8, (H, W, 4), np.uint8), want_u8)
    assert not pool.ptrs


def test_gpu_out_variance_at_levels_0_is_prepares():
    B = _backend()
    W, H = 70, 9
    A, Bh, guides, _ = VR.random_halves(W, H, 6)
    for demodulate in (False, True):
        _, var, _ = B.denoise_var(A, Bh, 3, 2, guides, W, H, variance=True, demodulate=demodulate, levels=0,
                                  want_variance=True)
        close(var, VR.prepare(A, Bh, 3, 2, guides, demodulate)[1])
        assert var.max() > 0.0


# ---- f. through the renderer -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell24():
    sc = scenes.cornell(24, 24)
    return sc, DR.aovs(sc)


def _plain_linear(B, sc, spp, rng):
    """The linear RGB of the frame a plain sc.render(spp, rng=rng) traces from numpy's current state."""
    if rng == "numpy":
        return B.render_scene(sc, spp, mt=True).rgb
    if rng == "numpy-host":
        jitter = sc.camera.draw_jitter(spp)
        sc.camera.draw_jitter(1)
        return B.render_scene(sc, spp, jitter=jitter).rgb
    return B.render_scene(sc, spp).rgb


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("rng", ["numpy", "numpy-host", "device"])
def test_gpu_render_half_frames_end_to_end(cornell24, rng):
    sc, guides = cornell24
    B = _backend()
    spp = 4
    np.random.seed(3)
    plain = _plain_linear(B, sc, spp, rng)
    np.random.seed(3)
    sc.render(spp, rng=rng)
    after_plain = np.random.get_state()
    # the two half-frames are samples 0..1 and 2..3 of that very frame
    np.random.seed(3)
    A, Bh, ka, kb, _ = B.render_halves(sc, spp, rng=rng)
    assert (ka, kb) == (2, 2) and _same_state(np.random.get_state(), after_plain)
    assert np.abs(A - Bh).max() > 1e-3
    np.testing.assert_allclose(VR.mean_of_halves(A, Bh, ka, kb), plain, rtol=1e-12, atol=0.0)
    # the image: half-frames -> restated pipeline -> the oracle's resolve
    np.random.seed(3)
    img = sc.render(spp, rng=rng, denoise={"variance": True, "demodulate": True})
    assert _same_state(np.random.get_state(), after_plain)
    assert img.mode == "RGB" and img.size == (24, 24)
    want = O.srgb_u8(VR.denoise_var(A, Bh, ka, kb, guides, 24, 24, variance=True, demodulate=True)[0], 24, 24)
    assert np.abs(np.asarray(img).astype(int) - want.astype(int)).max() <= 1
    dn = sc.last_stats["denoise"]
    assert dn["variance"] and dn["demodulate"] and dn["sigma_lum"] == VR.DEFAULTS["sigma_lum"]
    assert (dn["ka"], dn["kb"]) == (2, 2) and dn["ms_prepare"] > 0.0 and len(dn["ms_levels"]) == dn["levels"] == 4
    assert sc.last_stats["total_rays"] > 0


def test_gpu_render_half_frames_odd_spp_and_one_flag(cornell24):
    sc, guides = cornell24
    B = _backend()
    np.random.seed(5)
    plain = B.render_scene(sc, 3, mt=True).rgb
    np.random.seed(5)
    A, Bh, ka, kb, _ = B.render_halves(sc, 3)
    assert (ka, kb) == (1, 2)
    np.testing.assert_allclose(VR.mean_of_halves(A, Bh, ka, kb), plain, rtol=1e-12, atol=0.0)
    np.random.seed(5)
    img = sc.render(3, denoise={"demodulate": True, "levels": 2})
    want = O.srgb_u8(VR.denoise_var(A, Bh, ka, kb, guides, 24, 24, demodulate=True, levels=2)[0], 24, 24)
    assert np.abs(np.asarray(img).astype(int) - want.astype(int)).max() <= 1


def test_gpu_render_new_keys_refusals_and_the_old_path(cornell24):
    sc, guides = cornell24
    with pytest.raises(ValueError):
        sc.render(1, denoise={"variance": True})
    with pytest.raises(ValueError):
        sc.render(2, denoise={"variance": True, "nope": 1})
    with pytest.raises(ValueError):
        sc.render(2, denoise={"nope": 1})
    # a dict without the new keys (or with both off) runs today's path and gives today's bytes
    np.random.seed(3)
    want = sc.render(2, denoise=True)
    np.random.seed(3)
    got = sc.render(2, denoise={"variance": False, "demodulate": False})
    assert got.tobytes() == want.tobytes() and "ka" not in sc.last_stats["denoise"]
