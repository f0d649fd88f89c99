"""The denoiser on the device: srt_render_aovs (k_aov) and srt_denoise (k_atrous) against the restatement
in tests/denoise_ref.py on the shapes of tests/test_denoise.py, and Scene.render(denoise=...) end to end.
Hit ids exact, floats within rtol 1e-5 / atol 1e-12."""
import ctypes

import numpy as np
import pytest

import denoise_ref as DR
import scenes
import sightpy_oracle as O
import vattr_ref as VR
from conftest import golden
from denoise_ref import LEVELS, SHAPES, close, random_frame, same_aovs

pytestmark = pytest.mark.gpu


def _backend():
    from sightpy import _backend

    return _backend


# ---- 1. first-hit guide images ------------------------------------------------------------------------
@pytest.mark.parametrize("name,size", [("example1", (64, 48)), ("cornell", (24, 24)), ("features", (48, 36))])
def test_gpu_aovs_match_the_restatement(name, size):
    sc = getattr(scenes, name)(*size)
    got = _backend().render_aovs(sc)
    assert got["ms_kernel"] > 0.0
    same_aovs(got, DR.aovs(sc))


def test_gpu_aovs_smooth_textured_mesh_through_the_bvh(tmp_path, monkeypatch):
    p = str(tmp_path / "ico1.obj")
    VR.write_smooth_icosphere_obj(p, 1)
    sc = VR.mesh_scene(p, 64, 48, 3, smooth=True, texcoords=True, material=VR.checker())
    got = _backend().render_aovs(sc)
    VR.patch(monkeypatch)
    j = np.stack([np.full(64 * 48, 0.5), np.full(64 * 48, 0.5), np.zeros(64 * 48), np.zeros(64 * 48)])[None]
    same_aovs(got, DR.aovs(sc), skip=VR.texel_boundary_pixels(sc, j))


def test_gpu_get_aovs_is_public_and_draws_nothing():
    sc = scenes.example1(64, 48)
    np.random.seed(11)
    before = np.random.get_state()
    got = sc.get_aovs()
    after = np.random.get_state()
    assert before[2] == after[2] and np.array_equal(before[1], after[1])
    assert set(got) == {"hit_id", "depth", "position", "normal", "albedo"}
    same_aovs(got, DR.aovs(sc))


def test_gpu_aovs_without_a_scene():
    from sightpy import _native as N

    B = _backend()
    lib, _ = B.context()
    ctx = ctypes.c_void_p()
    N.check(lib, lib.srt_create(B._STATE["device"], ctypes.byref(ctx)))
    try:
        cd = B.camera_desc(scenes.cornell(8, 8).camera)
        out = N.AovOut()
        depth = np.empty(64)
        out.depth = N.ptr(depth)
        assert lib.srt_render_aovs(ctx, ctypes.byref(cd), ctypes.byref(out)) == N.ERR_NOSCENE
        assert b"no scene" in lib.srt_last_error()
    finally:
        N.check(lib, lib.srt_destroy(ctx))


# ---- 2. the filter --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    g = golden("denoise_cornell_64x64")
    W, H = int(g["width"]), int(g["height"])
    return {"noisy": g["noisy"], "W": W, "H": H, "guides": DR.aovs(scenes.cornell(W, H))}


@pytest.mark.parametrize("levels", LEVELS)
def test_gpu_denoise_matches_the_restatement_on_the_fixture(fixture, levels):
    W, H = fixture["W"], fixture["H"]
    ms = []
    got, u8 = _backend().denoise(fixture["noisy"], fixture["guides"], W, H, levels=levels, timings=ms)
    close(got, DR.atrous(fixture["noisy"], fixture["guides"], W, H, levels=levels))
    assert len(ms) == levels + 1 and all(v > 0.0 for v in ms)  # each level, then the whole chain
    assert np.abs(u8.astype(int) - O.srgb_u8(got, H, W).astype(int)).max() <= 1


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_denoise_matches_the_restatement_on_random_frames(shape, levels):
    W, H = shape
    rgb, guides, bg = random_frame(W, H, 10 * W + H)
    kw = dict(levels=levels, sigma_color=0.6, sigma_normal=0.3, sigma_albedo=0.2, sigma_plane=0.05)
    got, _ = _backend().denoise(rgb, guides, W, H, **kw)
    close(got, DR.atrous(rgb, guides, W, H, **kw))
    assert np.array_equal(got[:, bg], rgb[:, bg])


@pytest.mark.parametrize("levels", LEVELS)
def test_gpu_denoise_non_finite_pixels(levels):
    W, H = 70, 9
    rgb, guides, bg = random_frame(W, H, 3)
    a, b = 2 * W + 5, 6 * W + 66
    rgb[1, a] = np.inf
    rgb[2, b] = np.nan
    got, _ = _backend().denoise(rgb, guides, W, H, levels=levels)
    close(got, DR.atrous(rgb, guides, W, H, levels=levels))
    for p in (a, b):
        assert np.array_equal(got[:, p], rgb[:, p], equal_nan=True)
    others = np.ones(W * H, dtype=bool)
    others[[a, b]] = False
    assert np.isfinite(got[:, others]).all()


def test_gpu_denoise_device_pointers_equal_host_pointers():
    """Device arrays are filtered in place of staged copies: the same bits as from host arrays, the
    4-byte image included."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    W, H = 70, 9
    n = W * H
    rgb, guides, _ = random_frame(W, H, 5)
    want, want_u8 = B.denoise(rgb, guides, W, H, levels=3, rgbx=True)
    a = N.DenoiseArgs()
    for k, v in (("rgb", rgb), ("normal", guides["normal"]), ("albedo", guides["albedo"]),
                 ("position", guides["position"]), ("depth", guides["depth"])):
        v = np.ascontiguousarray(v)
        d = B.device_buffer("dn_test_" + k, v.nbytes)
        N.check(lib, lib.srt_memcpy(ctx, d, N.ptr(v), v.nbytes))
        setattr(a, k, d.value)
    d_out, d_u8 = B.device_buffer("dn_test_out", 24 * n), B.device_buffer("dn_test_u8", 4 * n)
    a.levels, a.flags = 3, N.DENOISE_RGBX
    a.sigma_color, a.sigma_normal, a.sigma_albedo, a.sigma_plane = (DR.DEFAULTS[k] for k in (
        "sigma_color", "sigma_normal", "sigma_albedo", "sigma_plane"))
    a.out_rgb, a.out_srgb8 = d_out.value, d_u8.value
    try:
        N.check(lib, lib.srt_denoise(ctx, W, H, ctypes.byref(a)))
        got, got_u8 = np.empty((3, n)), np.empty((H, W, 4), dtype=np.uint8)
        N.check(lib, lib.srt_memcpy(ctx, N.ptr(got), d_out, got.nbytes))
        N.check(lib, lib.srt_memcpy(ctx, N.ptr(got_u8), d_u8, got_u8.nbytes))
    finally:
        for k in ("rgb", "normal", "albedo", "position", "depth", "out", "u8"):
            B.release_buffer("dn_test_" + k)
    assert np.array_equal(got, want) and np.array_equal(got_u8, want_u8)


@pytest.mark.parametrize("bad", [{"levels": 9}, {"levels": -1}, {"sigma_normal": 0.0}, {"sigma_albedo": -2.0}])
def test_gpu_denoise_refuses_bad_arguments(bad):
    from sightpy import _native as N

    rgb, guides, _ = random_frame(5, 3, 1)
    with pytest.raises(N.SrtError) as e:
        _backend().denoise(rgb, guides, 5, 3, **bad)
    assert e.value.code == N.ERR_ARG


# ---- 3. through the renderer ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell24():
    sc = scenes.cornell(24, 24)
    return sc, DR.aovs(sc)


def test_gpu_denoise_levels_0_is_the_render_itself(cornell24):
    sc, guides = cornell24
    B = _backend()
    np.random.seed(2)
    out = B.render_scene(sc, 2, mt=True, seed=5)
    got, u8 = B.denoise(out.rgb, guides, 24, 24, levels=0)
    assert np.array_equal(got, out.rgb)
    assert np.array_equal(u8, out.srgb8)


def test_gpu_render_denoised_end_to_end(cornell24):
    sc, guides = cornell24
    B = _backend()
    np.random.seed(3)
    img = sc.render(2, denoise=True)
    state = np.random.get_state()
    assert img.mode == "RGB" and img.size == (24, 24)
    assert sc.last_stats["denoise"]["levels"] == DR.DEFAULTS["levels"] and len(sc.last_stats["denoise"]["ms_levels"]) == 4
    # the same frame by hand: the renderer's linear RGB, the restated filter, the oracle's resolve
    np.random.seed(3)
    out = B.render_scene(sc, 2, mt=True)
    want = O.srgb_u8(DR.atrous(out.rgb, guides, 24, 24), 24, 24)
    assert np.abs(np.asarray(img).astype(int) - want.astype(int)).max() <= 1
    assert np.abs(np.asarray(img).astype(int) - out.srgb8.astype(int)).max() > 1  # (it did filter)
    # numpy's stream is where a plain render leaves it
    np.random.seed(3)
    plain = sc.render(2)
    after = np.random.get_state()
    assert state[2] == after[2] and np.array_equal(state[1], after[1])
    # denoise=False is the call without the parameter
    np.random.seed(3)
    off = sc.render(2, denoise=False)
    assert off.tobytes() == plain.tobytes() and off.size == plain.size and off.mode == plain.mode
    # and a dict overrides the defaults
    np.random.seed(3)
    img2 = sc.render(2, denoise={"levels": 2, "sigma_color": 0.5})
    want2 = O.srgb_u8(DR.atrous(out.rgb, guides, 24, 24, levels=2, sigma_color=0.5), 24, 24)
    assert np.abs(np.asarray(img2).astype(int) - want2.astype(int)).max() <= 1
