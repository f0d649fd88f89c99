"""Temporal accumulation on the device: srt_temporal_accumulate (k_temporal) against the restatement in
tests/temporal_ref.py on the shapes and cases of tests/test_temporal.py, its arguments and pointers, and
Scene.render(denoise={"temporal": True, ...}) and create_animation(..., denoise=...) end to end.  Floats within
rtol 1e-5 / atol 1e-12."""
import ctypes

import numpy as np
import pytest

import denoise_ref as DR
import denoise_var_ref as VR
import scenes
import sightpy_oracle as O
import temporal_host as TH
import temporal_ref as TR
from denoise_ref import SHAPES

pytestmark = pytest.mark.gpu

RATIO_LEVELS_0, RATIO_LEVELS_3 = 0.22914871885517754, 0.192383505904628  # tests/test_temporal.py, on the CPU


def _backend():
    from sightpy import _backend

    return _backend


def _cam(prev_cam, W, H):
    if prev_cam is None:
        return None
    cd = TH.camera_desc(prev_cam)
    cd.width, cd.height = W, H
    return cd


def run(A, B, guides, W, H, history=None, prev_cam=None, demodulate=False, timings=None, **kw):
    """srt_temporal_accumulate over host arrays, with temporal_ref.accumulate's arguments and result."""
    return _backend().temporal_accumulate(A, B, guides, W, H, history=history, prev_cam=_cam(prev_cam, W, H),
                                          demodulate=demodulate, timings=timings, **kw)


# ---- a. against the restatement, with the pixels that are copied through ------------------------------------
@pytest.mark.parametrize("with_history", (False, True))
@pytest.mark.parametrize("demodulate", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_matches_the_restatement(shape, demodulate, with_history):
    W, H = shape
    ms = []
    got, ref, _ = TR.check_against_restatement(lambda *a, **kw: run(*a, timings=ms, **kw), W, H, demodulate, with_history)
    assert len(ms) == 1 and ms[0] > 0.0
    for k in TR.OUTPUTS:
        sel = np.isfinite(ref[k]) & (ref[k] != 0.0)
        if sel.any():
            print("deviation", k, shape, "rel %.3g" % float((np.abs(got[k][sel] - ref[k][sel]) / np.abs(ref[k][sel])).max()))


# ---- b. the cases with a known answer ------------------------------------------------------------------------
@pytest.mark.parametrize("columns", (1, -1))
def test_gpu_exact_shift(columns):
    TR.check_exact_shift(run, columns)


def test_gpu_static_camera_gives_the_arithmetic_mean():
    TR.check_static_mean(run)


def test_gpu_max_history_clamps():
    TR.check_max_history(run)


def test_gpu_accumulation_on_the_cornell_fixture():
    """The accumulated, filtered error ratios (srt_temporal_accumulate, then srt_denoise_var) within 1.05 of the
    restatement's CPU figures, and the issue's condition: at most half the error of the last frame alone."""
    B = _backend()
    filt = lambda a, b, ka, kb, g, W, H, **kw: B.denoise_var(a, b, ka, kb, g, W, H, want_u8=False, **kw)
    new, alone = TR.fixture_error_ratios(run, filt)
    print("E / E(mean of the last frame), on the device: accumulated", new, "the last frame alone", alone)
    assert new[0] <= RATIO_LEVELS_0 * 1.05 and new[3] <= RATIO_LEVELS_3 * 1.05
    assert new[3] <= 0.5 * alone[3]


# ---- c. pointers and arguments -------------------------------------------------------------------------------
def test_gpu_temporal_device_pointers_equal_host_pointers():
    """Device arrays are used in place and device outputs written in place (out_a / out_b over rgb_a / rgb_b
    included): the same bits as from host arrays."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    W, H = 70, 9
    n = W * H
    s = TR.random_sequence(W, H, 5)
    want = run(s["A"], s["B"], s["guides"], W, H, history=s["history"], prev_cam=s["prev_cam"], demodulate=True)
    with B.DeviceArrays() as pool:
        def up(v, dtype=np.float64):
            v = np.ascontiguousarray(v, dtype=dtype)
            p = pool.alloc(v.nbytes)
            N.check(lib, lib.srt_memcpy(ctx, p, N.ptr(v), v.nbytes))
            return p

        dA, dB = up(s["A"]), up(s["B"])
        dg = {k: up(s["guides"][k], np.int32 if k == "hit_id" else np.float64)
              for k in ("hit_id", "position", "normal", "albedo", "depth")}
        dh = {k: up(s["history"][k], np.int32 if k == "hit_id" else np.float64) for k in s["history"]}
        # device inputs, host outputs
        got = B.temporal_accumulate(dA, dB, dg, W, H, history=dh, prev_cam=_cam(s["prev_cam"], W, H), demodulate=True)
        assert all(TR.same_bits(got[k], want[k]) for k in TR.OUTPUTS)
        # device outputs, the half-frames in place
        out = {"a": dA, "b": dB, "hist_a": pool.doubles(3 * n), "hist_b": pool.doubles(3 * n), "len": pool.doubles(n)}
        res = B.temporal_accumulate(dA, dB, dg, W, H, history=dh, prev_cam=_cam(s["prev_cam"], W, H), demodulate=True,
                                    out=out)
        assert res is out
        for k in TR.OUTPUTS:
            assert TR.same_bits(pool.fetch(out[k], want[k].shape), want[k]), k
    assert not pool.ptrs


def _args(s, W, H, keep, history=True, demodulate=True, **kw):
    from sightpy import _native as N

    a = N.TemporalArgs()
    p = dict(TR.DEFAULTS, **kw)
    out = TH.fill_args(a, keep, s["A"], s["B"], s["guides"], W, H, s["history"] if history else None, s["prev_cam"],
                       demodulate, p["max_history"], p["normal_max"], p["plane_max"])
    keep.append(out)
    return a


BAD = [dict(max_history=0), dict(max_history=-3), dict(normal_max=-0.1), dict(normal_max=float("nan")),
       dict(normal_max=float("inf")), dict(plane_max=-1.0), dict(plane_max=float("nan")), dict(plane_max=float("inf")),
       dict(flags=2), dict(flags=-2)] + \
      [dict(null=k) for k in ("rgb_a", "rgb_b", "hit_id", "position", "normal", "albedo", "depth", "out_a", "out_b",
                              "out_hist_a", "out_hist_b", "out_len", "hist_a", "hist_b", "hist_hit_id", "hist_position",
                              "hist_normal", "prev_cam")] + \
      [dict(prev_size=(6, 3)), dict(prev_size=(5, 4)), dict(alias="hist_a"), dict(alias="hist_b"), dict(alias="hist_len")]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_gpu_temporal_refuses_bad_arguments(bad):
    from sightpy import _native as N

    lib, ctx = _backend().context()
    s = TR.random_sequence(5, 3, 1)
    kw = dict(bad)
    null, flags, prev_size, alias = kw.pop("null", None), kw.pop("flags", 0), kw.pop("prev_size", None), kw.pop("alias", None)
    keep = []
    a = _args(s, 5, 3, keep, **kw)
    if null:
        setattr(a, null, None)
    if prev_size:
        a.prev_cam.contents.width, a.prev_cam.contents.height = prev_size
    if alias:
        setattr(a, "out_" + alias.replace("hist_len", "len"), getattr(a, alias))
    a.flags |= flags
    assert lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)) == N.ERR_ARG
    assert b"srt_temporal_accumulate" in lib.srt_last_error()


def test_gpu_temporal_refuses_a_bad_size_and_needs_albedo_only_to_demodulate():
    from sightpy import _native as N

    lib, ctx = _backend().context()
    s = TR.random_sequence(5, 3, 1)
    keep = []
    a = _args(s, 5, 3, keep)
    for size in ((0, 3), (5, -1)):
        assert lib.srt_temporal_accumulate(ctx, size[0], size[1], ctypes.byref(a)) == N.ERR_ARG
        assert b"srt_temporal_accumulate" in lib.srt_last_error()
    a = _args(s, 5, 3, keep, demodulate=False)
    assert not a.albedo
    N.check(lib, lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)))
    # without hist_len nothing else of the history is read
    a = _args(s, 5, 3, keep, history=False)
    assert not a.hist_len and not a.prev_cam
    N.check(lib, lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)))
    # zero thresholds are legal
    a = _args(s, 5, 3, keep, normal_max=0.0, plane_max=0.0)
    N.check(lib, lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)))


# ---- d. through the renderer -----------------------------------------------------------------------------------
DN = {"temporal": True, "variance": True, "demodulate": True}


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


def _move(sc, dx, W=24, H=24):
    from sightpy import vec3

    sc.add_Camera(screen_width=W, screen_height=H, look_from=vec3(278 - dx, 278, 800), look_at=vec3(278, 278, 0),
                  focal_distance=1.0, field_of_view=40)


def test_gpu_render_temporal_end_to_end():
    """Three frames of cornell 24 x 24 at 4 spp with the camera nudged between them: each image is the restated
    pipeline's (render_halves -> temporal_ref -> denoise_var_ref -> the oracle's resolve) within one count, and
    numpy's RNG ends where the plain render leaves it."""
    B = _backend()
    sc = scenes.cornell(24, 24)
    hist, cam = None, None
    for k, dx in enumerate((8, 4, 0)):
        _move(sc, dx)
        np.random.seed(3 + k)
        sc.render(4)
        after_plain = np.random.get_state()
        np.random.seed(3 + k)
        A, Bh, ka, kb, _ = B.render_halves(sc, 4)
        np.random.seed(3 + k)
        img = sc.render(4, denoise=DN)
        assert _same_state(np.random.get_state(), after_plain)
        guides = DR.aovs(sc)
        info = {}
        out = TR.accumulate(A, Bh, guides, 24, 24, history=hist, prev_cam=cam, demodulate=True, info=info)
        assert info["has"].any() == (k > 0)
        want = O.srgb_u8(VR.denoise_var(out["a"], out["b"], ka, kb, guides, 24, 24, variance=True, demodulate=True)[0], 24, 24)
        assert np.abs(np.asarray(img).astype(int) - want.astype(int)).max() <= 1, k
        hist, cam = TR.next_history(out, guides), TR.camera_dict(sc.camera)
        dn = sc.last_stats["denoise"]
        assert dn["ms_temporal"] > 0.0 and dn["temporal"] and dn["max_history"] == 32 and dn["ms_prepare"] > 0.0
    # the accumulated frame differs from the same frame without history
    np.random.seed(5)
    alone = scenes.cornell(24, 24).render(4, denoise=DN)
    assert alone.tobytes() != img.tobytes()


def test_gpu_render_temporal_resets_and_the_old_path():
    sc = scenes.cornell(24, 24)
    dn2 = {"variance": True, "demodulate": True}

    def frame(scene, seed, dn=DN, spp=4):
        np.random.seed(seed)
        return scene.render(spp, denoise=dn).tobytes()

    first = frame(scenes.cornell(24, 24), 7)
    assert frame(sc, 6) != first
    assert frame(sc, 7) != first               # accumulated on the frame before
    sc.reset_history()
    assert frame(sc, 7) == first               # a first frame again
    # a frame of another size drops the history
    frame(sc, 8)
    _move(sc, 0, 20, 16)
    small = scenes.cornell(20, 16)
    assert frame(sc, 9) == frame(small, 9)
    # without "temporal" (or with it off): today's half-frame path and bytes, history untouched
    np.random.seed(9)
    want = small.render(4, denoise=dn2).tobytes()
    assert frame(small, 9, dict(dn2, temporal=False)) == want and "ms_temporal" not in small.last_stats["denoise"]
    frame(small, 2)                             # (a history of other samples than frame 9's own)
    assert frame(small, 9, dict(dn2, temporal=True)) != want


def test_gpu_create_animation_with_temporal_denoise(tmp_path, monkeypatch):
    """create_animation(..., denoise=...) writes the frames of the frame-by-frame loop on a scene of its own
    (test_gpu_create_animation_frames' moving sphere)."""
    from PIL import Image
    from sightpy import create_animation, vec3

    monkeypatch.chdir(tmp_path)

    def update(scene, t):
        scene.collider_list[0].center = vec3(-0.75 + t, 0.1, -3.0)

    sc = scenes.example1(48, 36, 3)
    np.random.seed(4)
    create_animation(sc, 2, 3, 0.0, 1.0, update, "anim", denoise=DN)
    sc2 = scenes.example1(48, 36, 3)
    sc2.reset_history()
    np.random.seed(4)
    t = 0.0
    frames = []
    for i in range(3):
        update(sc2, t)
        ref = np.array(sc2.render(2, denoise=DN))
        got = np.array(Image.open(tmp_path / "frames" / ("anim_%d.png" % i)))
        assert np.array_equal(got, ref), i
        frames.append(ref)
        t += 1.0 / 3
    # and the sequence did accumulate: the last frame alone looks different
    sc3 = scenes.example1(48, 36, 3)
    update(sc3, 2.0 / 3)
    np.random.seed(4)
    for i in range(2):
        sc3.render(2)  # (numpy's stream up to the third frame)
    assert not np.array_equal(np.array(sc3.render(2, denoise=DN)), frames[2])
