"""Per-collider motion in the temporal accumulation on the device: srt_temporal_accumulate with a motion table
(k_temporal<true>) on the checks of tests/test_temporal_motion.py, its pointers and arguments, and
Scene.render(denoise={"temporal": True, "motion": True, ...}) and create_animation end to end on example1's moving
sphere.  Floats within rtol 1e-5 / atol 1e-12."""
import ctypes

import numpy as np
import pytest

import denoise_ref as DR
import denoise_var_ref as VR
import scenes
import sightpy_oracle as O
import temporal_host as TH
import temporal_motion_ref as MR
import temporal_ref as TR
from denoise_ref import SHAPES

pytestmark = pytest.mark.gpu


def _backend():
    from sightpy import _backend

    return _backend


def _cam(prev_cam, W, H):
    if prev_cam is None:
        return None
    cd = TH.camera_desc(prev_cam)
    cd.width, cd.height = W, H
    return cd


def run(A, B, guides, W, H, history=None, prev_cam=None, demodulate=False, motion=None, **kw):
    """srt_temporal_accumulate over host arrays, with temporal_motion_ref.accumulate's arguments and result."""
    return _backend().temporal_accumulate(A, B, guides, W, H, history=history, prev_cam=_cam(prev_cam, W, H),
                                          demodulate=demodulate, motion=motion, **kw)


# ---- a. the CPU suite's checks, on the device ------------------------------------------------------------------
@pytest.mark.parametrize("columns", (1, -1))
def test_gpu_exact_shift_by_motion(columns):
    MR.check_exact_shift_by_motion(run, columns)


def test_gpu_rotation_the_normal_test_refuses_without_the_row():
    MR.check_rotation(run)


def test_gpu_identity_and_unknown_rows():
    MR.check_identity_and_unknown_rows(run)


@pytest.mark.parametrize("demodulate", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_matches_the_restatement_with_motion(shape, demodulate):
    W, H = shape
    MR.check_against_restatement(run, W, H, demodulate)


def test_gpu_a_first_frame_ignores_the_table():
    s = MR.moving_sequence(70, 9, 3)
    got = run(s["A"], s["B"], s["guides"], 70, 9, motion=s["motion"])
    want = run(s["A"], s["B"], s["guides"], 70, 9)
    assert all(TR.same_bits(got[k], want[k]) for k in TR.OUTPUTS)


# ---- b. pointers and arguments ---------------------------------------------------------------------------------
def test_gpu_motion_table_in_device_memory_gives_the_same_bits():
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    W, H = 70, 9
    s = MR.moving_sequence(W, H, 5)
    kw = dict(history=s["history"], prev_cam=s["prev_cam"], demodulate=True)
    want = run(s["A"], s["B"], s["guides"], W, H, motion=s["motion"], **kw)
    with B.DeviceArrays() as pool:
        rows = np.ascontiguousarray(s["motion"])
        p = pool.alloc(rows.nbytes)
        N.check(lib, lib.srt_memcpy(ctx, p, N.ptr(rows), rows.nbytes))
        got = run(s["A"], s["B"], s["guides"], W, H, motion=(p, len(rows)), **kw)
    assert all(TR.same_bits(got[k], want[k]) for k in TR.OUTPUTS)
    assert (got["len"][s["guides"]["hit_id"] == 1] > 1.0).any()


@pytest.mark.parametrize("n_motion", (0, -1))
def test_gpu_refuses_a_table_without_rows(n_motion):
    from sightpy import _native as N

    lib, ctx = _backend().context()
    s = TR.random_sequence(5, 3, 1)
    rows = MR.identity_rows(3)
    for history in (True, False):  # the check does not depend on a history being there
        keep = []
        a = N.TemporalArgs()
        keep.append(TH.fill_args(a, keep, s["A"], s["B"], s["guides"], 5, 3, s["history"] if history else None,
                                 s["prev_cam"], True, **TR.DEFAULTS))
        a.motion, a.n_motion = N.ptr(rows), 3
        N.check(lib, lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)))
        a.n_motion = n_motion
        assert lib.srt_temporal_accumulate(ctx, 5, 3, ctypes.byref(a)) == N.ERR_ARG
        assert lib.srt_last_error().startswith(b"srt_temporal_accumulate")


# ---- c. through the renderer -----------------------------------------------------------------------------------
DN = {"temporal": True, "variance": True, "demodulate": True}
DNM = dict(DN, motion=True)
W, H, SPP = 48, 36, 2


def _same_state(a, b):
    return a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


def update(scene, t):
    from sightpy import vec3

    scene.collider_list[0].center = vec3(-0.75 + t, 0.1, -3.0)


def _frames(dn, resets=(), plain=()):
    """Three frames of example1 48 x 36 at 2 spp with the gold sphere at x = -0.75 + t, t = 0, 1/3, 2/3, seeds
    4, 5, 6: [(image bytes, last_stats["denoise"])].  `resets`: frames before which reset_history() is called;
    `plain`: frames rendered with DN (no "motion") instead of `dn`."""
    sc = scenes.example1(W, H, 3)
    out = []
    for k in range(3):
        update(sc, k / 3.0)
        if k in resets:
            sc.reset_history()
        np.random.seed(4 + k)
        img = sc.render(SPP, denoise=DN if k in plain else dn)
        out.append((img.tobytes(), dict(sc.last_stats["denoise"])))
    return out


def test_gpu_render_motion_end_to_end(tmp_path, monkeypatch):
    """Each of the three frames is the restated pipeline's (render_halves -> temporal_motion_ref with rows from
    the objects -> denoise_var_ref -> the oracle's resolve) within one count; one collider moves on frames 2 and
    3; numpy's RNG ends where the plain render leaves it; the third image differs from the sequence without
    "motion"; create_animation writes the same three images."""
    from PIL import Image
    from sightpy import create_animation

    B = _backend()
    sc = scenes.example1(W, H, 3)
    hist, cam, snap, images = None, None, None, []
    for k in range(3):
        update(sc, k / 3.0)
        np.random.seed(4 + k)
        sc.render(SPP)
        after_plain = np.random.get_state()
        np.random.seed(4 + k)
        A, Bh, ka, kb, _ = B.render_halves(sc, SPP)
        np.random.seed(4 + k)
        img = sc.render(SPP, denoise=DNM)
        assert _same_state(np.random.get_state(), after_plain)
        guides, now = DR.aovs(sc), MR.snapshot(sc)
        rows = MR.object_motion(snap, now) if snap is not None else None
        info = {}
        out = MR.accumulate(A, Bh, guides, W, H, history=hist, prev_cam=cam, motion=rows, demodulate=True, info=info)
        sphere = guides["hit_id"] == 0
        assert info["has"][sphere].any() == (k > 0)  # (the moving sphere keeps history by its row alone)
        want = O.srgb_u8(VR.denoise_var(out["a"], out["b"], ka, kb, guides, W, H, variance=True, demodulate=True)[0], H, W)
        dev = np.abs(np.asarray(img).astype(int) - want.astype(int)).max()
        print("frame", k, "largest deviation in counts", dev)
        assert dev <= 1, k
        hist, cam, snap = TR.next_history(out, guides), TR.camera_dict(sc.camera), now
        dn = sc.last_stats["denoise"]
        assert dn["motion"] is True and dn["ms_temporal"] > 0.0
        assert (dn["motion_moved"], dn["motion_unknown"]) == ((1, 0) if k else (0, 0))
        images.append(img.tobytes())
    # without "motion" the sphere's history is refused: another third frame, and no motion keys
    without = _frames(DN)
    assert without[0][0] == images[0] and without[2][0] != images[2]
    assert "motion_moved" not in without[2][1] and "motion" not in without[2][1]
    # create_animation, on a scene of its own
    monkeypatch.chdir(tmp_path)
    sc2 = scenes.example1(W, H, 3)
    np.random.seed(4)
    create_animation(sc2, SPP, 3, 0.0, 1.0, update, "anim", denoise=DNM)
    np.random.seed(4)
    sc3 = scenes.example1(W, H, 3)
    t = 0.0
    for k in range(3):
        update(sc3, t)
        t += 1.0 / 3
        ref = np.array(sc3.render(SPP, denoise=DNM))
        got = np.array(Image.open(tmp_path / "frames" / ("anim_%d.png" % k)))
        assert np.array_equal(got, ref), k
    assert sc3.last_stats["denoise"]["motion_moved"] == 1


def test_gpu_render_motion_needs_the_previous_table():
    """After reset_history(), and after a frame rendered without "motion", the next motion frame runs without a
    table: no row counted, and the bytes of the same frame of the sequence without "motion"."""
    plain = _frames(DN)
    # reset before the third frame: a first frame again, with or without the key
    a, b = _frames(DNM, resets=(2,)), _frames(DN, resets=(2,))
    assert a[2][0] == b[2][0] and (a[2][1]["motion_moved"], a[2][1]["motion_unknown"]) == (0, 0)
    assert a[1][1]["motion_moved"] == 1
    # the second frame without the key: the third has a history but no table of the frame before
    c = _frames(DNM, plain=(1,))
    assert c[2][0] == plain[2][0] and (c[2][1]["motion_moved"], c[2][1]["motion_unknown"]) == (0, 0)
    assert "motion_moved" not in c[1][1]
    # (and with the table it is another image)
    assert _frames(DNM)[2][0] != plain[2][0]
