"""Temporal accumulation of half-frames without a GPU: hc_temporal (srt_temporal_accumulate's per-pixel function
of csrc/rt_denoise.h compiled for the CPU, tests/temporal_host.py) against the restatement in
tests/temporal_ref.py, the cases the definition singles out, what the accumulation buys on the cornell fixture,
Scene.render's new keys and create_animation's keyword.  Floats within rtol 1e-5 / atol 1e-12."""
import numpy as np
import pytest

import denoise_var_ref as VR
import scenes
import temporal_host as TH
import temporal_ref as TR
from denoise_ref import SHAPES


# ---- a. against the restatement, with the pixels that are copied through ------------------------------------
@pytest.mark.parametrize("with_history", (False, True))
@pytest.mark.parametrize("demodulate", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_hostcheck_matches_the_restatement(shape, demodulate, with_history):
    W, H = shape
    TR.check_against_restatement(TH.accumulate, W, H, demodulate, with_history)


def test_restatement_first_frame_is_the_input():
    s = TR.random_sequence(70, 9, 1)
    for run in (TR.accumulate, TH.accumulate):
        out = run(s["A"], s["B"], s["guides"], 70, 9)
        assert TR.same_bits(out["a"], s["A"]) and TR.same_bits(out["b"], s["B"])
        assert TR.same_bits(out["hist_a"], s["A"]) and TR.same_bits(out["hist_b"], s["B"])
        bad = (s["guides"]["hit_id"] < 0)
        bad[[s["inf"], s["nan"]]] = True
        assert np.array_equal(out["len"], np.where(bad, 0.0, 1.0))


# ---- b. the cases with a known answer ------------------------------------------------------------------------
@pytest.mark.parametrize("columns", (1, -1))
def test_hostcheck_exact_shift(columns):
    TR.check_exact_shift(TH.accumulate, columns)
    TR.check_exact_shift(TR.accumulate, columns)


def test_hostcheck_static_camera_gives_the_arithmetic_mean():
    """Measured on the CPU: largest relative deviation 1.1e-10 against the bound 1e-8."""
    TR.check_static_mean(TH.accumulate)


def test_hostcheck_max_history_clamps():
    TR.check_max_history(TH.accumulate)
    TR.check_max_history(TR.accumulate)


# ---- c. arguments ------------------------------------------------------------------------------------------------
BAD = [dict(max_history=0), dict(normal_max=-0.1), dict(plane_max=-1.0), dict(normal_max=float("nan")),
       dict(plane_max=float("inf"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_hostcheck_refuses_bad_arguments(bad):
    s = TR.random_sequence(5, 3, 1)
    with pytest.raises(ValueError):
        TH.accumulate(s["A"], s["B"], s["guides"], 5, 3, history=s["history"], prev_cam=s["prev_cam"], **bad)


# ---- d. quality on the fixture -------------------------------------------------------------------------------
# E / E(the last frame's unfiltered mean) on the four-frame cornell fixture by the restatement, on the CPU:
#   accumulated (demodulate), no filter (levels 0):            RATIO_LEVELS_0
#   accumulated, variance + demodulate, levels 3:              RATIO_LEVELS_3
#   the last frame alone, variance + demodulate, levels 3:     0.7926 (tests/test_denoise_var.py RATIO_LEVELS_3)
RATIO_LEVELS_0 = 0.22914871885517754
RATIO_LEVELS_3 = 0.192383505904628


def test_temporal_accumulation_on_the_cornell_fixture():
    new, alone = TR.fixture_error_ratios(TR.accumulate, VR.denoise_var)
    print("E / E(mean of the last frame): accumulated", new, "the last frame alone", alone)
    assert new[3] <= 0.5 * alone[3]
    assert new[0] <= RATIO_LEVELS_0 * 1.05 and new[3] <= RATIO_LEVELS_3 * 1.05
    # hc_temporal's accumulation, filtered by the restatement
    host, _ = TR.fixture_error_ratios(TH.accumulate, VR.denoise_var, levels=(3,))
    assert host[3] <= 0.5 * alone[3] and host[3] <= RATIO_LEVELS_3 * 1.05


def test_fixture_pixels_find_history():
    """Nearly every surface pixel of the fixture's last frame finds history in the frame before it: the 6-unit
    slide moves a surface 800 units away by about 0.7 pixel, so only pixels on a silhouette can lose theirs (a few
    dozen of 3600; the bound leaves room for 36).  Measured: 0.99917."""
    frames = TR.fixture_frames()
    (A0, B0, g0, c0), (A1, B1, g1, _) = frames[2], frames[3]
    first = TR.accumulate(A0, B0, g0, 64, 64)
    info = {}
    TR.accumulate(A1, B1, g1, 64, 64, history=TR.next_history(first, g0), prev_cam=c0, info=info)
    surface = (g1["normal"] != 0.0).any(axis=0)
    share = info["has"][surface].mean()
    print("share of surface pixels with history:", share)
    assert share >= 0.99


# ---- e. Scene.render's new keys ------------------------------------------------------------------------------
def test_denoise_params_temporal_keys():
    from sightpy import _backend as B

    base = dict(VR.DEFAULTS, variance=False, demodulate=False)
    t = {"temporal": True, "max_history": 32, "temporal_normal": 0.1, "temporal_plane": 0.02}
    assert B.denoise_params({"temporal": True}) == dict(base, **t)
    assert B.denoise_params({"temporal": True, "variance": True, "demodulate": True, "max_history": 8,
                             "temporal_normal": 0.2, "temporal_plane": 0}) == dict(
        base, variance=True, demodulate=True, temporal=True, max_history=8, temporal_normal=0.2, temporal_plane=0.0)
    # off: today's dictionaries, whatever the other temporal keys say
    assert B.denoise_params({"temporal": False, "max_history": 4}) == B.denoise_params(True)
    assert B.denoise_params({"variance": True, "temporal_plane": 0.5}) == dict(base, variance=True)


@pytest.mark.parametrize("spec", [{"temporal": 1}, {"temporal": True, "max_history": 0},
                                  {"temporal": True, "max_history": 2.5}, {"temporal": True, "max_history": True},
                                  {"temporal": True, "temporal_normal": -0.1},
                                  {"temporal": True, "temporal_plane": float("nan")},
                                  {"temporal": True, "temporal_plane": float("inf")}, {"max_history": 0},
                                  {"temporal": True, "temporal_normals": 0.1}])
def test_render_refuses_bad_temporal_keys_before_any_launch(spec, monkeypatch):
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(2, denoise=spec)


def test_render_temporal_refusals_are_the_half_frame_paths(monkeypatch):
    import plugin_scenes
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(1, denoise={"temporal": True})
    with pytest.raises(NotImplementedError):
        plugin_scenes.scene("texture", 16, 12).render(2, denoise={"temporal": True})
    monkeypatch.setenv("SIGHTPY_DEVICES", "0,1")
    with pytest.raises(NotImplementedError):
        scenes.cornell(24, 24).render(2, denoise={"temporal": True})
    scenes.cornell(24, 24).reset_history()  # nothing to drop, nothing reached


# ---- f. create_animation's keyword ---------------------------------------------------------------------------
class StubScene:
    """Records how the frame loop calls the scene."""

    def __init__(self):
        self.calls = []

    def render(self, *args, **kw):
        from PIL import Image

        self.calls.append(("render", args, kw))
        return Image.new("RGB", (4, 3))

    def reset_history(self):
        self.calls.append(("reset_history", (), {}))


def test_create_animation_without_denoise_calls_render_as_before(tmp_path, monkeypatch):
    from sightpy import create_animation

    monkeypatch.chdir(tmp_path)
    for kw in ({}, {"denoise": False}, {"denoise": None}):
        sc = StubScene()
        create_animation(sc, 3, 2, 0.0, 1.0, lambda scene, t: None, "a", **kw)
        assert sc.calls == [("render", (3,), {})] * 2


def test_create_animation_with_denoise_resets_once_and_passes_it_on(tmp_path, monkeypatch):
    from sightpy import create_animation

    monkeypatch.chdir(tmp_path)
    sc = StubScene()
    dn = {"temporal": True, "demodulate": True}
    create_animation(sc, 3, 3, 0.0, 1.0, lambda scene, t: None, "a", denoise=dn)
    assert sc.calls == [("reset_history", (), {})] + [("render", (3,), {"denoise": dn})] * 3
    assert sorted(p.name for p in (tmp_path / "frames").iterdir()) == ["a_0.png", "a_1.png", "a_2.png"]
