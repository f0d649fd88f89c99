"""The uint8 pixel rule on the CPU: the oracle's srgb_u8 and the host build of resolve_pixel (rt_device.h,
through the host check harness) against the exact statement in tests/resolve_ref.py -- inside [lo, hi]
everywhere, the one right byte wherever the value is unambiguous, the special-value table, and no 255."""
import numpy as np
import pytest

import denoise_host as DH
import hostcheck as HC
import resolve_ref as R
import scenes
import sightpy_oracle as O


@pytest.fixture(scope="module")
def fr():
    return R.frame()


def _oracle(rgb):
    with np.errstate(all="ignore"):  # (the specials: NaN and inf on purpose)
        return O.srgb_u8(rgb, 1, rgb.shape[1])[0]


def _host(fr, rgbx):
    n = fr["W"] * fr["H"]
    guides = {"normal": np.zeros((3, n)), "albedo": np.zeros((3, n)), "position": np.zeros((3, n)),
              "depth": np.zeros(n)}
    out, u8 = DH.denoise(fr["rgb"], guides, fr["W"], fr["H"], levels=0, rgbx=rgbx)
    assert np.array_equal(out, fr["rgb"], equal_nan=True) and np.array_equal(np.signbit(out), np.signbit(fr["rgb"]))
    u8 = u8.reshape(n, -1)
    if rgbx:
        assert np.all(u8[:, 3] == 255)
    return u8[:, :3]


def _check_frame(fr, u8, what):
    """Every assertion of the frame on one evaluation of the rule; returns the count of u8 != floor(q)."""
    R.check_bytes(u8, fr["lo"], fr["hi"], what)  # (the special pixels' lo == hi == SPECIALS' bytes)
    assert np.array_equal(u8[fr["special"]], fr["special_bytes"]), what
    assert u8[R.never_255(fr["rgb"])].max() == 254, what
    return int((u8.astype(np.int64) != fr["floor"]).sum())


def test_the_table_is_a_boundary_table(fr):
    """The table sits on the level boundaries -- a good part of it is ambiguous at EPS -- and still at least
    0.4 of its values (the zeros of the black channels not counted) have one right byte; the random set has
    no ambiguous value at all."""
    lo, hi = fr["lo"][fr["table"]], fr["hi"][fr["table"]]
    placed = fr["rgb"][:, fr["table"]].T != 0.0
    amb = (lo != hi) & placed
    share = 1.0 - amb.sum() / placed.sum()
    print("table: %d pixels, %d placed values, %d ambiguous, unambiguous share %.3f" % (
        lo.shape[0], placed.sum(), amb.sum(), share))
    assert lo.shape[0] > 20000 and 0.4 <= share <= 0.8
    assert ((hi - lo) >= 0).all() and ((hi - lo) <= 1).all()
    rl, rh = fr["lo"][fr["random"]], fr["hi"][fr["random"]]
    assert rl.shape == (6000, 3) and np.array_equal(rl, rh)
    # every level 1 .. 254 starts in the table, on the branch it belongs to
    xs = R.level_starts()
    assert len(xs) == 254 and (np.diff(xs) > 0).all()
    assert (xs[:R.LINEAR_LEVELS] <= 0.00304).all() and (xs[R.LINEAR_LEVELS:] > 0.00304).all()
    lo_s, hi_s, fl_s = R.classify(np.stack([xs, np.zeros(254), np.zeros(254)]))
    lo_p, hi_p, fl_p = R.classify(np.stack([np.nextafter(xs, 0.0), np.zeros(254), np.zeros(254)]))
    assert np.array_equal(fl_s[:, 0], np.arange(1, 255)) and np.array_equal(fl_p[:, 0], np.arange(0, 254))
    # and, divided by a peak of 1.825, in the normalised regime
    ns = R.normalised_level_starts()[:, :254]
    below = ns.copy()
    below[1] = np.nextafter(below[1], 0.0)
    assert np.array_equal(R.classify(ns)[2][:, 1], np.arange(1, 255))
    assert np.array_equal(R.classify(below)[2][:, 1], np.arange(0, 254))
    # the branch probes: one right byte, 10, where the linear branch carried past 0.00304 would give 9
    pr = R.branch_probes()
    lo_b, hi_b = R.bounds(pr)
    assert np.array_equal(lo_b, hi_b) and (lo_b[:, 1] == 10).all() and (lo_b[:, 0] == 254).all()
    assert ((255.0 * (12.92 * pr[1]) / (1.055 * pr[0] ** (1.0 / 2.4) - 0.055 + 0.00001)).astype(int) == 9).all()
    assert np.array_equal(fr["rgb"][:, fr["table"]][:, -pr.shape[1]:], pr)


def test_bounds_refuses_what_it_does_not_classify():
    for bad in (np.nan, np.inf, -np.inf, -1.0, -0.0):
        with pytest.raises(ValueError):
            R.bounds(np.array([[0.5], [bad], [0.25]]))
    lo, hi = R.bounds(np.array([[0.0, 0.25], [5e-324, 0.25], [1.0, 4.0]]))
    assert lo.tolist() == [[0, 0, 254], [75, 75, 254]] and np.array_equal(lo, hi)


def test_oracle_srgb_u8_is_the_exact_rule(fr):
    u8 = _oracle(fr["rgb"])
    off = _check_frame(fr, u8, "oracle")
    print("oracle: %d values, %d differ from floor(exact q)" % (u8.size, off))
    # (beyond never_255: m + 1e-5 == m in float64, and numpy itself gives 255)
    assert _oracle(np.array([[1e300], [0.0], [0.0]]))[0].tolist() == [255, 0, 0]


@pytest.mark.parametrize("rgbx", [False, True], ids=["rgb", "rgbx"])
def test_host_resolve_pixel_is_the_exact_rule(fr, rgbx):
    u8 = _host(fr, rgbx)
    off = _check_frame(fr, u8, "host resolve_pixel")
    print("host resolve_pixel: %d values, %d differ from floor(exact q)" % (u8.size, off))


def test_host_render_bytes_are_the_rule_on_its_own_rgb():
    """hc_render's uint8 image against its own linear RGB (example1, 13 x 7, 3 spp): no value of a rendered
    frame is ambiguous, so every byte is pinned."""
    sc = scenes.example1(13, 7, 3)
    np.random.seed(5)
    jit = sc.camera.draw_jitter(3)
    rgb, u8, _, _ = HC.render(sc, jit, seed=1)
    lo, hi = R.bounds(rgb)
    assert np.array_equal(lo, hi)
    R.check_bytes(u8, lo, hi, "hc_render")
    assert len(np.unique(u8)) > 20  # (a picture, not a constant)
