"""Per-collider motion in the temporal accumulation, without a GPU: hc_temporal with a motion table
(temporal_pixel<true> of csrc/rt_denoise.h compiled for the CPU, tests/temporal_motion_host.py) against the
restatement in tests/temporal_motion_ref.py and the cases with a known answer, sightpy/_motion.py's
collider_motion on colliders built through the public classes, the moving sphere of example1, and
denoise_params' "motion" key.  Floats within rtol 1e-5 / atol 1e-12."""
import numpy as np
import pytest

import denoise_ref as DR
import scenes
import temporal_motion_host as MH
import temporal_motion_ref as MR
import temporal_ref as TR
from denoise_ref import SHAPES


# ---- a. the cases with a known answer ------------------------------------------------------------------------
@pytest.mark.parametrize("columns", (1, -1))
def test_hostcheck_exact_shift_by_motion(columns):
    MR.check_exact_shift_by_motion(MH.accumulate, columns)
    MR.check_exact_shift_by_motion(MR.accumulate, columns)


def test_hostcheck_rotation_the_normal_test_refuses_without_the_row():
    MR.check_rotation(MH.accumulate)
    MR.check_rotation(MR.accumulate)


def test_hostcheck_identity_and_unknown_rows():
    MR.check_identity_and_unknown_rows(MH.accumulate)
    MR.check_identity_and_unknown_rows(MR.accumulate)


# ---- b. against the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("demodulate", (False, True))
@pytest.mark.parametrize("shape", SHAPES)
def test_hostcheck_matches_the_restatement_with_motion(shape, demodulate):
    W, H = shape
    MR.check_against_restatement(MH.accumulate, W, H, demodulate)


def test_a_first_frame_ignores_the_table():
    s = MR.moving_sequence(70, 9, 3)
    got = MH.accumulate(s["A"], s["B"], s["guides"], 70, 9, motion=s["motion"])
    want = MH.accumulate(s["A"], s["B"], s["guides"], 70, 9)
    assert all(TR.same_bits(got[k], want[k]) for k in TR.OUTPUTS)


# ---- c. arguments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_motion", (0, -1))
def test_hostcheck_refuses_a_table_without_rows(n_motion):
    s = TR.random_sequence(5, 3, 1)
    kw = dict(history=s["history"], prev_cam=s["prev_cam"], motion=MR.identity_rows(3))
    MH.accumulate(s["A"], s["B"], s["guides"], 5, 3, **kw)
    with pytest.raises(ValueError):
        MH.accumulate(s["A"], s["B"], s["guides"], 5, 3, n_motion=n_motion, **kw)


# ---- d. collider_motion ------------------------------------------------------------------------------------------
def _table(*colliders):
    from sightpy import _native as N
    from sightpy._lower import collider_record

    t = np.zeros(len(colliders), dtype=N.COLLIDER_DTYPE)
    for i, c in enumerate(colliders):
        t[i] = collider_record(c)
    return t


def _f3(v):
    return np.array([float(v.x), float(v.y), float(v.z)])


LOCAL = np.array([[0.3, -0.2, 0.1], [-1.0, 0.5, 0.0], [0.0, 0.0, 0.0], [0.25, 0.75, -0.5]])


def _points(c):
    """The points with the local coordinates LOCAL on the collider `c` as it stands."""
    kind = type(c).__name__
    if kind == "Sphere_Collider":
        o, F = _f3(c.center), np.eye(3)
    elif kind == "Plane_Collider":
        o, F = _f3(c.center), np.stack([_f3(c.u_axis), _f3(c.v_axis), _f3(c.normal)], axis=1)
    elif kind == "Cuboid_Collider":
        o, F = _f3(c.center), np.stack([_f3(c.ax_w), _f3(c.ax_h), _f3(c.ax_l)], axis=1)
    else:
        p1 = _f3(c.p1)
        o, F = p1, np.stack([_f3(c.p2) - p1, _f3(c.p3) - p1, _f3(c.normal)], axis=1)
    return o + LOCAL @ F.T


def _apply(row, P):
    return P @ row[:9].reshape(3, 3).T + row[9:]


def _gold():
    from sightpy import Glossy, rgb, vec3

    return Glossy(diff_color=rgb(1.0, 0.5, 0.2), n=vec3(1.3 + 1.91j, 1.3 + 1.91j, 1.4 + 2.91j), roughness=0.2,
                  spec_coeff=0.5, diff_coeff=0.3)


def _objects():
    from sightpy import Cuboid, Plane, Sphere, Triangle, vec3

    return [Sphere(material=_gold(), center=vec3(-0.75, 0.1, -3.0), radius=0.6),
            Plane(material=_gold(), center=vec3(0.5, -0.5, -3.0), width=4.0, height=2.0, u_axis=vec3(1.0, 0, 0),
                  v_axis=vec3(0, 0, -1.0)),
            Cuboid(material=_gold(), center=vec3(0.0, 0.3, -0.8), width=0.9, height=1.0, length=0.4),
            Triangle(center=vec3(0.0, 0.0, 0.0), material=_gold(), p1=vec3(0.0, 0.0, -2.0), p2=vec3(1.0, 0.2, -2.5),
                     p3=vec3(0.3, 1.1, -1.9)),
            Sphere(material=_gold(), center=vec3(1.25, 0.1, -3.0), radius=0.5)]


def _shift(c, d):
    """Translate the collider `c` by the vec3 `d`."""
    if type(c).__name__ == "Triangle_Collider":
        c.p1, c.p2, c.p3, c.centroid = c.p1 + d, c.p2 + d, c.p3 + d, c.centroid + d
        c.center = c.centroid
    else:
        c.center = c.center + d


def test_collider_motion_maps_local_points_back():
    """A translated Sphere, a Plane, a Cuboid and a Triangle after rotate(theta, u) and a shift: points with fixed
    local coordinates in the current frame map to the same local coordinates in the previous frame within 1e-12;
    the Sphere that was not touched gets the identity row exactly."""
    from sightpy import vec3
    from sightpy._motion import IDENTITY, collider_motion, count_rows

    objs = _objects()
    cols = [o.collider_list[0] for o in objs]
    prev = _table(*cols)
    before = [_points(c) for c in cols]
    _shift(cols[0], vec3(1.0 / 3, 0.0, 0.0))
    for o, (theta, u, d) in zip(objs[1:4], ((25.0, vec3(0.0, 1.0, 0.0), vec3(0.2, 0.0, -0.1)),
                                            (-40.0, vec3(1.0, 2.0, 0.5), vec3(-0.3, 0.1, 0.0)),
                                            (70.0, vec3(0.3, -1.0, 0.2), vec3(0.05, 0.4, 0.3)))):
        o.rotate(theta, u)
        _shift(o.collider_list[0], d)
    cur = _table(*cols)
    rows = collider_motion(prev, cur)
    assert rows.shape == (5, 12) and rows.dtype == np.float64
    for i in range(4):
        now = _points(cols[i])
        assert np.abs(now - before[i]).max() > 0.05
        dev = np.abs(_apply(rows[i], now) - before[i]).max()
        print(type(cols[i]).__name__, "largest deviation", dev)
        assert dev <= 1e-12
    assert np.array_equal(rows[0, :9], IDENTITY[:9])
    assert np.array_equal(rows[4], IDENTITY)
    assert count_rows(rows) == (4, 0)
    # a table against itself: every record unchanged
    assert np.array_equal(collider_motion(cur, cur), np.tile(IDENTITY, (5, 1)))


def test_collider_motion_unknown_rows():
    from sightpy import vec3
    from sightpy._motion import IDENTITY, collider_motion, count_rows

    objs = _objects()
    cols = [o.collider_list[0] for o in objs]
    prev = _table(*cols)
    cols[0].radius = 0.7                      # a changed radius
    cols[1].w = cols[1].w * 1.5               # a changed width
    cols[2].height = 1.25                     # a changed size
    cols[3].p3 = cols[3].p3 + vec3(0.0, 0.5, 0.0)  # a stretched triangle
    rows = collider_motion(prev, _table(*cols))
    assert np.isnan(rows[:4]).all() and np.array_equal(rows[4], IDENTITY)
    assert count_rows(rows) == (0, 4)
    # another type at the index
    rows = collider_motion(prev, _table(cols[4], *cols[1:]))
    assert np.isnan(rows[0]).all()
    # tables of different lengths, either way
    for a, b in ((prev, prev[:4]), (prev[:4], prev)):
        rows = collider_motion(a, b)
        assert rows.shape == (len(b), 12) and np.isnan(rows).all()


# ---- e. the moving sphere of example1 --------------------------------------------------------------------------
def test_moving_sphere_finds_history_by_its_row():
    """example1 at 64 x 48, depth 3, a static camera, the gold sphere moved by 1/3 unit: without the table none
    of the sphere's pixels finds history (measured 0.0 of 80), with it at least 0.95 do (measured 1.0); the
    share for every other surface pixel is the same with and without (measured 0.98672).  The table comes from
    collider_motion on the two lowered collider tables and equals the restatement's derivation from the objects."""
    from sightpy import vec3
    from sightpy._lower import lower_scene
    from sightpy._motion import collider_motion, count_rows

    W, H = 64, 48
    n = W * H
    sc = scenes.example1(W, H, 3)
    g0, t0, s0 = DR.aovs(sc), lower_scene(sc).colliders.copy(), MR.snapshot(sc)
    sc.collider_list[0].center = vec3(-0.75 + 1.0 / 3, 0.1, -3.0)
    g1, t1, s1 = DR.aovs(sc), lower_scene(sc).colliders.copy(), MR.snapshot(sc)
    cam = TR.camera_dict(sc.camera)
    rows = collider_motion(t0, t1)
    assert count_rows(rows) == (1, 0)
    np.testing.assert_allclose(rows, MR.object_motion(s0, s1), rtol=0, atol=1e-15)
    rng = np.random.default_rng(1)
    A0, B0, A1, B1 = (0.2 + rng.random((3, n)) for _ in range(4))
    hist = TR.next_history(TR.accumulate(A0, B0, g0, W, H), g0)
    sphere = g1["hit_id"] == 0
    others = (g1["normal"] != 0.0).any(axis=0) & ~sphere
    assert sphere.sum() > 60
    shares = {}
    for name, motion in (("without", None), ("with", rows)):
        info = {}
        MR.accumulate(A1, B1, g1, W, H, history=hist, prev_cam=cam, motion=motion, info=info)
        got = MH.accumulate(A1, B1, g1, W, H, history=hist, prev_cam=cam, motion=motion)
        assert np.array_equal(got["len"] > 1.0, info["has"])
        shares[name] = (float(info["has"][sphere].mean()), float(info["has"][others].mean()))
        print("history found", name, "the table: sphere %.5f (of %d pixels), other surfaces %.5f" %
              (shares[name][0], sphere.sum(), shares[name][1]))
    assert shares["without"][0] == 0.0
    assert shares["with"][0] >= 0.95
    assert shares["with"][1] == shares["without"][1]


# ---- f. Scene.render's new key ---------------------------------------------------------------------------------
def test_denoise_params_motion_key():
    from sightpy import _backend as B

    p = B.denoise_params({"temporal": True, "motion": True})
    assert p["motion"] is True and p == dict(B.denoise_params({"temporal": True}), motion=True)
    assert "motion" not in B.denoise_params({"temporal": True})
    assert "motion" not in B.denoise_params({"temporal": True, "motion": False})
    assert B.denoise_params({"motion": True}) == B.denoise_params(True)
    assert B.denoise_params({"variance": True, "motion": True}) == B.denoise_params({"variance": True})


@pytest.mark.parametrize("spec", [{"temporal": True, "motion": 1}, {"temporal": True, "motion": "yes"}, {"motion": 0},
                                  {"temporal": True, "motion": None}])
def test_render_refuses_a_bad_motion_key_before_any_launch(spec, monkeypatch):
    from sightpy import _backend as B

    monkeypatch.setattr(B, "context", lambda: pytest.fail("the device was reached"))
    with pytest.raises(ValueError):
        scenes.cornell(24, 24).render(2, denoise=spec)
