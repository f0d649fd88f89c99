"""Device-posed triangle meshes (TriangleMesh.set_pose -> srt_pose_colliders, csrc/rt_pose.h), without a GPU:
the record and refit functions the kernels run, compiled for the CPU (rt_hostcheck.cpp), against the numpy
restatement in mesh_pose_ref.py and `collider_record`; the lowering cache; set_pose's checks; the motion rows of
a pose pair.  The GPU versions are in test_gpu_mesh_pose.py."""
import numpy as np
import pytest

import hostcheck as HC
import mesh_pose_ref as MP
import scenes
import test_mesh
import vattr_ref as VR
from sightpy import _lower, _motion
from sightpy import _native as N
from sightpy.geometry.triangle_mesh import TriangleMesh

SKEW = MP.rotation(40.0, (1.0, 2.0, 0.5))
SHIFT = (0.3, -0.2, 0.15)
QUARTER = MP.rotation(90.0, (1.0, 2.0, 0.5))


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_pose")
    out = {}
    for sub in (1, 2):
        out["ico%d" % sub] = str(d / ("ico%d.obj" % sub))
        scenes.write_icosphere_obj(out["ico%d" % sub], subdiv=sub)
    out["smooth"] = str(d / "smooth.obj")
    VR.write_smooth_icosphere_obj(out["smooth"], 1)
    return out


def _mesh(sc):
    return next(p for p in sc.scene_primitives if isinstance(p, TriangleMesh))


def _mesh_range(sc):
    L = _lower.lower_scene(sc)
    tri = np.flatnonzero(L.colliders["type"] == N.TRIANGLE)
    return int(tri[0]), len(tri)


def _same_values(a, b):
    """Equal field by field; the sign of a zero may differ (as in the motion rows)."""
    return all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


@pytest.mark.parametrize("kind", ["flat", "smooth", "textured"])
def test_posed_records_equal_collider_record_of_restated_vertices(objs, kind):
    if kind == "flat":
        sc = scenes.mesh_scene(objs["ico1"])
    else:
        sc = VR.mesh_scene(objs["smooth"], smooth=True, texcoords=kind == "textured",
                           material=VR.checker() if kind == "textured" else None)
    mesh = _mesh(sc)
    rest = MP.records(mesh.collider_list)
    flags = N.CF_VNORMAL | (N.CF_VUV if kind == "textured" else 0) if kind != "flat" else 0
    assert (rest["flags"] == flags).all() and len(rest) == 80
    mesh.set_pose(SKEW, SHIFT)
    pose = mesh.pose
    c = np.array([mesh.center.x, mesh.center.y, mesh.center.z])
    assert np.array_equal(pose, MP.pose_numbers(SKEW, c, SHIFT))
    assert np.array_equal(mesh.posed_vertices(), MP.posed_vertices(MP.mesh_arrays(mesh)[0], pose))
    want = MP.records(MP.restated_mesh(mesh).collider_list)
    got = MP.hc_pose_triangles(rest, pose)
    assert _same_values(got, want)
    assert not np.array_equal(got["p"][:, 6:15], rest["p"][:, 6:15])
    # the identity pose gives the rest records back
    assert _same_values(MP.hc_pose_triangles(rest, MP.IDENTITY), rest)
    mesh.reset_pose()
    assert mesh.pose is None and np.array_equal(mesh.posed_vertices(), mesh.rest_vertices())


@pytest.mark.parametrize("which", ["ico1", "ico2"])
def test_refit_under_identity_gives_the_built_nodes(objs, which):
    sc = scenes.mesh_scene(objs[which])
    first, count = _mesh_range(sc)
    built, tri0, col0, bound0 = MP.hc_bvh_refit(sc, [])
    nodes, tri, col, bound = MP.hc_bvh_refit(sc, [(first, count, MP.IDENTITY)])
    assert len(built) > 4 and built.tobytes() == nodes.tobytes()
    assert np.array_equal(tri, tri0) and col.tobytes() == col0.tobytes() and bound == bound0


def _check_boxes(nodes, tri, col):
    """Every triangle vertex inside the box of its leaf slot and of every slot above it; returns the triangles seen."""
    def below(node, k):
        ch, cnt = int(nodes["child"][node, k]), int(nodes["count"][node, k])
        if ch == MP.BVH_EMPTY:
            return []
        ids = list(tri[-ch - 1:-ch - 1 + cnt]) if ch < 0 else [i for j in range(4) for i in below(ch, j)]
        v = col["p"][ids, 6:15].reshape(-1, 3)
        lo, hi = nodes["lo"][node, :, k].astype(np.float64), nodes["hi"][node, :, k].astype(np.float64)
        assert (v >= lo).all() and (v <= hi).all(), (node, k)
        return ids

    return sorted(i for k in range(4) for i in below(0, k))


@pytest.mark.parametrize("which", ["ico1", "ico2"])
def test_refit_under_a_quarter_turn_about_a_skew_axis(objs, which):
    sc = scenes.mesh_scene(objs[which])
    mesh = _mesh(sc)
    first, count = _mesh_range(sc)
    mesh.set_pose(QUARTER, SHIFT)
    ranges = [(first, count, mesh.pose)]
    nodes, tri, col, bound = MP.hc_bvh_refit(sc, ranges)
    built = MP.hc_bvh_refit(sc, [])[0]
    assert np.array_equal(nodes["child"], built["child"]) and np.array_equal(nodes["count"], built["count"])
    assert not np.array_equal(nodes["lo"], built["lo"])
    assert np.array_equal(col["p"][first:first + count, 6:15].reshape(-1, 3, 3), mesh.posed_vertices())
    assert _check_boxes(nodes, tri, col) == list(range(first, first + count))
    finite = np.isfinite(nodes["lo"])
    assert bound >= max(np.abs(nodes["lo"][finite]).max(), np.abs(nodes["hi"][finite]).max())
    # nearest hits through the refitted tree against the linear loop over the posed table, and against the
    # host harness on the scene restated with the posed vertices (its own build)
    restated = MP.restated_scene(sc)
    Oa, Da = test_mesh._probe_rays(restated, np.random.default_rng(11), n=3000)
    HC.set_bvh(1)
    tb, ib, ob = MP.hc_pose_nearest(sc, ranges, Oa, Da)
    tr, ir, orr = HC.nearest(restated, Oa, Da)
    HC.set_bvh(0)
    try:
        tl, il, ol = MP.hc_pose_nearest(sc, ranges, Oa, Da)
    finally:
        HC.set_bvh(1)
    for t, i, o in ((tl, il, ol), (tr, ir, orr)):
        assert np.array_equal(ib, i)
        assert np.array_equal(tb, t, equal_nan=True)
        assert np.array_equal(ob, o, equal_nan=True)
    assert ((ib >= first) & (ib < first + count)).mean() > 0.3  # the probe hits the posed mesh a lot


def test_lowering_takes_a_posed_mesh_from_its_cache(objs, monkeypatch):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _mesh(sc)
    calls = []
    real = _lower.collider_record
    monkeypatch.setattr(_lower, "collider_record", lambda c: (calls.append(c), real(c))[1])
    plain = _lower.lower_scene(sc)
    others = len(sc.collider_list) - 80
    assert len(calls) == len(sc.collider_list) and others == 3 and plain.posed == []
    mesh.set_pose(SKEW, SHIFT)
    del calls[:]
    first = _lower.lower_scene(sc)
    assert len(calls) == len(sc.collider_list)  # the cache is filled
    assert first.colliders.tobytes() == plain.colliders.tobytes()  # the table keeps the rest pose ...
    assert first.signature() == plain.signature()  # ... and the poses are no part of the signature
    assert [(p["first"], p["count"]) for p in first.posed] == [(1, 80)]
    assert np.array_equal(first.posed[0]["pose"], mesh.pose)
    mesh.set_pose(QUARTER)
    del calls[:]
    second = _lower.lower_scene(sc)
    assert len(calls) == others and not any(type(c).__name__ == "Triangle_Collider" for c in calls)
    assert second.colliders.tobytes() == plain.colliders.tobytes() and second.signature() == plain.signature()
    assert np.array_equal(second.posed[0]["pose"], mesh.pose)
    mesh.reset_pose()
    assert np.array_equal(_lower.lower_scene(sc).posed[0]["pose"], MP.IDENTITY)
    mesh.invalidate()
    del calls[:]
    _lower.lower_scene(sc)
    assert len(calls) == len(sc.collider_list)
    # rotate() edits the Python colliders and invalidates
    from sightpy import vec3

    mesh.rotate(20.0, vec3(0.0, 1.0, 0.0))
    del calls[:]
    turned = _lower.lower_scene(sc)
    assert len(calls) == len(sc.collider_list) and turned.signature() != plain.signature()


def test_set_pose_validation(objs):
    mesh = _mesh(scenes.mesh_scene(objs["ico1"]))
    bad = [np.eye(3) * 1.001, np.diag([1.0, 1.0, -1.0]), np.eye(4), np.eye(3)[:2], SKEW + 1e-6,
           np.full((3, 3), np.nan)]
    for R in bad:
        with pytest.raises(ValueError):
            mesh.set_pose(R)
    with pytest.raises(ValueError):
        mesh.set_pose(np.eye(3), (1.0, 2.0))
    assert mesh.pose is None and not mesh._device_posed
    mesh.set_pose(SKEW.tolist(), [0, 0, 1])
    assert mesh.pose.shape == (12,) and mesh._device_posed


def test_motion_rows_of_a_pose_pair(objs):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _mesh(sc)
    mesh.set_pose(SKEW, SHIFT)
    prev = _lower.lower_scene(sc)
    prev_pts = mesh.posed_vertices().reshape(-1, 3)
    mesh.set_pose(QUARTER, (0.0, 0.4, -0.1))
    cur = _lower.lower_scene(sc)
    cur_pts = mesh.posed_vertices().reshape(-1, 3)
    rows = _motion.collider_motion(prev.colliders, cur.colliders)
    assert (rows == _motion.IDENTITY).all()  # the records alone call the mesh static
    _motion.pose_motion(rows, prev.posed, cur.posed)
    sl = slice(1, 81)
    assert (rows[sl] == rows[1]).all() and (rows[0] == _motion.IDENTITY).all() and (rows[81:] == _motion.IDENTITY).all()
    R, t = rows[1, :9].reshape(3, 3), rows[1, 9:]
    assert np.abs(cur_pts @ R.T + t - prev_pts).max() <= 1e-12
    assert _motion.count_rows(rows) == (80, 0)
    # the same pose twice: the identity, exactly
    same = _motion.pose_motion(_motion.collider_motion(cur.colliders, cur.colliders), cur.posed, cur.posed)
    assert (same == _motion.IDENTITY).all()
    # invalidated between the frames, or posed in the current frame only: no pose pair
    mesh.invalidate()
    after = _lower.lower_scene(sc)
    rows = _motion.pose_motion(_motion.collider_motion(cur.colliders, after.colliders), cur.posed, after.posed)
    assert np.isnan(rows[sl]).all() and _motion.count_rows(rows) == (0, 80)
    rows = _motion.pose_motion(_motion.collider_motion(cur.colliders, after.colliders), [], after.posed)
    assert np.isnan(rows[sl]).all() and not np.isnan(rows[0]).any()


def test_a_posed_mesh_is_refused_in_a_hybrid_scene(objs):
    from sightpy import _hybrid

    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _mesh(sc)
    mesh.set_pose(SKEW)
    real = _hybrid.is_hybrid
    try:
        _hybrid.is_hybrid = lambda scene: True
        with pytest.raises(NotImplementedError, match="set_pose"):
            _lower.lower_scene(sc)
        mesh.reset_pose()
        _lower.lower_scene(sc)  # the rest pose is what the Python colliders hold
    finally:
        _hybrid.is_hybrid = real
