"""Device-deformed triangle meshes (TriangleMesh.set_vertices -> srt_deform_colliders, csrc/rt_deform.h), without a
GPU: the functions the kernels run, compiled for the CPU (rt_hostcheck.cpp), against `collider_record` of a mesh
reloaded from an OBJ file that holds the deformed vertices (mesh_deform_ref.py); the refit; the lowering cache;
set_vertices' checks; the motion rows.  The GPU versions are in test_gpu_mesh_deform.py."""
import numpy as np
import pytest

import hostcheck as HC
import mesh_deform_ref as MD
import mesh_pose_ref as MP
import scenes
import test_mesh
import vattr_ref as VR
from sightpy import _lower, _motion, vec3
from sightpy import _native as N
from sightpy.geometry.triangle_mesh import TriangleMesh

SKEW = MP.rotation(40.0, (1.0, 2.0, 0.5))
SHIFT = (0.3, -0.2, 0.15)


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_deform")
    out = {"dir": d}
    for sub in (1, 2):
        out["ico%d" % sub] = str(d / ("ico%d.obj" % sub))
        scenes.write_icosphere_obj(out["ico%d" % sub], subdiv=sub)
    out["vn"] = str(d / "vn.obj")
    VR.write_smooth_icosphere_obj(out["vn"], 1)
    out["uv"] = str(d / "uv.obj")  # the same with `v/vt` faces: texture coordinates, area-weighted normals
    with open(out["vn"]) as fi, open(out["uv"], "w") as fo:
        for line in fi:
            tok = line.split()
            if tok[0] == "f":
                fo.write("f " + " ".join("/".join(t.split("/")[:2]) for t in tok[1:]) + "\n")
            elif tok[0] != "vn":
                fo.write(line)
    return out


KINDS = {"flat": ("ico1", False, False), "smooth": ("ico1", True, False), "textured": ("uv", True, True),
         "vn": ("vn", True, True)}


def _scene(objs, kind, path=None):
    which, smooth, tex = KINDS[kind]
    return VR.mesh_scene(path or objs[which], smooth=smooth, texcoords=tex, material=VR.checker() if tex else None)


def _reloaded(objs, kind, P, name="deformed"):
    """The scene of `kind` with its mesh loaded from an OBJ holding the vertices P."""
    path = MD.write_deformed_obj(objs[KINDS[kind][0]], str(objs["dir"] / ("%s_%s.obj" % (name, kind))), P)
    return _scene(objs, kind, path)


def _equal(a, b):
    """Field by field with np.array_equal."""
    return all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


@pytest.mark.parametrize("kind", ["flat", "smooth", "textured", "vn"])
def test_deformed_records_equal_collider_record_of_the_reloaded_obj(objs, kind):
    mesh = MD.mesh_of(_scene(objs, kind))
    rest = MP.records(mesh.collider_list)
    assert len(rest) == 80 and mesh.file_vertices.shape == (42, 3) and mesh.corners.shape == (80, 3)
    flags = {"flat": 0, "smooth": N.CF_VNORMAL, "textured": N.CF_VNORMAL | N.CF_VUV, "vn": N.CF_VNORMAL | N.CF_VUV}[kind]
    assert (rest["flags"] == flags).all()
    assert mesh._recompute.all() == (kind in ("smooth", "textured")) and mesh._recompute.any() == mesh._recompute.all()
    # the file's own vertices give the rest records back
    assert _equal(MD.hc_deform_triangles(mesh, rest, mesh.file_vertices), rest)
    for name, fn in (("twist", MD.twist), ("bulge", MD.bulge)):
        P = fn(mesh.file_vertices)
        want = MP.records(MD.mesh_of(_reloaded(objs, kind, P, name)).collider_list)
        got = MD.hc_deform_triangles(mesh, rest, P)
        for f in got.dtype.names:
            assert np.array_equal(got[f], want[f]), (name, f)
        assert not np.array_equal(got["p"][:, 6:15], rest["p"][:, 6:15])
        if kind == "vn":  # the file's normals stay, everything else follows the vertices
            assert np.array_equal(got["p"][:, 24:33], rest["p"][:, 24:33])
            assert not np.array_equal(got["p"][:, 3:6], rest["p"][:, 3:6])
        elif kind != "flat":
            assert not np.array_equal(got["p"][:, 24:33], rest["p"][:, 24:33])
        if kind in ("textured", "vn"):
            assert np.array_equal(got["p"][:, 33:39], rest["p"][:, 33:39])
        # from the deformed records back to the file's: nothing of the earlier shape is left in them
        assert _equal(MD.hc_deform_triangles(mesh, got, mesh.file_vertices), rest)
    # the mesh's own view of the vertices the device renders
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    assert np.array_equal(mesh.deformed_vertices(), MD.hc_deform_triangles(mesh, rest, P)["p"][:, 6:15].reshape(-1, 3, 3))
    assert np.array_equal(mesh.vertices, P)
    mesh.reset_vertices()
    assert np.array_equal(mesh.deformed_vertices(), mesh.rest_vertices())


def test_a_vertex_whose_cross_products_cancel_gets_the_face_normal(objs):
    """Vertex 1 is named by two coincident, oppositely wound faces only: its sum is exactly zero, and each of its
    corners takes the face normal of its own face (of opposite sign in the two)."""
    path = str(objs["dir"] / "cancel.obj")
    V = [(0.0, 0.0, 0.0), (0.3, 0.1, 0.45), (0.5, 0.0, 0.1), (0.1, 0.5, 0.2), (-0.4, 0.2, 0.3)]
    F = [(2, 3, 4), (2, 4, 3), (1, 3, 4), (1, 4, 5), (3, 5, 4)]  # 1-based; vertex 2 (index 1): faces 0 and 1
    with open(path, "w") as fh:
        for v in V:
            fh.write("v %r %r %r\n" % v)
        for f in F:
            fh.write("f %d %d %d\n" % f)
    mesh = MD.mesh_of(VR.mesh_scene(path, smooth=True))
    rest = MP.records(mesh.collider_list)
    P = MD.twist(mesh.file_vertices, 100.0)
    cr = [np.cross(P[b] - P[a], P[c] - P[a]) for a, b, c in mesh.corners]
    assert np.array_equal(cr[0] + cr[1], np.zeros(3)) and np.abs(cr[0]).max() > 1e-3  # exactly zero, on the CPU
    dpath = MD.write_deformed_obj(path, str(objs["dir"] / "cancel_deformed.obj"), P)
    want = MP.records(MD.mesh_of(VR.mesh_scene(dpath, smooth=True)).collider_list)
    got = MD.hc_deform_triangles(mesh, rest, P)
    for f in got.dtype.names:
        assert np.array_equal(got[f], want[f]), f
    for face in (0, 1):  # corner 0 of faces 0 and 1 is vertex 1
        n = got["p"][face, 24:27]
        assert np.abs(n - got["p"][face, 3:6]).max() <= 4e-16 and abs(np.linalg.norm(n) - 1.0) <= 4e-16
    assert np.array_equal(got["p"][0, 3:6], -got["p"][1, 3:6])
    assert np.abs(got["p"][0, 27:30] - got["p"][0, 3:6]).max() > 1e-3  # vertex 2's normal is a sum of several faces'


def test_the_harness_refuses_a_corner_index_outside_the_vertices(objs):
    mesh = MD.mesh_of(_scene(objs, "flat"))
    rest = MP.records(mesh.collider_list)
    for bad in (42, -1):
        corners = mesh.corners
        corners[17, 2] = bad
        assert MD.hc_deform_triangles(mesh, rest, mesh.file_vertices, corners=corners) is None


def _check_boxes(nodes, tri, col):
    """Every triangle vertex inside the box of its leaf slot and of every slot above it; returns the triangles seen
    (test_mesh_pose._check_boxes' rule)."""
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
def test_refit_after_the_twist(objs, which):
    sc = scenes.mesh_scene(objs[which])
    mesh = MD.mesh_of(sc)
    first, count = MD.mesh_range(sc)
    built, tri0, col0, bound0 = MP.hc_bvh_refit(sc, [])
    # the file's own vertices: the uploaded records and the built nodes, bit for bit
    nodes, tri, col, bound = MD.hc_deform_refit(sc, 0, mesh.file_vertices)
    assert len(built) > 4 and nodes.tobytes() == built.tobytes() and np.array_equal(tri, tri0)
    assert all(np.array_equal(col[f], col0[f]) for f in col.dtype.names)
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    nodes, tri, col, bound = MD.hc_deform_refit(sc, 0, P)
    assert np.array_equal(nodes["child"], built["child"]) and np.array_equal(nodes["count"], built["count"])
    assert not np.array_equal(nodes["lo"], built["lo"])
    assert np.array_equal(col["p"][first:first + count, 6:15].reshape(-1, 3, 3), mesh.deformed_vertices())
    assert _check_boxes(nodes, tri, col) == list(range(first, first + count))
    finite = np.isfinite(nodes["lo"])
    assert bound >= max(np.abs(nodes["lo"][finite]).max(), np.abs(nodes["hi"][finite]).max())
    # nearest hits through the refitted tree against the linear loop over the rewritten table, and against the
    # harness's own build over the reloaded mesh
    path = MD.write_deformed_obj(objs[which], str(objs["dir"] / ("refit_%s.obj" % which)), P)
    reloaded = scenes.mesh_scene(path)
    Oa, Da = test_mesh._probe_rays(reloaded, np.random.default_rng(11), n=3000)
    HC.set_bvh(1)
    tb, ib, ob = MD.hc_deform_nearest(sc, 0, P, Oa, Da)
    tr, ir, orr = HC.nearest(reloaded, Oa, Da)
    HC.set_bvh(0)
    try:
        tl, il, ol = MD.hc_deform_nearest(sc, 0, P, Oa, Da)
    finally:
        HC.set_bvh(1)
    for t, i, o in ((tl, il, ol), (tr, ir, orr)):
        assert np.array_equal(ib, i)
        assert np.array_equal(tb, t, equal_nan=True)
        assert np.array_equal(ob, o, equal_nan=True)
    assert ((ib >= first) & (ib < first + count)).mean() > 0.3  # the probe hits the deformed mesh a lot


@pytest.mark.parametrize("kind", ["flat", "smooth"])
def test_deform_then_pose_equals_the_reloaded_mesh_posed(objs, kind):
    sc = _scene(objs, kind)
    mesh = MD.mesh_of(sc)
    first, count = MD.mesh_range(sc)
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    mesh.set_pose(SKEW, SHIFT)
    ref = MD.mesh_of(_reloaded(objs, kind, P, "posed"))
    ref.set_pose(SKEW, SHIFT)
    assert np.array_equal(mesh.pose, ref.pose)
    want_v = MP.posed_vertices(MP.mesh_arrays(ref)[0], ref.pose)
    assert np.array_equal(mesh.deformed_vertices(), want_v)
    want = MP.records(MP.restated_mesh(ref).collider_list)
    nodes, tri, col, bound = MD.hc_deform_refit(sc, 0, P, [(first, count, mesh.pose)])
    got = col[first:first + count]
    for f in ("type", "p"):  # (the scene's table carries the per-scene fields and flags besides)
        assert np.array_equal(got[f], want[f]), f
    attr = N.CF_VNORMAL | N.CF_VUV
    assert np.array_equal(got["flags"] & attr, want["flags"] & attr)
    assert _check_boxes(nodes, tri, col) == list(range(first, first + count))
    finite = np.isfinite(nodes["lo"])
    assert bound >= max(np.abs(nodes["lo"][finite]).max(), np.abs(nodes["hi"][finite]).max())
    # any order of the four calls
    mesh.reset_pose()
    assert np.array_equal(mesh.deformed_vertices(), MP.mesh_arrays(ref)[0])
    mesh.set_pose(SKEW, SHIFT)
    mesh.reset_vertices()
    assert np.array_equal(mesh.deformed_vertices(), mesh.posed_vertices())


def test_set_vertices_validation(objs):
    mesh = MD.mesh_of(_scene(objs, "flat"))
    P = mesh.file_vertices
    nan, inf = P.copy(), P.copy()
    nan[5, 1], inf[41, 2] = np.nan, -np.inf
    for bad in (P[:41], P.T, P.reshape(-1), np.zeros((42, 4)), np.zeros((43, 3)), nan, inf):
        with pytest.raises(ValueError):
            mesh.set_vertices(bad)
    assert mesh.vertices is None and not mesh._device_posed
    mesh.set_vertices(P.tolist())
    assert mesh._device_posed and np.array_equal(mesh.vertices, P)
    P[0, 0] = 9.0  # (the mesh keeps a copy)
    assert mesh.vertices[0, 0] != 9.0 and mesh.file_vertices[0, 0] != 9.0


def test_corner_indices_are_those_python_read(objs):
    """Negative OBJ indices: the constructor reads verts[i - 1] with Python's wrap-around; the mesh keeps the
    index that named."""
    path = str(objs["dir"] / "negative.obj")
    with open(path, "w") as fh:
        for v in ((0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5)):
            fh.write("v %r %r %r\n" % v)
        fh.write("f 1 2 3\nf 1 -1 2\nf 0 3 2\n")  # -1 -> verts[-2], 0 -> verts[-1]
    mesh = MD.mesh_of(VR.mesh_scene(path, smooth=True))
    assert mesh.corners.tolist() == [[0, 1, 2], [0, 2, 1], [3, 2, 1]]
    rest = MP.records(mesh.collider_list)
    assert np.array_equal(mesh.file_vertices[mesh.corners] + MD.center_of(mesh), mesh.rest_vertices())
    assert _equal(MD.hc_deform_triangles(mesh, rest, mesh.file_vertices), rest)


def test_lowering_takes_a_deformed_mesh_from_its_cache(objs, monkeypatch):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    plain = _lower.lower_scene(sc)
    assert plain.posed == []
    calls = []
    real = _lower.collider_record
    monkeypatch.setattr(_lower, "collider_record", lambda c: (calls.append(c), real(c))[1])
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    first = _lower.lower_scene(sc)  # (fills the cache)
    assert first.signature() == plain.signature() and first.colliders.tobytes() == plain.colliders.tobytes()
    (p,) = first.posed
    assert (p["first"], p["count"]) == (1, 80) and np.array_equal(p["pose"], MP.IDENTITY)
    d = p["deform"]
    assert np.array_equal(d["verts"], P) and np.array_equal(d["corners"], mesh.corners)
    assert np.array_equal(d["center"], MD.center_of(mesh)) and d["recompute"].shape == (80, 3)
    # a frame in which only vertices changed: nothing of the mesh is lowered, the signature stays
    mesh.set_vertices(MD.bulge(mesh.file_vertices))
    del calls[:]
    second = _lower.lower_scene(sc)
    assert len(calls) == len(sc.collider_list) - 80 and not any(type(c).__name__ == "Triangle_Collider" for c in calls)
    assert second.signature() == plain.signature() and second.colliders.tobytes() == plain.colliders.tobytes()
    assert second.posed[0]["vver"] == p["vver"] + 1 and second.posed[0]["key"] == p["key"]
    assert np.array_equal(second.posed[0]["deform"]["verts"], MD.bulge(mesh.file_vertices))
    # reset_vertices: the file's positions, still through the device
    mesh.reset_vertices()
    third = _lower.lower_scene(sc)
    assert np.array_equal(third.posed[0]["deform"]["verts"], mesh.file_vertices) and third.posed[0]["vver"] == p["vver"] + 2
    # invalidate() drops the deformation
    mesh.set_vertices(P)
    mesh.invalidate()
    assert mesh.vertices is None and _lower.lower_scene(sc).posed[0]["deform"] is None
    # ... and so does rotate(): the Python colliders are uploaded again
    mesh.set_vertices(P)
    key = _lower.lower_scene(sc).posed[0]["key"]
    mesh.rotate(20.0, vec3(0.0, 1.0, 0.0))
    assert mesh.vertices is None
    del calls[:]
    turned = _lower.lower_scene(sc)
    assert len(calls) == len(sc.collider_list) and turned.signature() != plain.signature()
    assert turned.posed[0]["deform"] is None and turned.posed[0]["key"] != key
    assert np.array_equal(mesh.deformed_vertices(), mesh.rest_vertices())
    # the colliders have left the file's frame: vertices in that frame are refused from here on
    with pytest.raises(NotImplementedError, match="rotate"):
        mesh.set_vertices(P)
    mesh.reset_vertices()
    assert mesh.vertices is None


def test_reset_vertices_of_a_mesh_that_is_not_deformed_does_nothing(objs):
    mesh = MD.mesh_of(scenes.mesh_scene(objs["ico1"]))
    mesh.reset_vertices()
    assert mesh.vertices is None and not mesh._device_posed and mesh._vert_version == 0


def test_motion_rows_of_a_vertex_version_change(objs):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    sl = slice(1, 81)
    mesh.set_vertices(MD.twist(mesh.file_vertices))
    prev = _lower.lower_scene(sc)
    # the same vertices in both frames: today's rows (the identity, or the pose pair's)
    cur = _lower.lower_scene(sc)
    rows = _motion.pose_motion(_motion.collider_motion(prev.colliders, cur.colliders), prev.posed, cur.posed)
    assert (rows == _motion.IDENTITY).all()
    mesh.set_pose(SKEW, SHIFT)
    cur = _lower.lower_scene(sc)
    rows = _motion.pose_motion(_motion.collider_motion(prev.colliders, cur.colliders), prev.posed, cur.posed)
    assert _motion.count_rows(rows) == (80, 0) and (rows[sl] == rows[1]).all()
    def strip(posed):  # entries without the field, as a caller's of before it existed
        return [{k: v for k, v in p.items() if k not in ("vver", "deform")} for p in posed]

    assert np.array_equal(_motion.pose_motion(_motion.collider_motion(prev.colliders, cur.colliders), strip(prev.posed),
                                              strip(cur.posed)), rows)
    # other vertices: NaN rows for the mesh, whatever the poses; the other colliders keep theirs
    mesh.set_vertices(MD.bulge(mesh.file_vertices))
    for pose in (True, False):
        if not pose:
            mesh.reset_pose()
        nxt = _lower.lower_scene(sc)
        rows = _motion.pose_motion(_motion.collider_motion(cur.colliders, nxt.colliders), cur.posed, nxt.posed)
        assert np.isnan(rows[sl]).all() and _motion.count_rows(rows) == (0, 80)
        assert (rows[0] == _motion.IDENTITY).all() and (rows[81:] == _motion.IDENTITY).all()
    assert cur.posed[0]["key"] == nxt.posed[0]["key"]  # ("key" is what it was: the rest geometry's)


def test_a_deformed_mesh_is_refused_in_a_hybrid_scene(objs):
    from sightpy import _hybrid

    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    mesh.set_vertices(MD.twist(mesh.file_vertices))
    real = _hybrid.is_hybrid
    try:
        _hybrid.is_hybrid = lambda scene: True
        with pytest.raises(NotImplementedError, match="set_vertices"):
            _lower.lower_scene(sc)
        mesh.invalidate()
        _lower.lower_scene(sc)  # the loaded shape is what the Python colliders hold
    finally:
        _hybrid.is_hybrid = real
