"""Device-posed triangle meshes on the GPU (TriangleMesh.set_pose -> srt_pose_colliders: k_pose_triangles and
k_bvh_refit, csrc/rt_pose.h): frames of a posed scene against the same scene uploaded from the restated posed
vertices (mesh_pose_ref.py) and against the oracle on it.  64 x 48, depth 3, 2 spp.  The CPU versions of the
record and refit checks are in test_mesh_pose.py."""
import ctypes

import numpy as np
import pytest

import hostcheck as HC
import mesh_pose_ref as MP
import scenes
import sightpy_oracle as O
import vattr_ref as VR
from sightpy import _native as N
from sightpy.geometry.triangle_mesh import TriangleMesh

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-12
SPP = 2
SKEW = MP.rotation(40.0, (1.0, 2.0, 0.5))
SHIFT = (0.25, 0.1, 0.2)
POSE_B = (MP.rotation(-115.0, (0.3, -1.0, 0.2)), (-0.4, 0.2, 0.3))


def _backend():
    from sightpy import _backend

    return _backend


def _set_option(key, value):
    lib, ctx = _backend().context()
    rc = lib.srt_set_option(ctx, key.encode(), ctypes.c_int64(value))
    assert rc == 0, lib.srt_last_error()


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_mesh_pose")
    out = {}
    for sub in (1, 2):
        out["ico%d" % sub] = str(d / ("ico%d.obj" % sub))
        scenes.write_icosphere_obj(out["ico%d" % sub], subdiv=sub)
    out["tetra"] = str(d / "tetra.obj")
    VR.write_tetrahedron_obj(out["tetra"])
    out["smooth"] = str(d / "smooth.obj")
    VR.write_smooth_icosphere_obj(out["smooth"], 1)
    out["octa"] = str(d / "octa.obj")
    with open(out["octa"], "w") as fh:
        for v in ((0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)):
            fh.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for f in ((1, 3, 5), (3, 2, 5), (2, 4, 5), (4, 1, 5), (3, 1, 6), (2, 3, 6), (4, 2, 6), (1, 4, 6)):
            fh.write("f %d %d %d\n" % f)
    return out


def _meshes(sc):
    return [p for p in sc.scene_primitives if isinstance(p, TriangleMesh)]


def _jitter(sc, seed=9):
    np.random.seed(seed)
    return np.ascontiguousarray(sc.camera.draw_jitter(SPP))


def _render(sc, jit):
    return _backend().render_scene(sc, SPP, jitter=jit, seed=1, want_hits=True)


def _mesh_ids(sc):
    return np.array([i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Triangle_Collider"])


def _against_restated(sc, jit, what):
    """The posed scene's frame against the frame of the scene uploaded from the restated posed vertices: primary
    hit ids equal, RGB within 1e-5 relative.  Returns (posed frame, restated scene)."""
    got = _render(sc, jit)
    restated = MP.restated_scene(sc)
    want = _render(restated, jit)
    dev = np.abs(got.rgb - want.rgb).max()
    print(what, "largest |RGB deviation| from the restated upload:", dev)
    assert np.array_equal(got.hit_ids, want.hit_ids), what
    np.testing.assert_allclose(got.rgb, want.rgb, rtol=RTOL, atol=ATOL)
    assert np.isin(got.hit_ids, _mesh_ids(sc)).sum() >= 50, what  # the mesh is in the picture (any part of it will do)
    return got, restated


@pytest.mark.parametrize("kind", ["flat", "smooth", "textured"])
def test_gpu_posed_mesh_against_an_upload_and_the_oracle(objs, kind, monkeypatch):
    if kind == "flat":
        sc = scenes.mesh_scene(objs["ico1"])
    else:
        VR.patch(monkeypatch)
        sc = VR.mesh_scene(objs["smooth"], smooth=True, texcoords=kind == "textured",
                           material=VR.checker() if kind == "textured" else None)
    _meshes(sc)[0].set_pose(SKEW, SHIFT)
    jit = _jitter(sc)
    got, restated = _against_restated(sc, jit, kind)
    rgb, ids, counts = O.render_linear(restated, jit)
    assert np.array_equal(got.hit_ids, ids)
    keep = slice(None)
    if kind == "textured":  # (a texel index may flip at a texel boundary: vattr_ref's rule for textured frames)
        keep = ~VR.texel_boundary_pixels(restated, jit)
        assert keep.mean() > 0.9
    np.testing.assert_allclose(got.rgb[:, keep], rgb[:, keep], rtol=RTOL, atol=ATOL)
    if kind != "textured":
        assert got.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]


def test_gpu_pose_out_of_the_rest_root_box(objs):
    """Without the refit the traversal would still cull by the rest pose's boxes and lose the mesh."""
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _meshes(sc)[0]
    mesh.set_pose(MP.rotation(25.0, (0.0, 1.0, 0.3)), (-1.15, 0.25, 0.3))
    rest, posed = mesh.rest_vertices().reshape(-1, 3), mesh.posed_vertices().reshape(-1, 3)
    assert posed[:, 0].max() < rest[:, 0].min() - 0.05  # entirely outside the rest pose's root box
    _against_restated(sc, _jitter(sc), "moved out")


def test_gpu_linear_loop_against_the_refitted_bvh(objs):
    B = _backend()
    sc = scenes.mesh_scene(objs["ico2"])
    _meshes(sc)[0].set_pose(*POSE_B)
    jit = _jitter(sc)
    on = _render(sc, jit)
    _set_option("bvh", 0)
    try:
        B.upload(sc, force=True)
        off = _render(sc, jit)
    finally:
        _set_option("bvh", 1)
        B.forget_resident()
    assert np.array_equal(on.hit_ids, off.hit_ids)
    assert np.array_equal(on.rgb, off.rgb) and np.array_equal(on.srgb8, off.srgb8)
    assert np.isin(on.hit_ids, _mesh_ids(sc)).mean() > 0.02


def test_gpu_no_drift_over_a_pose_sequence(objs):
    """identity -> pose A -> pose B -> identity: the last frame is the first, and a fresh context's, bit for bit;
    the frames after the first each cost one pose call and no upload."""
    B = _backend()
    sc = scenes.mesh_scene(objs["ico2"])
    mesh = _meshes(sc)[0]
    jit = _jitter(sc)
    B.forget_resident()
    frames, cost = [], []
    for pose in (None, (SKEW, SHIFT), POSE_B, (np.eye(3), (0.0, 0.0, 0.0))):
        if pose is not None:
            mesh.set_pose(*pose)
        before = (B._STATE["uploads"], B._STATE["pose_calls"])
        frames.append(_render(sc, jit))
        cost.append((B._STATE["uploads"] - before[0], B._STATE["pose_calls"] - before[1]))
    assert cost == [(1, 0), (0, 1), (0, 1), (0, 1)], cost
    assert not np.array_equal(frames[1].rgb, frames[0].rgb) and not np.array_equal(frames[2].rgb, frames[1].rgb)
    for f in (frames[3],):
        assert np.array_equal(f.hit_ids, frames[0].hit_ids) and np.array_equal(f.rgb, frames[0].rgb)
    # a context of its own, which has seen no other pose
    lib, old = B.context()
    B._STATE["ctx"] = None
    try:
        fresh = _render(sc, jit)
        new = B._STATE["ctx"]
    finally:
        made = B._STATE["ctx"]
        B._STATE["ctx"] = old
        if made is not None and made is not old:
            B.forget_resident(made)
            lib.srt_destroy(made)
    assert new is not old
    assert np.array_equal(fresh.hit_ids, frames[0].hit_ids) and np.array_equal(fresh.rgb, frames[0].rgb)


def test_gpu_two_meshes_one_posed_and_a_mesh_in_the_linear_loop(objs):
    from sightpy import vec3

    sc = scenes.mesh_scene(objs["ico1"])
    red = _meshes(sc)[0]
    sc.add(TriangleMesh(objs["ico1"], center=vec3(-0.3, 0.1, -0.2), material=red.material, max_ray_depth=3))
    one, two = _meshes(sc)
    two.set_pose(SKEW, (0.1, 0.0, -0.1))
    jit = _jitter(sc)
    got, _ = _against_restated(sc, jit, "second of two meshes posed")
    # the other one as well, then the first alone (the second back at rest)
    one.set_pose(*POSE_B)
    _against_restated(sc, jit, "both posed")
    two.reset_pose()
    _against_restated(sc, jit, "first posed, second back at rest")
    # four triangles: no BVH, the mesh stays in the linear loop and is posed all the same
    small = VR.mesh_scene(objs["tetra"], smooth=False)
    assert HC.bvh_nodes(small) == 0
    _meshes(small)[0].set_pose(SKEW, SHIFT)
    _against_restated(small, _jitter(small), "tetrahedron in the linear loop")


def test_gpu_ranges_on_either_side_of_a_wave(objs):
    """srt_pose_colliders itself, ranges of 1, 63, 64 and 65 triangles under four poses (the mesh is torn apart,
    which is no concern of the tables)."""
    B = _backend()
    lib, ctx = B.context()
    sc = scenes.mesh_scene(objs["ico2"])
    mesh = _meshes(sc)[0]
    jit = _jitter(sc)
    L = B.upload(sc, force=True)
    assert L.colliders["type"][1] == N.TRIANGLE and L.colliders["type"][320] == N.TRIANGLE
    c = np.array([mesh.center.x, mesh.center.y, mesh.center.z])
    ranges = [(1, 1, MP.pose_numbers(SKEW, c, (0.0, 0.5, 0.0))), (10, 63, MP.pose_numbers(POSE_B[0], c, (0.1, 0.0, 0.2))),
              (100, 64, MP.pose_numbers(np.eye(3), c, (-0.2, 0.1, 0.0))),
              (200, 65, MP.pose_numbers(MP.rotation(90.0, (1.0, 2.0, 0.5)), c, (0.0, 0.2, 0.1)))]
    first, count, poses = MP._ranges(ranges)
    try:
        N.check(lib, lib.srt_pose_colliders(ctx, 4, N.ptr(first), N.ptr(count), N.ptr(poses)))
        got = _render(sc, jit)  # (the same tables are resident: nothing is uploaded or posed again)
    finally:
        B.forget_resident()
    V, Nn, UV = MP.mesh_arrays(mesh)
    for f, n, pose in ranges:
        V[f - 1:f - 1 + n] = MP.posed_vertices(V[f - 1:f - 1 + n], pose)
    torn = MP.restated_scene(sc)
    k = sc.scene_primitives.index(mesh)
    torn.scene_primitives[k] = MP.ExplicitMesh(mesh, V)
    torn.collider_list = [c for p in torn.scene_primitives for c in p.collider_list]
    torn.shadowed_collider_list = [c for p in torn.scene_primitives[:3] for c in p.collider_list]
    assert len(torn.shadowed_collider_list) == len(sc.shadowed_collider_list)
    want = _render(torn, jit)
    assert np.array_equal(got.hit_ids, want.hit_ids)
    np.testing.assert_allclose(got.rgb, want.rgb, rtol=RTOL, atol=ATOL)
    print("ranges: largest |RGB deviation|", np.abs(got.rgb - want.rgb).max())
    rest = _render(sc, jit)
    assert not np.array_equal(rest.hit_ids, got.hit_ids)


def test_gpu_a_bvh_of_a_single_node(objs):
    sc = scenes.mesh_scene(objs["octa"])
    assert HC.bvh_nodes(sc) == 1
    _meshes(sc)[0].set_pose(SKEW, SHIFT)
    _against_restated(sc, _jitter(sc), "octahedron")


def test_gpu_pose_colliders_refusals(objs):
    B = _backend()
    lib, ctx = B.context()
    sc = scenes.mesh_scene(objs["ico1"])  # colliders: 0 sphere, 1..80 mesh, 81 plane, 82 sky box
    B.upload(sc, force=True)
    ident = MP.IDENTITY

    def call(c, ranges, n=None):
        first, count, poses = MP._ranges(ranges)
        rc = lib.srt_pose_colliders(c, len(first) if n is None else n, N.ptr(first), N.ptr(count), N.ptr(poses))
        return rc, lib.srt_last_error()

    bad_pose = ident.copy()
    bad_pose[4] = np.nan
    inf_pose = ident.copy()
    inf_pose[10] = np.inf
    cases = {"outside the table": [(70, 20, ident)], "negative first": [(-1, 4, ident)], "empty range": [(5, 0, ident)],
             "a sphere": [(0, 3, ident)], "the plane": [(79, 3, ident)], "overlap": [(1, 10, ident), (10, 5, ident)],
             "nan": [(1, 80, bad_pose)], "inf": [(1, 80, inf_pose)]}
    try:
        for what, ranges in cases.items():
            rc, msg = call(ctx, ranges)
            assert rc == N.ERR_ARG and msg.startswith(b"srt_pose_colliders"), (what, rc, msg)
        for n in (0, -3):
            rc, msg = call(ctx, [(1, 80, ident)], n=n)
            assert rc == N.ERR_ARG and msg.startswith(b"srt_pose_colliders"), (n, rc, msg)
        assert call(ctx, [(1, 80, ident)])[0] == 0 and call(ctx, [(1, 40, ident), (41, 40, ident)])[0] == 0
        # a context without a scene
        other = ctypes.c_void_p()
        N.check(lib, lib.srt_create(B._STATE["device"], ctypes.byref(other)))
        try:
            rc, msg = call(other, [(1, 80, ident)])
            assert rc == N.ERR_ARG and msg.startswith(b"srt_pose_colliders"), (rc, msg)
        finally:
            lib.srt_destroy(other)
    finally:
        B.forget_resident()


def test_gpu_guides_of_a_posed_scene(objs):
    sc = scenes.mesh_scene(objs["ico1"])
    _meshes(sc)[0].set_pose(SKEW, SHIFT)
    got = sc.get_aovs()
    want = MP.restated_scene(sc).get_aovs()
    assert set(got) == set(want) == {"hit_id", "depth", "position", "normal", "albedo"}
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.isin(got["hit_id"], _mesh_ids(sc)).mean() > 0.02


def test_gpu_a_posed_mesh_is_refused_on_several_gpus(objs, monkeypatch):
    sc = scenes.mesh_scene(objs["ico1"])
    _meshes(sc)[0].set_pose(SKEW)
    monkeypatch.setenv("SIGHTPY_DEVICES", "0,1")
    with pytest.raises(NotImplementedError, match="one GPU"):
        _backend().upload(sc)


def test_gpu_temporal_motion_of_a_translating_mesh(objs):
    """Three frames of a mesh moving 1/3 unit per frame through render(denoise={temporal, motion}): each is the
    restated pipeline's (half-frames -> temporal_motion_ref with rows from the restated objects -> denoise_var_ref
    -> the oracle's resolve) within one count; the mesh's pixels find history on frames 2 and 3 by their rows
    alone; motion_moved counts the mesh's colliders."""
    import denoise_ref as DR
    import denoise_var_ref as DV
    import temporal_motion_ref as MR
    import temporal_ref as TR

    B = _backend()
    DNM = {"temporal": True, "variance": True, "demodulate": True, "motion": True}
    W, H = 64, 48
    sc = scenes.mesh_scene(objs["ico1"], W, H, 3)
    mesh = _meshes(sc)[0]
    ids = _mesh_ids(sc)
    hist, cam, snap = None, None, None
    for k in range(3):
        mesh.set_pose(np.eye(3), (-k / 3.0, 0.0, 0.0))
        np.random.seed(4 + k)
        A, Bh, ka, kb, _ = B.render_halves(sc, SPP)
        np.random.seed(4 + k)
        img = sc.render(SPP, denoise=DNM)
        restated = MP.restated_scene(sc)
        guides, now = DR.aovs(restated), MR.snapshot(restated)
        rows = MR.object_motion(snap, now) if snap is not None else None
        info = {}
        out = MR.accumulate(A, Bh, guides, W, H, history=hist, prev_cam=cam, motion=rows, demodulate=True, info=info)
        on_mesh = np.isin(guides["hit_id"], ids)
        assert on_mesh.mean() > 0.02
        print("frame", k, "mesh pixels with history:", int(info["has"][on_mesh].sum()), "of", int(on_mesh.sum()))
        assert info["has"][on_mesh].any() == (k > 0)
        want = O.srgb_u8(DV.denoise_var(out["a"], out["b"], ka, kb, guides, W, H, variance=True, demodulate=True)[0], H, W)
        dev = np.abs(np.asarray(img).astype(int) - want.astype(int)).max()
        print("frame", k, "largest deviation in counts", dev)
        assert dev <= 1, k
        hist, cam, snap = TR.next_history(out, guides), TR.camera_dict(sc.camera), now
        dn = sc.last_stats["denoise"]
        assert (dn["motion_moved"], dn["motion_unknown"]) == ((80, 0) if k else (0, 0))
