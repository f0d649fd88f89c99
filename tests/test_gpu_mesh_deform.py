"""Device-deformed triangle meshes on the GPU (TriangleMesh.set_vertices -> srt_deform_colliders: k_deform_face_cross,
k_deform_vertex_normals, k_deform_triangles, then k_bvh_refit; csrc/rt_deform.h): frames of a deformed scene against
the ordinary upload of the same scene with its mesh reloaded from an OBJ file holding the deformed vertices
(mesh_deform_ref.py), and against the oracle on it.  64 x 48, depth 3, 2 spp.  Sizes: 42 vertices / 80 triangles (under
one wave), 162 / 320 (past a wave of vertices and a block of triangles), the 8-triangle octahedron (a single-node tree),
the 4-triangle tetrahedron (no tree).  The CPU versions of the record and refit checks are in test_mesh_deform.py."""
import ctypes

import numpy as np
import pytest

import hostcheck as HC
import mesh_deform_ref as MD
import mesh_pose_ref as MP
import scenes
import sightpy_oracle as O
import vattr_ref as VR
from sightpy import _native as N
from sightpy import vec3
from sightpy.geometry.triangle_mesh import TriangleMesh

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-12
SPP = 2
SKEW = MP.rotation(40.0, (1.0, 2.0, 0.5))
SHIFT = (0.25, 0.1, 0.2)


def _backend():
    from sightpy import _backend

    return _backend


def _set_option(key, value):
    lib, ctx = _backend().context()
    rc = lib.srt_set_option(ctx, key.encode(), ctypes.c_int64(value))
    assert rc == 0, lib.srt_last_error()


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_mesh_deform")
    out = {"dir": d}
    for sub in (1, 2):
        out["ico%d" % sub] = str(d / ("ico%d.obj" % sub))
        scenes.write_icosphere_obj(out["ico%d" % sub], subdiv=sub)
    out["tetra"] = str(d / "tetra.obj")
    VR.write_tetrahedron_obj(out["tetra"])
    vn = str(d / "vn.obj")
    VR.write_smooth_icosphere_obj(vn, 1)
    out["uv"] = str(d / "uv.obj")  # `v/vt` faces: texture coordinates, area-weighted normals
    with open(vn) as fi, open(out["uv"], "w") as fo:
        for line in fi:
            tok = line.split()
            if tok[0] == "f":
                fo.write("f " + " ".join("/".join(t.split("/")[:2]) for t in tok[1:]) + "\n")
            elif tok[0] != "vn":
                fo.write(line)
    out["octa"] = str(d / "octa.obj")
    with open(out["octa"], "w") as fh:
        for v in ((0.5, 0, 0), (-0.5, 0, 0), (0, 0.5, 0), (0, -0.5, 0), (0, 0, 0.5), (0, 0, -0.5)):
            fh.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for f in ((1, 3, 5), (3, 2, 5), (2, 4, 5), (4, 1, 5), (3, 1, 6), (2, 3, 6), (4, 2, 6), (1, 4, 6)):
            fh.write("f %d %d %d\n" % f)
    return out


# ("smooth2": the 320-triangle mesh, compared with uploads only -- the oracle takes 15 s on it)
KINDS = {"flat": ("ico1", False, False), "smooth": ("ico1", True, False), "textured": ("uv", True, True),
         "smooth2": ("ico2", True, False)}
_serial = [0]


def _scene(objs, kind, path=None):
    which, smooth, tex = KINDS[kind]
    return VR.mesh_scene(path or objs[which], smooth=smooth, texcoords=tex, material=VR.checker() if tex else None)


def _deformed_obj(objs, src, P):
    _serial[0] += 1
    return MD.write_deformed_obj(src, str(objs["dir"] / ("deformed_%d.obj" % _serial[0])), P)


def _jitter(sc, seed=9):
    np.random.seed(seed)
    return np.ascontiguousarray(sc.camera.draw_jitter(SPP))


def _render(sc, jit):
    return _backend().render_scene(sc, SPP, jitter=jit, seed=1, want_hits=True)


def _mesh_ids(sc):
    return np.array([i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Triangle_Collider"])


def _against(sc, ref, jit, what):
    """The deformed scene's frame against the frame of `ref`, uploaded in the ordinary way: primary hit ids equal,
    RGB within 1e-5 relative, at least 50 pixels on the mesh.  Returns the deformed frame."""
    got = _render(sc, jit)
    want = _render(ref, jit)
    print(what, "largest |RGB deviation| from the reloaded upload:", np.abs(got.rgb - want.rgb).max())
    assert np.array_equal(got.hit_ids, want.hit_ids), what
    np.testing.assert_allclose(got.rgb, want.rgb, rtol=RTOL, atol=ATOL)
    assert np.isin(got.hit_ids, _mesh_ids(sc)).sum() >= 50, what
    return got


def _posed_ref(ref, pose):
    """The reloaded scene `ref` with its meshes under `pose` (R, t), restated as mesh_pose_ref restates a posed scene."""
    for m in (p for p in ref.scene_primitives if isinstance(p, TriangleMesh)):
        m.set_pose(*pose)
    return MP.restated_scene(ref)


@pytest.mark.parametrize("kind", ["flat", "smooth", "textured"])
def test_gpu_deformed_mesh_against_an_upload_and_the_oracle(objs, kind, monkeypatch):
    if kind != "flat":
        VR.patch(monkeypatch)
    sc = _scene(objs, kind)
    mesh = MD.mesh_of(sc)
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    ref = _scene(objs, kind, _deformed_obj(objs, objs[KINDS[kind][0]], P))
    jit = _jitter(sc)
    got = _against(sc, ref, jit, kind)
    rgb, ids, counts = O.render_linear(ref, jit)
    assert np.array_equal(got.hit_ids, ids)
    keep = slice(None)
    if kind == "textured":  # (a texel index may flip at a texel boundary: vattr_ref's rule for textured frames)
        keep = ~VR.texel_boundary_pixels(ref, jit)
        assert keep.mean() > 0.9
    print(kind, "largest |RGB deviation| from the oracle:", np.abs(got.rgb[:, keep] - rgb[:, keep]).max())
    np.testing.assert_allclose(got.rgb[:, keep], rgb[:, keep], rtol=RTOL, atol=ATOL)
    # the undeformed frame is another one
    assert not np.array_equal(_render(_scene(objs, kind), jit).rgb, got.rgb)


def test_gpu_deformation_out_of_the_loaded_root_box(objs):
    """Without the refit the traversal would still cull by the loaded shape's boxes and lose the mesh."""
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    P = MD.twist(mesh.file_vertices) * 0.8 + np.array([-1.2, 0.25, 0.3])
    mesh.set_vertices(P)
    rest, now = mesh.rest_vertices().reshape(-1, 3), mesh.deformed_vertices().reshape(-1, 3)
    assert now[:, 0].max() < rest[:, 0].min() - 0.05  # entirely outside the loaded shape's root box
    _against(sc, scenes.mesh_scene(_deformed_obj(objs, objs["ico1"], P)), _jitter(sc), "moved out")


def test_gpu_linear_loop_against_the_refitted_bvh(objs):
    B = _backend()
    sc = scenes.mesh_scene(objs["ico2"])
    mesh = MD.mesh_of(sc)
    mesh.set_vertices(MD.twist(mesh.file_vertices))
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


def test_gpu_no_drift_over_a_deformation_sequence(objs):
    """file shape -> A -> B -> file shape: the last frame is the first bit for bit; the frames after the first each
    cost one deform call and no upload."""
    B = _backend()
    sc = scenes.mesh_scene(objs["ico2"])
    mesh = MD.mesh_of(sc)
    V = mesh.file_vertices
    jit = _jitter(sc)
    B.forget_resident()
    frames, cost = [], []
    for P in (None, MD.twist(V), MD.bulge(V), V):
        if P is not None:
            mesh.set_vertices(P)
        before = (B._STATE["uploads"], B._STATE["deform_calls"])
        frames.append(_render(sc, jit))
        cost.append((B._STATE["uploads"] - before[0], B._STATE["deform_calls"] - before[1]))
    assert cost == [(1, 0), (0, 1), (0, 1), (0, 1)], cost
    assert not np.array_equal(frames[1].rgb, frames[0].rgb) and not np.array_equal(frames[2].rgb, frames[1].rgb)
    assert np.array_equal(frames[3].hit_ids, frames[0].hit_ids) and np.array_equal(frames[3].rgb, frames[0].rgb)
    assert np.array_equal(frames[3].srgb8, frames[0].srgb8)
    # frame B again, by reset_vertices() and back: the same frame, one call each
    before = B._STATE["deform_calls"]
    mesh.reset_vertices()
    again0 = _render(sc, jit)
    mesh.set_vertices(MD.bulge(V))
    again2 = _render(sc, jit)
    assert B._STATE["deform_calls"] - before == 2
    assert np.array_equal(again0.rgb, frames[0].rgb) and np.array_equal(again2.rgb, frames[2].rgb)
    # the timing entry point saw the calls
    lib, ctx = B.context()
    ms = [ctypes.c_double(-1.0) for _ in range(3)]
    calls = ctypes.c_int64(0)
    N.check(lib, lib.srt_debug_deform_times(ctx, *[ctypes.byref(m) for m in ms], ctypes.byref(calls)))
    assert calls.value >= 5 and all(m.value >= 0.0 for m in ms) and ms[1].value > 0.0 and ms[2].value > 0.0


def test_gpu_another_scene_with_the_same_tables_after_a_deformed_one(objs):
    """A deformed mesh's table holds the loaded shape, so a fresh Scene of the same OBJ has the resident signature
    while the device holds the deformed records and boxes: it must be uploaded all the same.  Nothing is rendered
    between the two scenes."""
    from sightpy._lower import lower_scene

    B = _backend()
    sc = scenes.plain_mesh_scene(objs["ico2"])
    mesh = MD.mesh_of(sc)
    mesh.set_vertices(MD.twist(mesh.file_vertices))
    jit = _jitter(sc)
    B.forget_resident()
    deformed = _render(sc, jit)
    assert np.isin(deformed.hit_ids, _mesh_ids(sc)).sum() >= 50
    for posed in (False, True):
        fresh = scenes.plain_mesh_scene(objs["ico2"])
        if posed:  # device-posed, in the rest pose and the loaded shape: an entry of Lowered.posed without vertices
            MD.mesh_of(fresh).set_pose(np.eye(3))
        assert lower_scene(fresh).signature() == lower_scene(sc).signature()  # (what makes the case)
        before = (B._STATE["uploads"], B._STATE["deform_calls"])
        got = _render(fresh, jit)
        assert (B._STATE["uploads"] - before[0], B._STATE["deform_calls"] - before[1]) == (1, 0), posed
        B.upload(fresh, force=True)
        want = _render(fresh, jit)
        assert np.array_equal(got.hit_ids, want.hit_ids) and np.array_equal(got.rgb, want.rgb), posed
        assert not np.array_equal(got.rgb, deformed.rgb)
        # the same fresh scene again: resident now, nothing to do
        before = B._STATE["uploads"]
        _render(fresh, jit)
        assert B._STATE["uploads"] == before
        # and the deformed scene after it: no upload (the tables are resident), one deform call
        before = (B._STATE["uploads"], B._STATE["deform_calls"])
        again = _render(sc, jit)
        assert (B._STATE["uploads"] - before[0], B._STATE["deform_calls"] - before[1]) == (0, 1), posed
        assert np.array_equal(again.rgb, deformed.rgb)


def test_gpu_deform_then_pose_then_deform_under_the_pose(objs, monkeypatch):
    VR.patch(monkeypatch)
    B = _backend()
    sc = _scene(objs, "smooth2")
    mesh = MD.mesh_of(sc)
    V = mesh.file_vertices
    jit = _jitter(sc)
    src = objs[KINDS["smooth2"][0]]
    mesh.set_vertices(MD.twist(V))
    _against(sc, _scene(objs, "smooth2", _deformed_obj(objs, src, MD.twist(V))), jit, "deformed A")
    mesh.set_pose(SKEW, SHIFT)
    _against(sc, _posed_ref(_scene(objs, "smooth2", _deformed_obj(objs, src, MD.twist(V))), (SKEW, SHIFT)), jit,
             "deformed A, posed")
    _render(sc, jit)  # (the scene is resident again, deformed and posed)
    before = (B._STATE["uploads"], B._STATE["deform_calls"], B._STATE["pose_calls"])
    mesh.set_vertices(MD.bulge(V))
    ref = _posed_ref(_scene(objs, "smooth2", _deformed_obj(objs, src, MD.bulge(V))), (SKEW, SHIFT))
    got = _render(sc, jit)  # (before the reference's upload: what the change of vertices alone costs)
    assert (B._STATE["uploads"] - before[0], B._STATE["deform_calls"] - before[1], B._STATE["pose_calls"] - before[2]) \
        == (0, 1, 1)
    want = _render(ref, jit)
    assert np.array_equal(got.hit_ids, want.hit_ids)
    np.testing.assert_allclose(got.rgb, want.rgb, rtol=RTOL, atol=ATOL)
    mesh.reset_pose()
    _against(sc, _scene(objs, "smooth2", _deformed_obj(objs, src, MD.bulge(V))), jit, "deformed B, pose reset")


def test_gpu_two_meshes_one_deformed_then_both(objs):
    def two(path_one, path_two):
        sc = scenes.mesh_scene(path_one)
        red = MD.mesh_of(sc)
        sc.add(TriangleMesh(path_two, center=vec3(-0.3, 0.1, -0.2), material=red.material, max_ray_depth=3))
        return sc

    sc = two(objs["ico1"], objs["ico1"])
    one, other = MD.mesh_of(sc, 0), MD.mesh_of(sc, 1)
    V = one.file_vertices
    jit = _jitter(sc)
    other.set_vertices(MD.twist(V))
    a = _deformed_obj(objs, objs["ico1"], MD.twist(V))
    _against(sc, two(objs["ico1"], a), jit, "second of two meshes deformed")
    one.set_vertices(MD.bulge(V))
    b = _deformed_obj(objs, objs["ico1"], MD.bulge(V))
    _against(sc, two(b, a), jit, "both deformed")
    other.reset_vertices()
    _against(sc, two(b, objs["ico1"]), jit, "first deformed, second back at the file's shape")


def test_gpu_a_bvh_of_a_single_node_and_a_mesh_in_the_linear_loop(objs):
    sc = scenes.mesh_scene(objs["octa"])
    assert HC.bvh_nodes(sc) == 1
    mesh = MD.mesh_of(sc)
    P = MD.twist(mesh.file_vertices, 100.0)
    mesh.set_vertices(P)
    _against(sc, scenes.mesh_scene(_deformed_obj(objs, objs["octa"], P)), _jitter(sc), "octahedron")
    # four triangles: no BVH, the mesh stays in the linear loop and is deformed all the same
    small = VR.mesh_scene(objs["tetra"], smooth=False)
    assert HC.bvh_nodes(small) == 0
    mesh = MD.mesh_of(small)
    P = MD.twist(mesh.file_vertices, 100.0)
    mesh.set_vertices(P)
    _against(small, VR.mesh_scene(_deformed_obj(objs, objs["tetra"], P), smooth=False), _jitter(small), "tetrahedron")


def test_gpu_guides_of_a_deformed_scene(objs):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    P = MD.twist(mesh.file_vertices)
    mesh.set_vertices(P)
    got = sc.get_aovs()
    want = scenes.mesh_scene(_deformed_obj(objs, objs["ico1"], P)).get_aovs()
    assert set(got) == set(want) == {"hit_id", "depth", "position", "normal", "albedo"}
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.isin(got["hit_id"], _mesh_ids(sc)).mean() > 0.02


def test_gpu_deform_entry_points_refusals(objs):
    """Every SRT_ERR_ARG case of srt_deform_topology and srt_deform_colliders.  The bad corner indices and ranges
    are refused by the host's checks: none reaches a kernel."""
    B = _backend()
    lib, ctx = B.context()
    sc = scenes.mesh_scene(objs["ico1"])  # colliders: 0 sphere, 1..80 mesh, 81 plane, 82 sky box
    mesh = MD.mesh_of(sc)
    B.upload(sc, force=True)
    corners = np.ascontiguousarray(mesh.corners)
    flags = np.zeros((80, 3), dtype=np.uint8)
    center = MD.center_of(mesh)
    V = np.ascontiguousarray(mesh.file_vertices)

    def topology(c, first=1, count=80, n_verts=42, cn=corners, ctr=center, fl=flags):
        rc = lib.srt_deform_topology(c, first, count, n_verts, N.ptr(cn), N.ptr(ctr), N.ptr(fl))
        return rc, lib.srt_last_error()

    def deform(c, ranges, arrays, n=None):
        first = np.array([r[0] for r in ranges], dtype=np.int32)
        count = np.array([r[1] for r in ranges], dtype=np.int32)
        ptrs = (ctypes.c_void_p * max(1, len(arrays)))(*[N.ptr(a) for a in arrays])
        rc = lib.srt_deform_colliders(c, len(first) if n is None else n, N.ptr(first), N.ptr(count), ptrs)
        return rc, lib.srt_last_error()

    def refused(res, name, what):
        rc, msg = res
        assert rc == N.ERR_ARG and msg.startswith(name), (what, rc, msg)

    high, low = corners.copy(), corners.copy()
    high[79, 2], low[0, 0] = 42, -1
    try:
        T = b"srt_deform_topology"
        refused(topology(ctx, first=70, count=20), T, "outside the table")
        refused(topology(ctx, first=-1, count=4), T, "negative first")
        refused(topology(ctx, first=5, count=0), T, "empty range")
        refused(topology(ctx, first=0, count=3), T, "a sphere")
        refused(topology(ctx, first=79, count=3), T, "the plane")
        refused(topology(ctx, n_verts=0), T, "no vertices")
        refused(topology(ctx, cn=high), T, "a corner index of n_verts")
        refused(topology(ctx, cn=low), T, "a negative corner index")
        refused(topology(ctx, cn=None), T, "null corners")
        D = b"srt_deform_colliders"
        refused(deform(ctx, [(1, 80)], [V]), D, "not registered yet")
        assert topology(ctx)[0] == 0
        refused(topology(ctx), T, "registered twice")
        refused(topology(ctx, first=41, count=10, cn=corners[:10], fl=flags[:10]), T, "overlapping a registered range")
        nan, inf = V.copy(), V.copy()
        nan[7, 1], inf[41, 2] = np.nan, np.inf
        refused(deform(ctx, [(1, 40)], [V]), D, "part of a registered range")
        refused(deform(ctx, [(2, 80)], [V]), D, "an unregistered range")
        refused(deform(ctx, [(1, 80)], [None]), D, "a null vertex array")
        refused(deform(ctx, [(1, 80)], [nan]), D, "nan")
        refused(deform(ctx, [(1, 80)], [inf]), D, "inf")
        refused(deform(ctx, [(1, 80), (1, 80)], [V, V]), D, "named twice")
        for n in (0, -2):
            refused(deform(ctx, [(1, 80)], [V], n=n), D, n)
        # a valid call afterwards succeeds, and the frame is the deformed one
        P = np.ascontiguousarray(MD.twist(V))
        assert deform(ctx, [(1, 80)], [P])[0] == 0 and deform(ctx, [(1, 80)], [P])[0] == 0
        jit = _jitter(sc)
        got = _render(sc, jit)  # (the same tables are resident: nothing is uploaded or deformed again)
        want = _render(scenes.mesh_scene(_deformed_obj(objs, objs["ico1"], P)), jit)
        assert np.array_equal(got.hit_ids, want.hit_ids)
        np.testing.assert_allclose(got.rgb, want.rgb, rtol=RTOL, atol=ATOL)
        # an upload drops the registrations
        B.upload(sc, force=True)
        refused(deform(ctx, [(1, 80)], [V]), D, "dropped by the upload")
        # a context without a scene
        other = ctypes.c_void_p()
        N.check(lib, lib.srt_create(B._STATE["device"], ctypes.byref(other)))
        try:
            refused(topology(other), T, "no scene")
            refused(deform(other, [(1, 80)], [V]), D, "no scene")
        finally:
            lib.srt_destroy(other)
    finally:
        B.forget_resident()


def test_gpu_a_deformed_mesh_is_refused_on_several_gpus(objs, monkeypatch):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    mesh.set_vertices(MD.twist(mesh.file_vertices))
    monkeypatch.setenv("SIGHTPY_DEVICES", "0,1")
    with pytest.raises(NotImplementedError, match="one GPU"):
        _backend().upload(sc)


def test_gpu_temporal_history_of_a_mesh_deformed_each_frame(objs):
    """Three frames of a mesh deformed each frame through render(denoise={temporal, variance, demodulate, motion}):
    the mesh's rows are NaN from frame 2 on (motion_unknown counts its triangles, motion_moved is 0), so its pixels
    find no history; each frame is the restated pipeline's within one count (half-frames -> temporal_motion_ref with
    those rows -> denoise_var_ref -> the oracle's resolve)."""
    import denoise_ref as DR
    import denoise_var_ref as DV
    import temporal_motion_ref as MR
    import temporal_ref as TR

    B = _backend()
    DNM = {"temporal": True, "variance": True, "demodulate": True, "motion": True}
    W, H = 64, 48
    sc = scenes.mesh_scene(objs["ico1"], W, H, 3)
    mesh = MD.mesh_of(sc)
    V = mesh.file_vertices
    ids = _mesh_ids(sc)
    hist, cam = None, None
    for k in range(3):
        P = MD.twist(V, 20.0 * (k + 1))
        mesh.set_vertices(P)
        np.random.seed(4 + k)
        A, Bh, ka, kb, _ = B.render_halves(sc, SPP)
        np.random.seed(4 + k)
        img = sc.render(SPP, denoise=DNM)
        dn = sc.last_stats["denoise"]
        assert (dn["motion_moved"], dn["motion_unknown"]) == ((0, 80) if k else (0, 0))
        ref = scenes.mesh_scene(_deformed_obj(objs, objs["ico1"], P), W, H, 3)
        guides = DR.aovs(ref)
        rows = None
        if k:
            rows = MR.identity_rows(len(sc.collider_list))
            rows[ids] = np.nan
        info = {}
        out = MR.accumulate(A, Bh, guides, W, H, history=hist, prev_cam=cam, motion=rows, demodulate=True, info=info)
        on_mesh = np.isin(guides["hit_id"], ids)
        assert on_mesh.mean() > 0.02
        print("frame", k, "mesh pixels with history:", int(info["has"][on_mesh].sum()), "of", int(on_mesh.sum()),
              "; other pixels with history:", int(info["has"][~on_mesh].sum()))
        assert not info["has"][on_mesh].any()
        assert info["has"][~on_mesh].any() == (k > 0)
        want = O.srgb_u8(DV.denoise_var(out["a"], out["b"], ka, kb, guides, W, H, variance=True, demodulate=True)[0], H, W)
        dev = np.abs(np.asarray(img).astype(int) - want.astype(int)).max()
        print("frame", k, "largest deviation in counts", dev)
        assert dev <= 1, k
        hist, cam = TR.next_history(out, guides), TR.camera_dict(sc.camera)
