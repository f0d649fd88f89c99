"""Which library calls a frame costs (_backend.upload: plan_upload and its executor over the per-context Resident
record), without a GPU or the library: upload() is driven with a stand-in library that records the calls and returns
0.  The GPU suites count the same decisions around renders (test_gpu_mesh_pose.py, test_gpu_mesh_deform.py)."""
import ctypes

import numpy as np
import pytest

import mesh_deform_ref as MD
import mesh_pose_ref as MP
import scenes
import vattr_ref as VR
from sightpy import _backend as B
from sightpy import _native as N
from sightpy import vec3
from sightpy.geometry.triangle_mesh import TriangleMesh

SKEW = MP.rotation(40.0, (1.0, 2.0, 0.5))
UPLOAD, POSE = ("upload",), ("pose",)


class StandIn:
    """Records the calls upload() makes, in order, and returns 0 -- or, once, `fail_next`'s error code."""

    def __init__(self):
        self.calls = []
        self.fail_next = None

    def take(self):
        out, self.calls = self.calls, []
        return out

    def _done(self, name, what):
        self.calls.append(what)
        if self.fail_next == name:
            self.fail_next = None
            return N.ERR_ARG
        return 0

    def srt_last_error(self):
        return b"stand-in refusal"

    def srt_upload_scene(self, ctx, desc):
        return self._done("upload", UPLOAD)

    def srt_deform_topology(self, ctx, first, count, n_verts, corners, center, flags):
        return self._done("topology", ("topology", (first, count)))

    def srt_deform_colliders(self, ctx, n, first, count, verts):
        first = (ctypes.c_int32 * n).from_address(first)
        count = (ctypes.c_int32 * n).from_address(count)
        return self._done("deform", ("deform", [(first[k], count[k]) for k in range(n)]))

    def srt_pose_colliders(self, ctx, n, first, count, poses):
        return self._done("pose", POSE)


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("upload_plan")
    out = {"ico1": str(d / "ico1.obj"), "tetra": str(d / "tetra.obj")}
    scenes.write_icosphere_obj(out["ico1"], subdiv=1)
    VR.write_tetrahedron_obj(out["tetra"])
    return out


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.delenv("SIGHTPY_DEVICES", raising=False)
    lib = StandIn()
    monkeypatch.setitem(B._STATE, "lib", lib)
    monkeypatch.setitem(B._STATE, "resident", {})
    for counter in ("uploads", "pose_calls", "deform_calls"):
        monkeypatch.setitem(B._STATE, counter, 0)
    return lib


CTX = ctypes.c_void_p(1)


def _calls(lib, scene, ctx=CTX, **kw):
    B.upload(scene, ctx=ctx, **kw)
    return lib.take()


def _deformed(mesh, how=MD.twist):
    mesh.set_vertices(how(mesh.file_vertices))
    return mesh


def _device_posed(mesh):
    """In the rest pose, but an entry of Lowered.posed from the first frame on."""
    mesh.set_pose(np.eye(3))
    return mesh


@pytest.mark.parametrize("which", ["tetra", "ico1"])
def test_first_frame_then_nothing_then_one_pose_call(lib, objs, which):
    sc = scenes.mesh_scene(objs[which])
    mesh = MD.mesh_of(sc)
    assert _calls(lib, sc) == [UPLOAD]
    assert _calls(lib, sc) == []
    mesh.set_pose(SKEW, (0.1, 0.0, 0.2))
    assert _calls(lib, sc) == [POSE]
    assert _calls(lib, sc) == []
    mesh.set_pose(np.eye(3))
    assert _calls(lib, sc) == [POSE]
    mesh.reset_pose()  # (the same poses as np.eye(3): nothing)
    assert _calls(lib, sc) == []
    assert (B._STATE["uploads"], B._STATE["pose_calls"], B._STATE["deform_calls"]) == (1, 2, 0)


@pytest.mark.parametrize("which", ["tetra", "ico1"])
def test_vertices_changed_topology_once_then_deform_alone(lib, objs, which):
    sc = scenes.mesh_scene(objs[which])
    mesh = _device_posed(MD.mesh_of(sc))
    rng = MD.mesh_range(sc)
    assert _calls(lib, sc) == [UPLOAD]
    _deformed(mesh)
    assert _calls(lib, sc) == [("topology", rng), ("deform", [rng])]
    assert _calls(lib, sc) == []
    _deformed(mesh, MD.bulge)
    assert _calls(lib, sc) == [("deform", [rng])]
    mesh.reset_vertices()
    assert _calls(lib, sc) == [("deform", [rng])]
    assert _calls(lib, sc) == []
    assert (B._STATE["uploads"], B._STATE["pose_calls"], B._STATE["deform_calls"]) == (1, 0, 3)


def test_a_mesh_that_becomes_device_posed_after_the_upload_is_posed_once(lib, objs):
    """The resident poses name the ranges: a mesh uploaded as an ordinary one and then deformed is a new entry of
    them, so its first deformed frame makes one pose call (with the identity) as well."""
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = MD.mesh_of(sc)
    rng = MD.mesh_range(sc)
    assert _calls(lib, sc) == [UPLOAD]
    _deformed(mesh)
    assert _calls(lib, sc) == [("topology", rng), ("deform", [rng]), POSE]
    _deformed(mesh, MD.bulge)
    assert _calls(lib, sc) == [("deform", [rng])]


def test_first_frame_of_a_deformed_and_posed_mesh(lib, objs):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _deformed(MD.mesh_of(sc))
    mesh.set_pose(SKEW)
    rng = MD.mesh_range(sc)
    assert _calls(lib, sc) == [UPLOAD, ("topology", rng), ("deform", [rng]), POSE]
    assert _calls(lib, sc) == []


def test_vertices_changed_under_a_pose_deform_then_pose(lib, objs):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _deformed(MD.mesh_of(sc))
    mesh.set_pose(SKEW, (0.25, 0.1, 0.2))
    rng = MD.mesh_range(sc)
    _calls(lib, sc)
    _deformed(mesh, MD.bulge)
    assert _calls(lib, sc) == [("deform", [rng]), POSE]
    assert _calls(lib, sc) == []
    # under the identity pose the deform call leaves the range where it is wanted: no pose call
    mesh.reset_pose()
    assert _calls(lib, sc) == [POSE]
    _deformed(mesh)
    assert _calls(lib, sc) == [("deform", [rng])]


def test_two_meshes_only_the_changed_one_is_deformed(lib, objs):
    sc = scenes.mesh_scene(objs["ico1"])
    one = _device_posed(MD.mesh_of(sc, 0))
    sc.add(TriangleMesh(objs["tetra"], center=vec3(-0.3, 0.1, -0.2), material=one.material, max_ray_depth=3))
    other = MD.mesh_of(sc, 1)
    r0, r1 = MD.mesh_range(sc, 0), MD.mesh_range(sc, 1)
    _deformed(other)
    assert _calls(lib, sc) == [UPLOAD, ("topology", r1), ("deform", [r1])]
    _deformed(one)
    _deformed(other, MD.bulge)
    assert _calls(lib, sc) == [("topology", r0), ("deform", [r0, r1])]
    _deformed(one, MD.bulge)
    assert _calls(lib, sc) == [("deform", [r0])]


@pytest.mark.parametrize("how", ["invalidate", "rotate"])
def test_invalidate_or_rotate_of_a_deformed_mesh_uploads(lib, objs, how):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _deformed(MD.mesh_of(sc))
    _calls(lib, sc)
    if how == "invalidate":
        mesh.invalidate()
    else:
        mesh.rotate(30.0, vec3(0.0, 1.0, 0.0))
    assert _calls(lib, sc) == [UPLOAD]
    assert B.resident(CTX).verts == {} and B.resident(CTX).topology == set()
    assert _calls(lib, sc) == []


@pytest.mark.parametrize("posed", [False, True])
def test_a_fresh_scene_with_an_equal_signature_while_a_deformed_range_is_resident(lib, objs, posed):
    from sightpy._lower import lower_scene

    sc = scenes.plain_mesh_scene(objs["ico1"])
    _deformed(MD.mesh_of(sc))
    rng = MD.mesh_range(sc)
    assert _calls(lib, sc) == [UPLOAD, ("topology", rng), ("deform", [rng])]
    fresh = scenes.plain_mesh_scene(objs["ico1"])
    if posed:  # device-posed, in the rest pose and the loaded shape: an entry of Lowered.posed without vertices
        MD.mesh_of(fresh).set_pose(np.eye(3))
    assert lower_scene(fresh).signature() == lower_scene(sc).signature()  # (what makes the case)
    assert _calls(lib, fresh) == [UPLOAD]
    assert _calls(lib, fresh) == []
    # the deformed scene after it: the tables are resident, the topology went with the upload (and after the plain
    # scene, which names no posed range, the mesh is a new entry of the resident poses: one identity pose call)
    assert _calls(lib, sc) == [("topology", rng), ("deform", [rng])] + ([] if posed else [POSE])
    assert _calls(lib, sc) == []


def test_force_uploads_and_empties_the_topology_set(lib, objs):
    sc = scenes.mesh_scene(objs["ico1"])
    _deformed(MD.mesh_of(sc))
    rng = MD.mesh_range(sc)
    _calls(lib, sc)
    assert B.resident(CTX).topology == {rng}
    lib.fail_next = "topology"  # (stops upload() between the upload and the registration)
    with pytest.raises(N.SrtError):
        B.upload(sc, force=True, ctx=CTX)
    assert lib.take() == [UPLOAD, ("topology", rng)]
    assert B.resident(CTX).topology == set() and B.resident(CTX).verts == {}
    assert _calls(lib, sc) == [("topology", rng), ("deform", [rng])]
    assert _calls(lib, sc, force=True) == [UPLOAD, ("topology", rng), ("deform", [rng])]
    assert _calls(lib, sc) == []


def test_two_contexts_keep_independent_records(lib, objs):
    one, two = ctypes.c_void_p(1), ctypes.c_void_p(2)
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _device_posed(MD.mesh_of(sc))
    rng = MD.mesh_range(sc)
    assert _calls(lib, sc, ctx=one) == [UPLOAD]
    _deformed(mesh)
    assert _calls(lib, sc, ctx=two) == [UPLOAD, ("topology", rng), ("deform", [rng])]
    assert _calls(lib, sc, ctx=one) == [("topology", rng), ("deform", [rng])]
    mesh.set_pose(SKEW)
    assert _calls(lib, sc, ctx=two) == [POSE]
    assert _calls(lib, sc, ctx=two) == []
    assert _calls(lib, sc, ctx=one) == [POSE]
    assert B.resident(one) is not B.resident(two) and B.resident(one).scene == B.resident(two).scene
    B.forget_resident(one)
    assert _calls(lib, sc, ctx=two) == []
    assert _calls(lib, sc, ctx=one) == [UPLOAD, ("topology", rng), ("deform", [rng]), POSE]


@pytest.mark.parametrize("failing", ["deform", "pose", "upload"])
def test_a_call_that_raises_is_made_again_by_the_next_upload(lib, objs, failing):
    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _deformed(MD.mesh_of(sc))
    mesh.set_pose(SKEW)
    rng = MD.mesh_range(sc)
    _calls(lib, sc)
    _deformed(mesh, MD.bulge)
    before = (B._STATE["uploads"], B._STATE["deform_calls"], B._STATE["pose_calls"])
    lib.fail_next = failing
    with pytest.raises(N.SrtError, match="stand-in refusal"):
        B.upload(sc, force=failing == "upload", ctx=CTX)
    assert lib.take() == {"deform": [("deform", [rng])], "pose": [("deform", [rng]), POSE], "upload": [UPLOAD]}[failing]
    # the call that raised was not counted, and the next upload() makes it and what follows it again
    after = (B._STATE["uploads"], B._STATE["deform_calls"], B._STATE["pose_calls"])
    assert after == (before[0], before[1] + (failing == "pose"), before[2])
    again = _calls(lib, sc)
    assert again == {"deform": [("deform", [rng]), POSE], "pose": [POSE],
                     "upload": [UPLOAD, ("topology", rng), ("deform", [rng]), POSE]}[failing]
    assert _calls(lib, sc) == []


def test_forget_resident_makes_the_next_upload_upload(lib, objs):
    sc = scenes.mesh_scene(objs["tetra"])
    assert _calls(lib, sc) == [UPLOAD]
    B.forget_resident()
    assert _calls(lib, sc) == [UPLOAD]
    B.forget_resident(CTX)
    assert _calls(lib, sc) == [UPLOAD]
    assert _calls(lib, sc) == []


def test_the_plan_is_pure(lib, objs):
    from sightpy._lower import lower_scene

    sc = scenes.mesh_scene(objs["ico1"])
    mesh = _deformed(MD.mesh_of(sc))
    mesh.set_pose(SKEW)
    rng = MD.mesh_range(sc)
    res, L = B.Resident(), lower_scene(sc)
    steps = B.plan_upload(res, L)
    assert [s[0] for s in steps] == ["upload", "topology", "deform", "pose"]
    assert steps[0][1] == L.signature() and steps[1][1] == rng and steps[2][1] == [rng]
    assert B.plan_upload(res, L) == steps and lib.take() == []
    assert (res.scene, res.poses, res.verts, res.topology, res.per_hit_inputs) == (None, (), {}, set(), False)
