"""Cost of animating a TriangleMesh: the mesh bench's frame (scenes.mesh_bench: a 20,480-triangle icosphere in
the ex1 setting, 1920x1080, depth 3, 2 spp) with the mesh posed on the device (TriangleMesh.set_pose ->
srt_pose_colliders) against the same mesh rotated on the host (TriangleMesh.rotate, then a full lowering and
upload).  On a tree without set_pose (the parent commit) only the host-rotated figures are measured, so the same
file run from both trees on one box gives the comparison.

    the pipelined frame (bench.py's mesh line: numpy's jitter stream generated on the device, the uint8 image to
        pinned host memory) of the static scene and after poses of 0, 30 and 90 degrees about a skew axis
    device time of k_pose_triangles and of the summed k_bvh_refit launches, by HIP events (srt_debug_pose_times)
    host time per animated frame, split: moving the mesh (set_pose / rotate), lowering (lower_scene + signature),
        the pose call or the upload, the render call

    python tools/mesh_pose_cost.py [--steps 300] [--warmup 300] [--size 1920x1080] [--subdiv 5] [--frames 5]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests", ROOT):
    sys.path.insert(0, str(p))

from vattr_cost import frames_ms  # noqa: E402  (tools/ is the script's directory)

AXIS = (1.0, 2.0, 0.5)


def rotation(deg, axis=AXIS):
    import numpy as np

    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    t = np.deg2rad(deg)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def runs(sc, a, first=True):
    out = []
    for r in range(a.repeats):
        ms, rays, kpath = frames_ms(sc, a.spp, a.steps, a.warmup if (first and r == 0) else 20)
        out.append(round(ms, 4))
    return {"ms_runs": out, "ms_median": sorted(out)[len(out) // 2], "ms_range": round(max(out) - min(out), 4),
            "rays_per_frame": int(rays), "kernel_path": kpath}


def host_frames(sc, mesh, a, posed):
    """Host seconds per animated frame over `a.frames` frames, by part (medians)."""
    import numpy as np
    from sightpy import _backend as B, vec3
    from sightpy._lower import lower_scene

    parts = {"move": [], "lowering": [], "pose_or_upload": [], "render": [], "total": []}
    for k in range(a.frames + 1):
        t0 = time.perf_counter()
        if posed:
            mesh.set_pose(rotation(5.0 * (k + 1)))
        else:
            mesh.rotate(5.0, vec3(*AXIS))
        t1 = time.perf_counter()
        L = lower_scene(sc)
        L.signature()
        t2 = time.perf_counter()  # (the lowering alone, timed apart: upload() below lowers again)
        B.upload(sc)
        t3 = time.perf_counter()
        np.random.seed(k)
        B.render_scene(sc, a.spp, mt=True, want_rgb=False)  # (its own upload() finds everything resident)
        t4 = time.perf_counter()
        if k == 0:
            continue  # (the first frame fills the record cache and sizes the buffers)
        low = t2 - t1
        parts["move"].append(t1 - t0)
        parts["lowering"].append(low)
        parts["pose_or_upload"].append(max(0.0, (t3 - t2) - low))
        parts["render"].append(max(0.0, (t4 - t3) - low))
        parts["total"].append((t1 - t0) + (t3 - t2) + max(0.0, (t4 - t3) - low))
    return {k: round(sorted(v)[len(v) // 2] * 1e3, 3) for k, v in parts.items()}


def main():
    import scenes
    from sightpy import _backend as B, _native as N
    from sightpy.geometry.triangle_mesh import TriangleMesh

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--subdiv", type=int, default=5)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per figure (median and range reported)")
    ap.add_argument("--frames", type=int, default=5, help="animated frames of the host-time split")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    sc = scenes.mesh_bench(W, H, 3, a.subdiv)
    mesh = next(p for p in sc.scene_primitives if isinstance(p, TriangleMesh))
    posed = hasattr(TriangleMesh, "set_pose")
    out = {"what": "mesh bench frame with a posed mesh: pipelined ms per frame, pose kernels' ms, host ms per animated frame",
           "tree": "set_pose" if posed else "parent (rotate on the host)", "size": [W, H],
           "triangles": 20 * 4 ** a.subdiv, "spp": a.spp, "steps": a.steps, "warmup": a.warmup}
    out["static"] = runs(sc, a)
    if posed:
        lib, ctx = B.context()
        for deg in (0, 30, 90):
            mesh.set_pose(rotation(float(deg)))
            r = runs(sc, a, first=False)  # (frames_ms uploads: here one srt_pose_colliders call)
            ms_pose, ms_refit, calls = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
            N.check(lib, lib.srt_debug_pose_times(ctx, ctypes.byref(ms_pose), ctypes.byref(ms_refit), ctypes.byref(calls)))
            r["ms_k_pose_triangles"], r["ms_k_bvh_refit_sum"] = round(ms_pose.value, 5), round(ms_refit.value, 5)
            out["posed_%d_deg" % deg] = r
        out["pose_calls"] = int(calls.value)
        mesh.reset_pose()
        out["posed_0_over_static"] = round(out["posed_0_deg"]["ms_median"] / out["static"]["ms_median"], 4)
    lib, ctx = B.context()
    N.check(lib, lib.srt_set_option(ctx, b"pipeline", 0))  # (frames_ms turned it on)
    out["host_ms_per_animated_frame"] = host_frames(sc, mesh, a, posed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
