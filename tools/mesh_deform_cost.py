"""Cost of deforming a TriangleMesh: the mesh bench's frame (scenes.mesh_bench: a 20,480-triangle icosphere in the
ex1 setting, 1920x1080, depth 3, 2 spp) with the mesh's vertices set on the device (TriangleMesh.set_vertices ->
srt_deform_colliders) against the only route without it: rewrite every Python Triangle_Collider from the new
vertices, invalidate(), lower in full and upload.  On a tree without set_vertices (the parent commit) only the static
frame and the host route are measured, so the same file run from both trees on one box gives the comparison.

    the pipelined frame (bench.py's mesh line: numpy's jitter stream generated on the device, the uint8 image to
        pinned host memory) of the static scene, after a zero deformation (the file's own vertices through the
        device) and after a twist of 30 degrees along the y axis (the tree keeps the loaded shape's topology); the
        static scene uploaded and timed once more afterwards, on both trees (what one process's figures move by
        on their own)
    device time of the normals step, the record kernel and the summed k_bvh_refit launches, by HIP events
        (srt_debug_deform_times), for the flat bench mesh and for the same mesh loaded with smooth=True
    host time per animated frame, split: moving the mesh (set_vertices / rewriting the colliders), lowering
        (lower_scene + signature), the deform call or the upload, the render call

    python tools/mesh_deform_cost.py [--steps 300] [--warmup 300] [--size 1920x1080] [--subdiv 5] [--frames 5]
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


def read_obj(path):
    """(vertices (n_v, 3), corner indices (n_f, 3)) of an OBJ file's `v` and `f` records."""
    import numpy as np

    V, F = [], []
    for line in open(path):
        tok = line.split()
        if tok and tok[0] == "v":
            V.append([float(x) for x in tok[1:4]])
        elif tok and tok[0] == "f":
            F.append([int(t.split("/")[0]) - 1 for t in tok[1:4]])
    return np.array(V, dtype=np.float64), np.array(F, dtype=np.int32)


def twist(V, deg_over_height):
    """Every vertex turned about the y axis by an angle proportional to its y: `deg_over_height` from the lowest to
    the highest vertex."""
    import numpy as np

    y = V[:, 1]
    a = np.deg2rad(deg_over_height) * (y - y.min()) / (y.max() - y.min())
    return np.stack([np.cos(a) * V[:, 0] + np.sin(a) * V[:, 2], y, -np.sin(a) * V[:, 0] + np.cos(a) * V[:, 2]], axis=1)


def runs(sc, a, first=True):
    out = []
    for r in range(a.repeats):
        ms, rays, kpath = frames_ms(sc, a.spp, a.steps, a.warmup if (first and r == 0) else 20)
        out.append(round(ms, 4))
    return {"ms_runs": out, "ms_median": sorted(out)[len(out) // 2], "ms_range": round(max(out) - min(out), 4),
            "rays_per_frame": int(rays), "kernel_path": kpath}


def rewrite_colliders(mesh, V, F):
    """The host route: every Python collider of the mesh recomputed in place from the vertices V (the constructor's
    verts[i] + center), then invalidate() where the tree has it."""
    from sightpy import vec3

    P = [vec3(*row) + mesh.center for row in V.tolist()]
    for c, (i, j, k) in zip(mesh.collider_list, F.tolist()):
        c.__init__(assigned_primitive=mesh, p1=P[i], p2=P[j], p3=P[k], normals=None, uvs=c.uvs)
    if hasattr(mesh, "invalidate"):
        mesh.invalidate()


def host_frames(sc, mesh, V, F, a, device):
    """Host seconds per animated frame over `a.frames` frames, by part (medians)."""
    import numpy as np
    from sightpy import _backend as B
    from sightpy._lower import lower_scene

    parts = {"move": [], "lowering": [], "deform_or_upload": [], "render": [], "total": []}
    for k in range(a.frames + 1):
        P = twist(V, 5.0 * (k + 1))
        t0 = time.perf_counter()
        if device:
            mesh.set_vertices(P)
        else:
            rewrite_colliders(mesh, P, F)
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
        parts["deform_or_upload"].append(max(0.0, (t3 - t2) - low))
        parts["render"].append(max(0.0, (t4 - t3) - low))
        parts["total"].append((t1 - t0) + (t3 - t2) + max(0.0, (t4 - t3) - low))
    return {k: round(sorted(v)[len(v) // 2] * 1e3, 3) for k, v in parts.items()}


def deform_times(lib, ctx):
    from sightpy import _native as N

    ms = [ctypes.c_double() for _ in range(3)]
    calls = ctypes.c_int64()
    N.check(lib, lib.srt_debug_deform_times(ctx, *[ctypes.byref(m) for m in ms], ctypes.byref(calls)))
    return {"ms_normals": round(ms[0].value, 5), "ms_k_deform_triangles": round(ms[1].value, 5),
            "ms_k_bvh_refit_sum": round(ms[2].value, 5)}, int(calls.value)


def main():
    import os
    import tempfile

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
    V, F = read_obj(os.path.join(tempfile.gettempdir(), "sightpy_icosphere_%d.obj" % a.subdiv))
    device = hasattr(TriangleMesh, "set_vertices")
    out = {"what": "mesh bench frame with a deformed mesh: pipelined ms per frame, deform kernels' ms, host ms per animated frame",
           "tree": "set_vertices" if device else "parent (colliders rewritten on the host)", "size": [W, H],
           "triangles": len(F), "vertices": len(V), "spp": a.spp, "steps": a.steps, "warmup": a.warmup}
    out["static"] = runs(sc, a)
    if device:
        lib, ctx = B.context()
        for name, P in (("zero_deformation", V), ("twist_30_deg", twist(V, 30.0))):
            mesh.set_vertices(P)
            r = runs(sc, a, first=False)  # (frames_ms uploads: here one srt_deform_colliders call)
            r["kernels"], calls = deform_times(lib, ctx)
            out[name] = r
        out["deform_calls"] = calls
        out["bytes_per_call"] = int(V.nbytes)
        out["zero_over_static"] = round(out["zero_deformation"]["ms_median"] / out["static"]["ms_median"], 4)
        # the normals step: the same mesh loaded smooth (area-weighted vertex normals), one call
        import vattr_ref as VR

        sc2 = VR.mesh_scene(os.path.join(tempfile.gettempdir(), "sightpy_icosphere_%d.obj" % a.subdiv), W, H, 3,
                            smooth=True)
        smooth = next(p for p in sc2.scene_primitives if isinstance(p, TriangleMesh))
        smooth.set_vertices(twist(V, 30.0))
        B.upload(sc2)
        out["smooth_twist_30_deg_kernels"] = deform_times(lib, ctx)[0]
        mesh.invalidate()  # (the deformation is dropped: the static scene is uploaded again)
    # the static frame once more, later in the process: how far one process's figures move on their own
    B.forget_resident()
    out["static_again"] = runs(sc, a, first=False)
    lib, ctx = B.context()
    N.check(lib, lib.srt_set_option(ctx, b"pipeline", 0))  # (frames_ms turned it on)
    if device:
        out["host_ms_per_animated_frame"] = host_frames(sc, mesh, V, F, a, True)
    # the host route, on either tree (on this one after invalidate(): the colliders are read again)
    if device:
        mesh.invalidate()
    route = host_frames(sc, mesh, V, F, a, False)
    if device:  # (the mesh is device-posed here: the timed lowering fills its record cache, so the split of the
        #          rest is another than on the parent's tree; the total holds)
        route = {k: route[k] for k in ("move", "total")}
    out["host_ms_per_animated_frame_host_route"] = route
    print(json.dumps(out))


if __name__ == "__main__":
    main()
