"""Cost of smooth shading and texturing a TriangleMesh: the mesh bench's frame (scenes.mesh_bench:
a 20,480-triangle icosphere in the ex1 setting, 1920x1080, depth 3, 2 spp) rendered flat, with
interpolated vertex normals, and with vertex normals plus an image texture over `vt` coordinates, on
the same build -- pipelined frames as bench.py's mesh line queues them (numpy's jitter stream
generated on the device, the uint8 image to pinned host memory, the linear RGB kept in HBM).

    python tools/vattr_cost.py [--steps 300] [--warmup 300] [--size 1920x1080] [--subdiv 5]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests", ROOT):
    sys.path.insert(0, str(p))


def frames_ms(sc, spp, steps, warmup):
    """ms per frame of `steps` pipelined frames after `warmup` (bench.py's step / timed)."""
    import numpy as np
    from sightpy import _backend as B, _native as N

    lib, ctx = B.context()
    W, H = int(sc.camera.screen_width), int(sc.camera.screen_height)
    N.check(lib, lib.srt_set_option(ctx, b"pipeline", 1))
    B.upload(sc)
    cd = B.camera_desc(sc.camera)
    outs = []
    for _ in range(3):  # one image per frame in flight
        pu = ctypes.c_void_p()
        N.check(lib, lib.srt_host_alloc(ctx, 3 * W * H, ctypes.byref(pu)))
        outs.append(pu)
    np.random.seed(0)
    mt = N.MtState.from_numpy()
    a = N.RenderArgs()
    a.spp, a.sample_base, a.n_rows, a.batch_spp = spp, 0, H, 0
    a.rows, a.jitter, a.mt, a.seed = None, None, ctypes.pointer(mt), 12345
    a.out_hit_id, a.out_rgb = None, None
    k = 0

    def step(async_ok):
        nonlocal k
        a.out_srgb8 = outs[k % 3]
        k += 1
        a.flags = N.RENDER_RGB_LOCAL | (N.RENDER_ASYNC if async_ok else 0)
        N.check(lib, lib.srt_render(ctx, ctypes.byref(cd), ctypes.byref(a), None))

    def barrier(st=None):
        N.check(lib, lib.srt_render_finish(ctx, ctypes.byref(st) if st is not None else None))
        N.check(lib, lib.srt_synchronize(ctx))

    for w in range(max(1, warmup)):
        step(w > 0)  # the first frame runs synchronously (sizes queues and rings)
        if (w + 1) % 50 == 0:
            barrier()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(True)
    st = N.Stats()
    N.check(lib, lib.srt_render_finish(ctx, ctypes.byref(st)))
    el = time.perf_counter() - t0
    st = st.as_dict()
    for pu in outs:
        N.check(lib, lib.srt_host_free(ctx, pu))
    return el / steps * 1e3, st["total_rays"], st["kernel_path"]


def main():
    import vattr_ref as VR

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--subdiv", type=int, default=5)
    ap.add_argument("--spp", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per scene (median and spread reported)")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    path = os.path.join(tempfile.gettempdir(), "sightpy_smooth_icosphere_%d.obj" % a.subdiv)
    VR.write_smooth_icosphere_obj(path, a.subdiv)
    scenes = {
        "flat": VR.mesh_scene(path, W, H, 3, smooth=False),
        "smooth": VR.mesh_scene(path, W, H, 3, smooth=True),
        "smooth_textured": VR.mesh_scene(path, W, H, 3, smooth=True, texcoords=True, material=VR.checker()),
    }
    out = {"what": "mesh bench frame, pipelined, ms per frame: flat / smooth / smooth + image texture",
           "size": [W, H], "triangles": 20 * 4 ** a.subdiv, "spp": a.spp, "steps": a.steps, "warmup": a.warmup}
    for name, sc in scenes.items():
        runs = []
        for r in range(a.repeats):
            ms, rays, kpath = frames_ms(sc, a.spp, a.steps, a.warmup if r == 0 else 20)
            runs.append(round(ms, 4))
        out[name] = {"ms_runs": runs, "ms_median": sorted(runs)[len(runs) // 2], "rays_per_frame": int(rays),
                     "kernel_path": kpath}
    out["smooth_over_flat"] = round(out["smooth"]["ms_median"] / out["flat"]["ms_median"], 4)
    out["smooth_textured_over_flat"] = round(out["smooth_textured"]["ms_median"] / out["flat"]["ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
