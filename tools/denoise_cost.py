"""Cost of the denoiser (srt_render_aovs, srt_denoise) on this GPU, by HIP events:

1. at 1920x1080, on the guide images and a 2-sample frame of example1 and of the cornell box, kept in
   device memory: k_aov,
   each filter level and the whole filter chain, each level beside its compulsory traffic -- 13 planes
   read and 3 written, 128 B per pixel;
2. cornell at 800x800: 16 samples + denoise against 512 samples plain, from Scene.last_stats and by wall
   clock.

    python tools/denoise_cost.py [--size 1920x1080] [--levels 5] [--repeats 7] [--out profiles/denoise_cost.json]
"""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))


def median(v):
    return sorted(v)[len(v) // 2]


def filter_times(B, N, W, H, planes, levels, repeats):
    """srt_denoise on device arrays: per-level and whole-chain ms (median of `repeats`, after one warm-up)."""
    lib, ctx = B.context()
    n = W * H
    a = N.DenoiseArgs()
    for k, v in planes.items():
        setattr(a, k, v.value)
    a.levels, a.flags = levels, N.DENOISE_RGBX
    a.sigma_color, a.sigma_normal, a.sigma_albedo, a.sigma_plane = (N.DENOISE_DEFAULTS[k] for k in (
        "sigma_color", "sigma_normal", "sigma_albedo", "sigma_plane"))
    a.out_rgb = B.device_buffer("cost_out", 24 * n).value
    a.out_srgb8 = B.device_buffer("cost_u8", 4 * n).value
    ms = np.zeros(levels + 1)
    a.ms_levels = N.ptr(ms)
    runs, walls = [], []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        N.check(lib, lib.srt_denoise(ctx, W, H, ctypes.byref(a)))
        walls.append((time.perf_counter() - t0) * 1e3)
        runs.append(ms.copy())
    runs, walls = np.array(runs[1:]), walls[1:]
    gb = 128.0 * n / 1e9
    per_level = [round(float(median(list(runs[:, l]))), 4) for l in range(levels)]
    return {"ms_levels": per_level, "ms_chain": round(float(median(list(runs[:, levels]))), 4),
            "ms_chain_spread": round(float(runs[:, levels].max() - runs[:, levels].min()), 4),
            "ms_wall_call": round(median(walls), 4),
            "gb_per_s_of_compulsory_traffic": [round(gb / (v * 1e-3), 1) for v in per_level]}


def main():
    import scenes
    from sightpy import _backend as B, _native as N

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cornell", default="800x800:16:512", help="WxH:spp denoised:spp plain ('' skips it)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    n = W * H
    out = {"what": "denoiser cost, ms by HIP events (median of %d runs)" % a.repeats, "size": [W, H],
           "levels": a.levels, "compulsory_bytes_per_pixel_per_level": 128,
           "compulsory_gb_per_level": round(128.0 * n / 1e9, 4)}
    lib, ctx = B.context()
    # example1 (the sky fills part of the frame: background pixels are copied through) and the cornell
    # box (no background: every pixel takes its 25 taps)
    for name in ("example1", "cornell"):
        sc = getattr(scenes, name)(W, H)
        aov_ms = []
        for r in range(a.repeats + 1):
            aovs = B.render_aovs(sc)
            aov_ms.append(aovs["ms_kernel"])
        frame = B.render_scene(sc, 2, seed=1)
        planes = {}
        for k, v in (("rgb", frame.rgb), ("normal", aovs["normal"]), ("albedo", aovs["albedo"]),
                     ("position", aovs["position"]), ("depth", aovs["depth"])):
            v = np.ascontiguousarray(v)
            planes[k] = B.device_buffer("cost_" + k, v.nbytes)
            N.check(lib, lib.srt_memcpy(ctx, planes[k], N.ptr(v), v.nbytes))
        out[name] = {"k_aov_ms": round(median(aov_ms[1:]), 4),
                     "background_pixel_fraction": round(float((aovs["normal"] == 0.0).all(axis=0).mean()), 4),
                     "filter": filter_times(B, N, W, H, planes, a.levels, a.repeats)}
    for k in list(planes) + ["out", "u8"]:
        B.release_buffer("cost_" + k)
    if a.cornell:
        size, spp_dn, spp_plain = a.cornell.split(":")
        cw, ch = (int(v) for v in size.lower().split("x"))
        csc = scenes.cornell(cw, ch)
        csc.render(1, denoise=True)  # warm-up: context, kernels, buffers
        res = {}
        for name, spp, dn in (("denoised", int(spp_dn), True), ("plain", int(spp_plain), False)):
            np.random.seed(1)
            t0 = time.perf_counter()
            csc.render(spp, denoise=dn)
            wall = time.perf_counter() - t0
            st = csc.last_stats
            res[name] = {"spp": spp, "wall_s": round(wall, 4), "render_ms_device": round(st["ms_device"], 3),
                         "render_ms_wall": round(st["ms_wall"], 3)}
            if dn:
                res[name]["denoise"] = {k: (v if not isinstance(v, list) else [round(x, 4) for x in v])
                                        for k, v in st["denoise"].items()}
        res["plain_over_denoised_wall"] = round(res["plain"]["wall_s"] / res["denoised"]["wall_s"], 3)
        out["cornell_%s" % size] = res
    text = json.dumps(out, indent=1)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
