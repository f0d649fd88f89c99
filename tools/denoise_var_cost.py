"""Cost of the half-frame denoiser (srt_denoise_var) on this GPU beside srt_denoise's, in one session:

1. at 1920x1080, on the guide images and two 1-sample half-frames of example1 and of the cornell box, kept in
   device memory: srt_denoise's levels on the mean (the yardstick, tools/denoise_cost.py filter_times), then for
   each flag combination k_dn_prepare, each k_atrous level, the finish (k_dn_finish or k_denoise_resolve: the
   chain less the prepare kernel and the levels) and the whole chain, by HIP events, median of --repeats;
2. cornell at 800x800, 16 samples through Scene.render: denoise=True against the half-frame mode, wall clock,
   alternating, --runs each.

    python tools/denoise_var_cost.py [--size 1920x1080] [--levels 5] [--repeats 7] [--out profiles/denoise_var_cost.json]
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

from denoise_cost import filter_times, median  # noqa: E402


def var_times(B, N, W, H, dev, levels, repeats, variance, demodulate):
    """srt_denoise_var on device arrays: ms per level, prepare, finish and chain (median of `repeats` after a warm-up)."""
    lib, ctx = B.context()
    n = W * H
    a = N.DenoiseVarArgs()
    a.rgb_a, a.rgb_b = dev["a"].value, dev["b"].value
    for k in ("normal", "albedo", "position", "depth"):
        setattr(a, k, dev[k].value)
    a.spp_a = a.spp_b = 1
    a.levels = levels
    a.flags = N.DENOISE_RGBX | (N.DENOISE_VARIANCE if variance else 0) | (N.DENOISE_DEMODULATE if demodulate else 0)
    for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_plane"):
        setattr(a, k, N.DENOISE_DEFAULTS[k])
    a.sigma_lum = N.DENOISE_VAR_DEFAULTS["sigma_lum"]
    a.out_rgb = B.device_buffer("cost_out", 24 * n).value
    a.out_srgb8 = B.device_buffer("cost_u8", 4 * n).value
    ms = np.zeros(levels + 2)
    a.ms_levels = N.ptr(ms)
    runs, walls = [], []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        N.check(lib, lib.srt_denoise_var(ctx, W, H, ctypes.byref(a)))
        walls.append((time.perf_counter() - t0) * 1e3)
        runs.append(ms.copy())
    runs, walls = np.array(runs[1:]), walls[1:]
    finish = runs[:, levels] - runs[:, levels + 1] - runs[:, :levels].sum(axis=1)
    return {"ms_levels": [round(float(median(list(runs[:, l]))), 4) for l in range(levels)],
            "ms_prepare": round(float(median(list(runs[:, levels + 1]))), 4),
            "ms_finish": round(float(median(list(finish))), 4),
            "ms_chain": round(float(median(list(runs[:, levels]))), 4),
            "ms_wall_call": round(median(walls), 4)}


def main():
    import scenes
    from sightpy import _backend as B, _native as N

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cornell", default="800x800:16", help="WxH:spp through Scene.render ('' skips it)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    n = W * H
    out = {"what": "srt_denoise_var beside srt_denoise, ms by HIP events (median of %d runs, one session)" % a.repeats,
           "size": [W, H], "levels": a.levels}
    lib, ctx = B.context()
    for name in ("example1", "cornell"):
        sc = getattr(scenes, name)(W, H)
        aovs = B.render_aovs(sc)
        A, Bh, _, _, _ = B.render_halves(sc, 2, rng="device", seed=1)
        dev = {}
        for k, v in (("a", A), ("b", Bh), ("rgb", (A + Bh) / 2), ("normal", aovs["normal"]), ("albedo", aovs["albedo"]),
                     ("position", aovs["position"]), ("depth", aovs["depth"])):
            v = np.ascontiguousarray(v)
            dev[k] = B.device_buffer("cost_" + k, v.nbytes)
            N.check(lib, lib.srt_memcpy(ctx, dev[k], N.ptr(v), v.nbytes))
        res = {"srt_denoise": filter_times(B, N, W, H, {k: dev[k] for k in ("rgb", "normal", "albedo", "position", "depth")},
                                           a.levels, a.repeats)}
        base = res["srt_denoise"]["ms_levels"]
        for variance, demodulate in ((False, False), (True, False), (False, True), (True, True)):
            r = var_times(B, N, W, H, dev, a.levels, a.repeats, variance, demodulate)
            r["level_over_srt_denoise_level"] = [round(x / y, 3) for x, y in zip(r["ms_levels"], base)]
            res["variance=%d demodulate=%d" % (variance, demodulate)] = r
        out[name] = res
    for k in list(dev) + ["out", "u8"]:
        B.release_buffer("cost_" + k)
    if a.cornell:
        size, spp = a.cornell.split(":")
        cw, ch = (int(v) for v in size.lower().split("x"))
        csc = scenes.cornell(cw, ch)
        modes = (("denoise=True", True), ("variance+demodulate", {"variance": True, "demodulate": True}))
        for _, dn in modes:
            csc.render(2, denoise=dn)  # warm-up: context, kernels, buffers
        res = {name: [] for name, _ in modes}
        for r in range(a.runs):
            for name, dn in modes:
                np.random.seed(1)
                t0 = time.perf_counter()
                csc.render(int(spp), denoise=dn)
                wall = time.perf_counter() - t0
                st = csc.last_stats
                row = {"wall_s": round(wall, 4), "render_ms_device": round(st["ms_device"], 3),
                       "render_ms_wall": round(st["ms_wall"], 3)}
                row["denoise"] = {k: (v if not isinstance(v, list) else [round(x, 4) for x in v])
                                  for k, v in st["denoise"].items()}
                res[name].append(row)
        out["cornell_%s_%sspp" % (size, spp)] = res
        out["cornell_wall_s_median"] = {name: median([r["wall_s"] for r in rows]) for name, rows in res.items()}
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
