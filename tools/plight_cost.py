"""Cost of a positional light: example1's scene (1920x1080, depth 5, 6 spp) rendered with its
directional light, with that light replaced by a PositionalLight above the spheres, and with a
SpotLight there, on the same build -- pipelined frames as bench.py's headline queues them (numpy's
jitter stream generated on the device, the uint8 image to pinned host memory, the linear RGB kept in
HBM).

The directional frame runs the kernel specialised for example1's collider sequence under its register
cap (k_primary_lean); the positional and spot frames run the fused k_primary of the
MATS_GLOSSY_SKY | MAT_PLIGHT variant, which intersects the colliders in the loop.  Part of the ratio is
therefore the variant, not the light: `directional_loop` renders the directional frame with the
collider sequences switched off (option "collider_seq" = 0), which tells the two apart.

    python tools/plight_cost.py [--steps 300] [--warmup 300] [--size 1920x1080] [--depth 5] [--spp 6]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))


def example1_with(kind, W, H, depth):
    import scenes
    from sightpy import rgb, vec3

    sc = scenes.example1(W, H, depth)
    if kind == "directional":
        return sc
    sc.Light_list.clear()
    if kind == "positional":
        sc.add_PositionalLight(pos=vec3(0.25, 2.5, -2.0), color=rgb(0.15, 0.15, 0.15), intensity=8.0)
    else:
        sc.add_SpotLight(pos=vec3(0.25, 2.5, -2.0), direction=vec3(0.0, -1.0, -0.35), color=rgb(0.15, 0.15, 0.15),
                         inner_deg=25.0, outer_deg=40.0, intensity=8.0)
    return sc


def main():
    from vattr_cost import frames_ms
    from sightpy import _backend as B, _native as N

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--spp", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3, help="timed runs per scene (median and spread reported)")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    out = {"what": "example1 frame, pipelined, ms per frame: directional / positional / spot light",
           "size": [W, H], "depth": a.depth, "spp": a.spp, "steps": a.steps, "warmup": a.warmup}
    lib, ctx = B.context()
    for name in ("directional", "directional_loop", "positional", "spot"):
        sc = example1_with(name.split("_")[0], W, H, a.depth)
        N.check(lib, lib.srt_set_option(ctx, b"collider_seq", 0 if name == "directional_loop" else 1))
        runs = []
        for r in range(a.repeats):
            ms, rays, kpath = frames_ms(sc, a.spp, a.steps, a.warmup if r == 0 else 20)
            runs.append(round(ms, 4))
        out[name] = {"ms_runs": runs, "ms_median": sorted(runs)[len(runs) // 2],
                     "ms_spread": round(max(runs) - min(runs), 4), "rays_per_frame": int(rays), "kernel_path": kpath}
    N.check(lib, lib.srt_set_option(ctx, b"collider_seq", 1))
    for name in ("directional_loop", "positional", "spot"):
        out[name + "_over_directional"] = round(out[name]["ms_median"] / out["directional"]["ms_median"], 4)
    out["positional_over_directional_loop"] = round(out["positional"]["ms_median"] / out["directional_loop"]["ms_median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
