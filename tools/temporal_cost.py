"""Cost of the temporal accumulation pass (srt_temporal_accumulate, k_temporal) on this GPU, beside one filter
level as the yardstick, in one session:

1. at 1920x1080, on the guide images and two 1-sample half-frames of example1 and of the cornell box, everything in
   device memory: a previous frame from a slightly moved camera leaves its history (one call without history), then
   the current frame's call is timed -- k_temporal by HIP events, median of --repeats after a warm-up -- with and
   without SRT_TEMPORAL_DEMODULATE, and the first-frame call (no history: no gathers) with it; beside them one
   k_atrous<true> level (srt_denoise_var, levels 1, variance + demodulate; tools/denoise_var_cost.py var_times) on
   the same frame.  Also the share of surface pixels that found history.
2. cornell at 800x800, 16 samples through Scene.render: variance + demodulate with and without "temporal", wall
   clock, alternating, --runs each (the temporal frames accumulate on one another under an unchanged camera).
3. --motion (instead of 1 and 2): on the inputs of 1, the current frame's call with SRT_TEMPORAL_DEMODULATE without
   a motion table (k_temporal<false>) and with an all-identity table of one row per collider (k_temporal<true>),
   alternating, median of --repeats each.  The identity rows leave every tap where it is, so the two calls gather
   the same history and differ by the row loads and the 18 multiply-adds per pixel alone.

    python tools/temporal_cost.py [--size 1920x1080] [--repeats 7] [--out profiles/temporal_cost.json]
    python tools/temporal_cost.py --motion [--out profiles/temporal_motion_cost.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "python-raytracer_amd", ROOT / "oracle", ROOT / "tests", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))

from denoise_cost import median  # noqa: E402
from denoise_var_cost import var_times  # noqa: E402

# bytes per pixel: what a call must read and write at least (every plane once), and the most it can touch (each
# of the four taps of every history plane on its own)
STREAM_IN = 8 * (3 + 3 + 3 + 3 + 3 + 1) + 4       # A, B, normal, position, albedo, depth, hit_id
HISTORY = 8 * (3 + 3 + 1 + 3 + 3) + 4             # hist_a, hist_b, hist_len, hist_normal, hist_position, hist_hit_id
STORES = 8 * 13                                   # out_a, out_b, out_hist_a, out_hist_b, out_len
COMPULSORY, WORST = STREAM_IN + HISTORY + STORES, STREAM_IN + 4 * HISTORY + STORES


def moved(name, W, H, prev):
    """The scene `name`, and with `prev` its camera a little to the side (the previous frame's)."""
    import scenes
    import temporal_ref as TR
    from sightpy import vec3

    if name == "cornell":
        return TR.cornell_at(6 if prev else 0, W, H)
    sc = scenes.example1(W, H)
    if prev:
        c = sc.camera
        sc.add_Camera(look_from=c.look_from + vec3(0.02, 0.0, 0.0), look_at=c.look_at, screen_width=W, screen_height=H)
    return sc


def upload(B, N, tag, arrays):
    lib, ctx = B.context()
    dev = {}
    for k, v in arrays.items():
        v = np.ascontiguousarray(v, dtype=np.int32 if k == "hit_id" else np.float64)
        dev[k] = B.device_buffer("tcost_%s_%s" % (tag, k), v.nbytes)
        N.check(lib, lib.srt_memcpy(ctx, dev[k], N.ptr(v), v.nbytes))
    return dev


def timed(B, dev, W, H, out, repeats, **kw):
    """k_temporal's time; the rate is over the bytes the call must move (no history planes on a first frame, no
    albedo without the flag)."""
    bytes_pp = (COMPULSORY if kw.get("history") is not None else STREAM_IN + STORES) - (0 if kw.get("demodulate") else 24)
    runs = []
    for r in range(repeats + 1):
        ms = []
        B.temporal_accumulate(dev["a"], dev["b"], dev, W, H, out=out, timings=ms, **kw)
        runs.append(ms[0])
    runs = runs[1:]
    m = median(runs)
    n = W * H
    return {"ms_kernel": round(m, 4), "ms_spread": round(max(runs) - min(runs), 4),
            "gb_per_s_of_compulsory_traffic": round(bytes_pp * n / 1e9 / (m * 1e-3), 1)}


def motion_leg(B, N, dev, hit_id, W, H, out, repeats, **kw):
    """k_temporal<false> against k_temporal<true> with an identity table, alternating in one session."""
    from sightpy._motion import IDENTITY

    n = W * H
    rows = np.tile(IDENTITY, (int(hit_id.max()) + 1, 1))
    table = B.device_buffer("tcost_motion", rows.nbytes)
    lib, ctx = B.context()
    N.check(lib, lib.srt_memcpy(ctx, table, N.ptr(rows), rows.nbytes))
    runs = {False: [], True: []}
    lens = {}
    for r in range(repeats + 1):
        for on in (False, True):
            ms = []
            B.temporal_accumulate(dev["a"], dev["b"], dev, W, H, out=out, timings=ms,
                                  motion=(table, len(rows)) if on else None, **kw)
            runs[on].append(ms[0])
            if r == 0:
                with B.DeviceArrays() as pool:
                    lens[on] = pool.fetch(out["len"], (n,))
    res = {"rows": len(rows), "table_bytes": int(rows.nbytes), "same_out_len": bool(np.array_equal(lens[False], lens[True]))}
    for on, name in ((False, "k_temporal<false>"), (True, "k_temporal<true> identity table")):
        t = runs[on][1:]
        m = median(t)
        res[name] = {"ms_kernel": round(m, 4), "ms_spread": round(max(t) - min(t), 4),
                     "gb_per_s_of_compulsory_traffic": round(COMPULSORY * n / 1e9 / (m * 1e-3), 1)}
    res["true_over_false"] = round(res["k_temporal<true> identity table"]["ms_kernel"] / res["k_temporal<false>"]["ms_kernel"], 4)
    B.release_buffer("tcost_motion")
    return res


def main():
    from sightpy import _backend as B, _native as N
    from sightpy._lower import camera_desc

    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cornell", default="800x800:16", help="WxH:spp through Scene.render ('' skips it)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--motion", action="store_true", help="the motion leg alone (3. above)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    n = W * H
    out = {"what": "srt_temporal_accumulate beside one k_atrous<true> level, ms by HIP events (median of %d runs, one "
                   "session)" % a.repeats, "size": [W, H],
           "bytes_per_pixel": {"compulsory": COMPULSORY, "first_frame": STREAM_IN + STORES, "worst_case": WORST}}
    if a.motion:
        out["what"] = ("srt_temporal_accumulate without a motion table and with an all-identity one, alternating, ms by "
                       "HIP events (median of %d runs each, one session)" % a.repeats)
        a.cornell = ""
    names = set()
    for name in ("example1", "cornell"):
        frames = {}
        for tag, prev in (("prev", True), ("cur", False)):
            sc = moved(name, W, H, prev)
            aovs = B.render_aovs(sc)
            A, Bh, _, _, _ = B.render_halves(sc, 2, rng="device", seed=1 + prev)
            planes = {k: aovs[k] for k in ("hit_id", "position", "normal", "albedo", "depth")}
            frames[tag] = (upload(B, N, tag, dict(planes, a=A, b=Bh)), camera_desc(sc.camera))
        sets = [{k: B.device_buffer("tcost_out%d_%s" % (s, k), 8 * n * (1 if k == "len" else 3))
                 for k in ("a", "b", "hist_a", "hist_b", "len")} for s in (0, 1)]
        names.update("tcost_%s_%s" % (t, k) for t in ("prev", "cur") for k in frames["cur"][0])
        names.update("tcost_out%d_%s" % (s, k) for s in (0, 1) for k in sets[0])
        pdev, pcam = frames["prev"]
        cdev, _ = frames["cur"]
        B.temporal_accumulate(pdev["a"], pdev["b"], pdev, W, H, demodulate=True, out=sets[0])
        hist = {"a": sets[0]["hist_a"], "b": sets[0]["hist_b"], "len": sets[0]["len"], "hit_id": pdev["hit_id"],
                "position": pdev["position"], "normal": pdev["normal"]}
        if a.motion:
            out[name] = motion_leg(B, N, cdev, np.asarray(aovs["hit_id"]), W, H, sets[1], a.repeats, history=hist,
                                   prev_cam=pcam, demodulate=True)
            continue
        res = {"demodulate=1": timed(B, cdev, W, H, sets[1], a.repeats, history=hist, prev_cam=pcam, demodulate=True)}
        with B.DeviceArrays() as pool:
            ln = pool.fetch(sets[1]["len"], (n,))
            nm = pool.fetch(cdev["normal"], (3, n))
        surface = (nm != 0.0).any(axis=0)
        res["surface_pixels_with_history"] = round(float((ln[surface] > 1.0).mean()), 5)
        res["demodulate=0"] = timed(B, cdev, W, H, sets[1], a.repeats, history=hist, prev_cam=pcam, demodulate=False)
        res["first_frame demodulate=1"] = timed(B, cdev, W, H, sets[1], a.repeats, demodulate=True)
        lvl = var_times(B, N, W, H, cdev, 1, a.repeats, True, True)
        res["k_atrous<true> level 0"] = {"ms_kernel": lvl["ms_levels"][0], "ms_prepare": lvl["ms_prepare"]}
        res["temporal_over_filter_level"] = round(res["demodulate=1"]["ms_kernel"] / lvl["ms_levels"][0], 3)
        out[name] = res
    for k in sorted(names) + ["cost_out", "cost_u8"]:
        B.release_buffer(k)
    if a.cornell:
        import scenes

        size, spp = a.cornell.split(":")
        cw, ch = (int(v) for v in size.lower().split("x"))
        base = {"variance": True, "demodulate": True}
        modes = (("variance+demodulate", base), ("temporal+variance+demodulate", dict(base, temporal=True)))
        csc = scenes.cornell(cw, ch)
        for _, dn in modes:
            csc.render(2, denoise=dn)  # warm-up: context, kernels, buffers
        csc.reset_history()
        res = {name: [] for name, _ in modes}
        for r in range(a.runs):
            for name, dn in modes:
                np.random.seed(1 + r)
                t0 = time.perf_counter()
                csc.render(int(spp), denoise=dn)
                wall = time.perf_counter() - t0
                st = csc.last_stats
                row = {"wall_s": round(wall, 4), "render_ms_device": round(st["ms_device"], 3)}
                row["denoise"] = {k: (v if not isinstance(v, list) else [round(x, 4) for x in v])
                                  for k, v in st["denoise"].items()}
                res[name].append(row)
        csc.reset_history()
        out["cornell_%s_%sspp" % (size, spp)] = res
        out["cornell_wall_s_median"] = {name: median([r["wall_s"] for r in rows]) for name, rows in res.items()}
        out["cornell_ms_temporal_median"] = median([r["denoise"]["ms_temporal"] for r in res[modes[1][0]]])
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
