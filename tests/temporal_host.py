"""The host check harness' hc_temporal (rt_hostcheck.cpp): srt_temporal_accumulate's per-pixel function of
csrc/rt_denoise.h compiled for the CPU and driven sequentially, so the CPU suite checks the kernel's math against
tests/temporal_ref.py without a GPU."""
import ctypes

import numpy as np

import hostcheck as HC
import temporal_ref as TR
from sightpy import _native as N


def camera_desc(cam):
    """srt_camera of a temporal_ref.camera_dict (xs / ys NULL: the projection does not read them)."""
    d = N.CameraDesc()
    d.look_from[:], d.right[:], d.up[:], d.fwd_fd[:] = (list(cam[k]) for k in ("look_from", "right", "up", "fwd_fd"))
    d.cam_width, d.cam_height = cam["cam_width"], cam["cam_height"]
    d.focal_distance = cam["focal_distance"]
    return d


def fill_args(a, keep, A, B, guides, W, H, history, prev_cam, demodulate, max_history, normal_max, plane_max):
    """The inputs and parameters of an srt_temporal_args from host arrays (kept alive in `keep`), and new host
    output arrays: {"a", "b", "hist_a", "hist_b", "len"}."""
    n = W * H

    def put(field, v, dtype=np.float64):
        v = np.ascontiguousarray(v, dtype=dtype)
        keep.append(v)
        setattr(a, field, N.ptr(v))

    put("rgb_a", A)
    put("rgb_b", B)
    put("hit_id", guides["hit_id"], np.int32)
    for k in ("position", "normal", "depth"):
        put(k, guides[k])
    if demodulate:
        put("albedo", guides["albedo"])
    if history is not None:
        for field, k in (("hist_a", "a"), ("hist_b", "b"), ("hist_len", "len"), ("hist_position", "position"),
                         ("hist_normal", "normal")):
            put(field, history[k])
        put("hist_hit_id", history["hit_id"], np.int32)
        cd = camera_desc(prev_cam)
        cd.width, cd.height = W, H
        keep.append(cd)
        a.prev_cam = ctypes.pointer(cd)
    a.max_history, a.flags = int(max_history), (N.TEMPORAL_DEMODULATE if demodulate else 0)
    a.normal_max, a.plane_max = float(normal_max), float(plane_max)
    out = {k: np.empty((3, n) if k != "len" else n) for k in TR.OUTPUTS}
    for k, v in out.items():
        setattr(a, "out_" + k, N.ptr(v))
    return out


def accumulate(A, B, guides, W, H, history=None, prev_cam=None, demodulate=False, max_history=TR.DEFAULTS["max_history"],
               normal_max=TR.DEFAULTS["normal_max"], plane_max=TR.DEFAULTS["plane_max"]):
    """hc_temporal with temporal_ref.accumulate's arguments and result."""
    lib = HC.lib()
    lib.hc_temporal.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(N.TemporalArgs)]
    a, keep = N.TemporalArgs(), []
    out = fill_args(a, keep, A, B, guides, W, H, history, prev_cam, demodulate, max_history, normal_max, plane_max)
    rc = lib.hc_temporal(W, H, ctypes.byref(a))
    if rc:
        raise ValueError(lib.hc_last_error().decode())
    return out
