"""The host check harness' hc_denoise_var (rt_hostcheck.cpp): srt_denoise_var's per-pixel functions of
csrc/rt_denoise.h compiled for the CPU and driven sequentially, so the CPU suite checks the kernels' math
against tests/denoise_var_ref.py without a GPU."""
import ctypes

import numpy as np

import hostcheck as HC
from sightpy import _native as N


def fill_args(a, keep, A, B, ka, kb, guides, levels, variance, demodulate, rgbx, sigmas):
    """The inputs and parameters of an srt_denoise_var_args from host arrays (kept alive in `keep`)."""
    arrs = [np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)] + \
           [np.ascontiguousarray(guides[k], dtype=np.float64) for k in ("normal", "albedo", "position", "depth")]
    keep.extend(arrs)
    a.rgb_a, a.rgb_b, a.normal, a.albedo, a.position, a.depth = (N.ptr(v) for v in arrs)
    a.spp_a, a.spp_b, a.levels = int(ka), int(kb), int(levels)
    a.flags = (N.DENOISE_RGBX if rgbx else 0) | (N.DENOISE_VARIANCE if variance else 0) | \
              (N.DENOISE_DEMODULATE if demodulate else 0)
    for k in ("sigma_color", "sigma_lum", "sigma_normal", "sigma_albedo", "sigma_plane"):
        setattr(a, k, float(sigmas.get(k, N.DENOISE_VAR_DEFAULTS.get(k, N.DENOISE_DEFAULTS.get(k)))))


def denoise_var(A, B, ka, kb, guides, W, H, variance=False, demodulate=False, levels=4, rgbx=False, **sigmas):
    """hc_denoise_var: (c' (3, W*H), the last level's v (W*H,) or None, uint8 image (H, W, 3 or 4))."""
    lib = HC.lib()
    lib.hc_denoise_var.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(N.DenoiseVarArgs)]
    n = W * H
    a, keep = N.DenoiseVarArgs(), []
    fill_args(a, keep, A, B, ka, kb, guides, levels, variance, demodulate, rgbx, sigmas)
    out = np.empty((3, n))
    var = np.empty(n) if variance else None
    u8 = np.empty((n, 4 if rgbx else 3), dtype=np.uint8)
    a.out_rgb, a.out_variance, a.out_srgb8 = N.ptr(out), N.ptr(var), N.ptr(u8)
    rc = lib.hc_denoise_var(W, H, ctypes.byref(a))
    if rc:
        raise ValueError(lib.hc_last_error().decode())
    return out, var, u8.reshape(H, W, -1)
