"""The host check harness' denoiser entry points (rt_hostcheck.cpp hc_aovs / hc_denoise): the per-pixel
functions of csrc/rt_denoise.h compiled for the CPU and driven sequentially, so the CPU suite checks the
kernels' math against tests/denoise_ref.py without a GPU."""
import ctypes

import numpy as np

import hostcheck as HC
from sightpy import _native as N
from sightpy._lower import lower_scene, camera_desc


def _lib():
    lib = HC.lib()
    lib.hc_aovs.argtypes = [ctypes.POINTER(N.SceneDesc), ctypes.POINTER(N.CameraDesc), ctypes.POINTER(N.AovOut)]
    lib.hc_denoise.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(N.DenoiseArgs)]
    return lib


def aovs(scene):
    """hc_aovs: {"hit_id", "depth", "position", "normal", "albedo"} of `scene`."""
    lib = _lib()
    L = lower_scene(scene)
    d = L.desc()
    cd = camera_desc(scene.camera)
    n = int(scene.camera.screen_width) * int(scene.camera.screen_height)
    res = {"hit_id": np.empty(n, dtype=np.int32), "depth": np.empty(n), "position": np.empty((3, n)),
           "normal": np.empty((3, n)), "albedo": np.empty((3, n))}
    out = N.AovOut()
    for k, v in res.items():
        setattr(out, k, N.ptr(v))
    rc = lib.hc_aovs(ctypes.byref(d), ctypes.byref(cd), ctypes.byref(out))
    if rc:
        raise RuntimeError(lib.hc_last_error().decode())
    return res


def denoise(rgb, guides, W, H, levels=4, sigma_color=1.0, sigma_normal=0.35, sigma_albedo=0.1, sigma_plane=0.02,
            rgbx=False):
    """hc_denoise: (filtered rgb (3, W*H), uint8 image (H, W, 3 or 4))."""
    lib = _lib()
    n = W * H
    keep = [np.ascontiguousarray(rgb, dtype=np.float64)] + \
           [np.ascontiguousarray(guides[k], dtype=np.float64) for k in ("normal", "albedo", "position", "depth")]
    a = N.DenoiseArgs()
    a.rgb, a.normal, a.albedo, a.position, a.depth = (N.ptr(v) for v in keep)
    a.levels, a.flags = int(levels), (N.DENOISE_RGBX if rgbx else 0)
    a.sigma_color, a.sigma_normal, a.sigma_albedo, a.sigma_plane = sigma_color, sigma_normal, sigma_albedo, sigma_plane
    out = np.empty((3, n))
    u8 = np.empty((n, 4 if rgbx else 3), dtype=np.uint8)
    a.out_rgb, a.out_srgb8 = N.ptr(out), N.ptr(u8)
    rc = lib.hc_denoise(W, H, ctypes.byref(a))
    if rc:
        raise ValueError(lib.hc_last_error().decode())
    return out, u8.reshape(H, W, -1)
