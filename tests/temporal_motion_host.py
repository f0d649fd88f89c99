"""hc_temporal (rt_hostcheck.cpp) with a motion table: tests/temporal_host.py's call with srt_temporal_args'
`motion` / `n_motion` filled in, so the CPU suite runs temporal_pixel<true> of csrc/rt_denoise.h."""
import ctypes

import numpy as np

import hostcheck as HC
import temporal_host as TH
import temporal_ref as TR
from sightpy import _native as N


def accumulate(A, B, guides, W, H, history=None, prev_cam=None, demodulate=False, max_history=TR.DEFAULTS["max_history"],
               normal_max=TR.DEFAULTS["normal_max"], plane_max=TR.DEFAULTS["plane_max"], motion=None, n_motion=None):
    """hc_temporal with temporal_motion_ref.accumulate's arguments and result.  `n_motion`: the count passed, when
    it is not the table's own (the argument checks)."""
    lib = HC.lib()
    lib.hc_temporal.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(N.TemporalArgs)]
    a, keep = N.TemporalArgs(), []
    out = TH.fill_args(a, keep, A, B, guides, W, H, history, prev_cam, demodulate, max_history, normal_max, plane_max)
    if motion is not None:
        motion = np.ascontiguousarray(motion, dtype=np.float64).reshape(-1, 12)
        keep.append(motion)
        a.motion, a.n_motion = N.ptr(motion), (len(motion) if n_motion is None else n_motion)
    rc = lib.hc_temporal(W, H, ctypes.byref(a))
    if rc:
        assert rc == N.ERR_ARG
        raise ValueError(lib.hc_last_error().decode())
    return out
