"""The uint8 image on the device, byte for byte.

1. The arithmetic: resolve_pixel (rt_device.h) as k_denoise_resolve and k_dn_finish compile it, fed the
   boundary table, the random set and the special values of tests/resolve_ref.py as one frame through
   srt_denoise / srt_denoise_var at levels 0 (a pass-through) -- inside [lo, hi] of the exact rule everywhere,
   the one right byte wherever the value is unambiguous.
2. The stores: store_u8_tile / store_u8_chunk (rt_trace_kernels.h) at the frame shapes, sample counts and
   output addresses where they take their different paths.  A frame's bytes are classified against the
   kernel's own linear RGB, which no rendered value leaves ambiguous: a byte in the wrong place fails
   whatever its neighbours hold."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest

import denoise_ref as DR
import resolve_ref as R
import scenes
import sightpy_oracle as O
from test_gpu import ATOL, OPTION_KEYS, RTOL, _set_option

pytestmark = pytest.mark.gpu


def _backend():
    from sightpy import _backend

    return _backend


@contextmanager
def _options(**kv):
    try:
        for k, v in kv.items():
            _set_option(k, v)
        yield
    finally:
        for k in kv:
            _set_option(k, OPTION_KEYS[k])


# ---- 1. the arithmetic ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr():
    return R.frame()


def _guides(n):
    return {"normal": np.zeros((3, n)), "albedo": np.zeros((3, n)), "position": np.zeros((3, n)), "depth": np.zeros(n)}


def _denoise_device_pointers(rgb, guides, W, H, rgbx):
    """srt_denoise at levels 0 with every array in device memory: (out_rgb, uint8 (n, 3 or 4))."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    n = W * H
    ch = 4 if rgbx else 3
    a = N.DenoiseArgs()
    with B.DeviceArrays() as pool:
        for k, v in (("rgb", rgb), ("normal", guides["normal"]), ("albedo", guides["albedo"]),
                     ("position", guides["position"]), ("depth", guides["depth"])):
            v = np.ascontiguousarray(v, dtype=np.float64)
            d = pool.alloc(v.nbytes)
            N.check(lib, lib.srt_memcpy(ctx, d, N.ptr(v), v.nbytes))
            setattr(a, k, d.value)
        d_out, d_u8 = pool.doubles(3 * n), pool.alloc(ch * n)
        a.levels, a.flags = 0, (N.DENOISE_RGBX if rgbx else 0)
        a.sigma_color, a.sigma_normal, a.sigma_albedo, a.sigma_plane = (DR.DEFAULTS[k] for k in (
            "sigma_color", "sigma_normal", "sigma_albedo", "sigma_plane"))
        a.out_rgb, a.out_srgb8 = d_out.value, d_u8.value
        N.check(lib, lib.srt_denoise(ctx, W, H, ctypes.byref(a)))
        return pool.fetch(d_out, (3, n)), pool.fetch(d_u8, (n, ch), np.uint8)


@pytest.mark.parametrize("pointers", ["host", "device"])
@pytest.mark.parametrize("rgbx", [False, True], ids=["rgb", "rgbx"])
def test_gpu_resolve_pixel_is_the_exact_rule(fr, rgbx, pointers):
    """k_denoise_resolve on the whole frame of tests/resolve_ref.py (width 67): [lo, hi], the unambiguous
    bytes, the special values, no 255 below the cap, alpha 255, and out_rgb the input bit for bit."""
    W, H = fr["W"], fr["H"]
    n = W * H
    if pointers == "host":
        out, u8 = _backend().denoise(fr["rgb"], _guides(n), W, H, levels=0, rgbx=rgbx)
        u8 = u8.reshape(n, -1)
    else:
        out, u8 = _denoise_device_pointers(fr["rgb"], _guides(n), W, H, rgbx)
    assert np.array_equal(out.view(np.uint64), fr["rgb"].view(np.uint64))
    if rgbx:
        assert u8.shape == (n, 4) and np.all(u8[:, 3] == 255)
    u8 = u8[:, :3]
    band = R.check_bytes(u8, fr["lo"], fr["hi"], "k_denoise_resolve")
    assert np.array_equal(u8[fr["special"]], fr["special_bytes"])
    assert u8[R.never_255(fr["rgb"])].max() == 254
    amb = fr["lo"] != fr["hi"]
    print("k_denoise_resolve (%s, %s): %d values, %d ambiguous, %d with u8 != lo, %d with u8 != floor(exact q)" % (
        pointers, "rgbx" if rgbx else "rgb", u8.size, amb.sum(), band, (u8.astype(np.int64) != fr["floor"]).sum()))


@pytest.mark.parametrize("rgbx", [False, True], ids=["rgb", "rgbx"])
def test_gpu_dn_finish_bytes_are_the_rule_on_its_own_rgb(rgbx):
    """k_dn_finish (srt_denoise_var, demodulate, levels 0, equal halves, a noisy albedo): the image against the
    out_rgb the same kernel returned."""
    W, H = 67, 31
    n = W * H
    _, guides, bg = DR.random_frame(W, H, 41)
    half = np.ascontiguousarray(R.random_pixels()[:, :n])
    out, _, u8 = _backend().denoise_var(half, half, 2, 2, guides, W, H, demodulate=True, levels=0, rgbx=rgbx)
    np.testing.assert_allclose(out, half, rtol=1e-14, atol=0.0)  # (c / d * d)
    assert not np.array_equal(out, half) and np.array_equal(out[:, bg], half[:, bg])
    u8 = u8.reshape(n, -1)
    if rgbx:
        assert np.all(u8[:, 3] == 255)
    lo, hi = R.bounds(out)
    assert np.array_equal(lo, hi)
    R.check_bytes(u8[:, :3], lo, hi, "k_dn_finish")


# ---- 2. the stores -----------------------------------------------------------------------------------------------
_CASES = {}


def _case(W, H, spp):
    """example1 at depth 3 with draw_jitter's jitter from numpy seed 1, and the oracle's frame on it."""
    key = (W, H, spp)
    if key not in _CASES:
        sc = scenes.example1(W, H, 3)
        np.random.seed(1)
        jit = sc.camera.draw_jitter(spp)
        _CASES[key] = (sc, jit, O.render_linear(sc, jit))
    return _CASES[key]


def _render(sc, jit, **kw):
    return _backend().render_scene(sc, jit.shape[0], jitter=jit, seed=1, **kw)


def _check_against_oracle(out, ref, pixels=None):
    rgb, ids, counts = ref
    if pixels is not None:
        rgb, ids = rgb[:, pixels], ids[:, pixels]
    assert np.array_equal(out.hit_ids, ids)
    if pixels is None:
        assert out.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    np.testing.assert_allclose(out.rgb, rgb, rtol=RTOL, atol=ATOL)


TOTALS = {"values": 0, "ambiguous": 0, "band": 0}


def _check_bytes_on_own_rgb(out, what):
    """out.srgb8 (3-byte or RGBX) against bounds(out.rgb): no rendered value is ambiguous (~1e-12 per value at
    EPS: a count here is a bug of the test), so every byte is pinned."""
    lo, hi = R.bounds(out.rgb)
    assert np.array_equal(lo, hi), what
    u8 = out.srgb8.reshape(lo.shape[0], -1)
    if u8.shape[1] == 4:
        assert np.all(u8[:, 3] == 255), what
    TOTALS["band"] += R.check_bytes(u8[:, :3], lo, hi, what)
    TOTALS["values"] += lo.size
    TOTALS["ambiguous"] += int((lo != hi).sum())


FUSED_SHAPES = [(1, 1), (7, 5), (12, 9), (67, 13), (13, 67), (129, 3)]
# rt_kernels.hip pix_groups(): `while (g * 2 <= std::min(ns, 64) && npix * g < want) g *= 2;`, then for the fused
# paths `if (fused && g < 2 && ns % 2 == 0) g = 2;` and `g = std::min(g, 8);` -- on these frames, far below
# `want` pixels, g is the largest power of two <= spp, at most 8.  rt_primary_body.inc: a wave's tile is 8 x th
# pixels, th = (64 / g) >> 3, and group k takes the samples [k spg, (k + 1) spg) below spp, spg = ceil(spp / g):
#   spp     1  2  3  4  5  8  9
#   groups  1  2  2  4  4  8  8
#   th      8  4  4  2  2  1  1
#   empty   0  0  0  0  1  0  3     (5 spp: 2, 2, 1, 0;  9 spp: 2, 2, 2, 2, 1, 0, 0, 0)
FUSED_SPP = [1, 2, 3, 4, 5, 8, 9]


@pytest.mark.parametrize("spp", FUSED_SPP)
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: "%dx%d" % s)
def test_gpu_fused_tiles_store_every_byte(shape, spp):
    """k_primary's fused resolve through store_u8_tile at every tile height, on frames whose tile rows are
    whole and cut, aligned and unaligned (W mod 4 = 1, 3, 0, 3, 1, 1)."""
    W, H = shape
    sc, jit, ref = _case(W, H, spp)
    with _options(fuse_primary=1):
        out = _render(sc, jit, want_hits=True)
    assert out.stats["kernel_path"] == "fused" and out.stats["passes"] == 1
    _check_against_oracle(out, ref)
    _check_bytes_on_own_rgb(out, "fused %dx%d %d spp" % (W, H, spp))


@pytest.mark.parametrize("spp", [2, 5, 9])
@pytest.mark.parametrize("shape", [(7, 5), (67, 13), (13, 67)], ids=lambda s: "%dx%d" % s)
def test_gpu_lean_fused_kernel_stores_the_same_bytes(shape, spp):
    W, H = shape
    sc, jit, ref = _case(W, H, spp)
    with _options(fuse_primary=1):
        plain = _render(sc, jit, want_hits=True)
    with _options(fuse_primary=1, sync_lean=1):
        lean = _render(sc, jit, want_hits=True)
    assert lean.stats["kernel_path"] == "fused" and plain.stats["kernel_path"] == "fused"
    _check_against_oracle(lean, ref)
    _check_bytes_on_own_rgb(lean, "lean %dx%d %d spp" % (W, H, spp))
    assert np.array_equal(lean.srgb8, plain.srgb8) and np.array_equal(lean.rgb, plain.rgb)


@pytest.mark.parametrize("mode", ["fused", "wavefront"])
@pytest.mark.parametrize("shape", [(67, 13), (13, 67)], ids=lambda s: "%dx%d" % s)
def test_gpu_several_passes_resolve_in_k_resolve(shape, mode):
    """5 spp in passes of 2: the trace kernels leave the frame in the framebuffer, k_resolve stores it through
    store_u8_chunk, whose last chunk of these 871 pixels holds 39 (n % 4 != 0: the byte path)."""
    W, H = shape
    sc, jit, ref = _case(W, H, 5)
    with _options(fuse_primary=1 if mode == "fused" else 0, frame_kernel=0):
        out = _render(sc, jit, want_hits=True, batch_size=2)
    assert out.stats["kernel_path"] == mode and out.stats["passes"] == 3
    _check_against_oracle(out, ref)
    _check_bytes_on_own_rgb(out, "%s, 3 passes, %dx%d" % (mode, W, H))


def _mode_options(mode):
    return dict(fuse_primary=1 if mode == "fused" else 0, frame_kernel=0)


@pytest.mark.parametrize("mode", ["fused", "wavefront"])
@pytest.mark.parametrize("spp", [2, 5])
def test_gpu_row_shard_bytes_are_the_frames_rows(spp, mode):
    W, H = 67, 13
    rows = np.array([1, 4, 5, 12], dtype=np.int32)
    sc, jit, ref = _case(W, H, spp)
    pixels = (rows[:, None] * W + np.arange(W)[None, :]).reshape(-1)
    with _options(**_mode_options(mode)):
        full = _render(sc, jit)
        shard = _render(sc, np.ascontiguousarray(jit[:, :, pixels]), rows=rows, want_hits=True)
    assert full.stats["kernel_path"] == mode and shard.stats["kernel_path"] == mode
    _check_against_oracle(shard, ref, pixels)
    _check_bytes_on_own_rgb(shard, "%s rows %s" % (mode, rows.tolist()))
    assert shard.srgb8.shape == (4, W, 3) and np.array_equal(shard.srgb8, full.srgb8[rows])
    assert np.array_equal(shard.rgb, full.rgb[:, pixels])


@pytest.mark.parametrize("mode", ["fused", "wavefront"])
@pytest.mark.parametrize("shape,spp", [((67, 13), 2), ((13, 67), 9), ((12, 9), 5)], ids=lambda v: str(v).replace(" ", ""))
def test_gpu_rgb_local_and_rgbx_give_the_same_bytes(shape, spp, mode):
    """want_rgb=False (SRT_RENDER_RGB_LOCAL: the linear RGB stays in HBM) and SRT_RENDER_RGBX (k_rgbx over the
    3-byte image): the bytes of the plain frame, alpha 255."""
    W, H = shape
    sc, jit, ref = _case(W, H, spp)
    with _options(**_mode_options(mode)):
        plain = _render(sc, jit, want_hits=True)
        local = _render(sc, jit, want_rgb=False)
        rgbx = _render(sc, jit, rgbx=True)
        both = _render(sc, jit, want_rgb=False, rgbx=True)
    assert plain.stats["kernel_path"] == mode
    _check_against_oracle(plain, ref)
    _check_bytes_on_own_rgb(plain, "%s %dx%d %d spp" % (mode, W, H, spp))
    _check_bytes_on_own_rgb(rgbx, "%s rgbx %dx%d %d spp" % (mode, W, H, spp))
    assert local.rgb is None and np.array_equal(local.srgb8, plain.srgb8)
    assert rgbx.srgb8.shape == (H, W, 4) and np.array_equal(rgbx.srgb8[..., :3], plain.srgb8)
    assert np.array_equal(rgbx.rgb, plain.rgb) and np.array_equal(both.srgb8, rgbx.srgb8)


@pytest.mark.parametrize("spp", [1, 2, 4])
def test_gpu_mesh_fused_chunks_store_every_byte(tmp_path, spp):
    """The fused BVH variant stores ppw = 64, 32, 16 consecutive pixels per wave through store_u8_chunk
    (pix_groups(): a BVH scene takes one sample per lane up to 4 groups); 13 x 9 = 117 pixels leave a last chunk
    of 53 (odd), 21 (odd) and 5."""
    path = str(tmp_path / "ico1.obj")
    scenes.write_icosphere_obj(path, subdiv=1)
    sc = scenes.mesh_scene(path, 13, 9, 3)
    np.random.seed(1)
    jit = sc.camera.draw_jitter(spp)
    with _options(fuse_primary=1):
        out = _render(sc, jit, want_hits=True)
    assert out.stats["kernel_path"] == "fused"
    _check_against_oracle(out, O.render_linear(sc, jit))
    _check_bytes_on_own_rgb(out, "mesh fused %d spp" % spp)
    assert len(np.unique(out.hit_ids)) > 3  # (the mesh is in the picture)


GUARD = 64


@pytest.mark.parametrize("mode", ["fused", "wavefront"])
@pytest.mark.parametrize("shape", [(12, 9), (67, 13)], ids=lambda s: "%dx%d" % s)
def test_gpu_unaligned_device_image_and_its_guard_bytes(shape, mode):
    """A 3-byte device out_srgb8 at k = 0 .. 3 bytes past a 4-byte boundary, between guard bytes: the image of
    the host-output frame, and not one guard byte touched (the dword paths of store_u8_tile / store_u8_chunk
    must fall back to bytes by the address, not by the pixel index)."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    W, H = shape
    npix = W * H
    sc, jit, ref = _case(W, H, 2)
    jd = np.ascontiguousarray(jit)
    size = GUARD + 3 * npix + 4 + GUARD
    with _options(**_mode_options(mode)):
        want = _render(sc, jit)
        assert want.stats["kernel_path"] == mode
        _check_bytes_on_own_rgb(want, "%s %dx%d" % (mode, W, H))
        B.upload(sc)
        cd = B.camera_desc(sc.camera)
        with B.DeviceArrays() as pool:
            d = pool.alloc(size)
            assert d.value % 4 == 0
            for k in range(4):
                fill = np.full(size, 0xA5, dtype=np.uint8)
                N.check(lib, lib.srt_memcpy(ctx, d, N.ptr(fill), size))
                a = N.RenderArgs()
                a.spp, a.sample_base, a.n_rows, a.batch_spp = 2, 0, H, 0
                a.rows, a.out_hit_id, a.mt, a.seed = None, None, None, 1
                a.jitter = N.ptr(jd)
                a.out_rgb, a.out_srgb8 = None, d.value + GUARD + k
                a.flags = 0
                st = N.Stats()
                N.check(lib, lib.srt_render(ctx, ctypes.byref(cd), ctypes.byref(a), ctypes.byref(st)))
                assert st.as_dict()["kernel_path"] == mode
                got = pool.fetch(d, (size,), np.uint8)
                img = got[GUARD + k:GUARD + k + 3 * npix]
                assert np.array_equal(img.reshape(H, W, 3), want.srgb8), "offset %d" % k
                assert np.all(got[:GUARD + k] == 0xA5) and np.all(got[GUARD + k + 3 * npix:] == 0xA5), "offset %d" % k


def test_gpu_rendered_frames_have_no_ambiguous_value():
    """(Last in the file: the sum over the frames classified above, for the record.)"""
    print("rendered frames: %(values)d values classified, %(ambiguous)d ambiguous, %(band)d with u8 != lo" % TOTALS)
    assert TOTALS["ambiguous"] == 0 and TOTALS["band"] == 0
