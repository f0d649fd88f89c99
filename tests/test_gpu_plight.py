"""PositionalLight / SpotLight on the device: the MAT_PLIGHT kernel variants (per-depth, fused and
pipelined paths; BVH and linear triangle loop), the forced-shade kernels behind _hybrid, and a light
moved between two renders, against the oracle with the restatement of tests/plight_ref.py.  Hit ids
exact, linear RGB within 1e-5 relative, uint8 exact where two device paths are compared; no pixel is
left out of a comparison."""
import ctypes

import numpy as np
import pytest

import plight_ref as PR
import sightpy_oracle as O

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-12


def _backend():
    from sightpy import _backend

    return _backend


def _set_option(key, value):
    lib, ctx = _backend().context()
    rc = lib.srt_set_option(ctx, key.encode(), ctypes.c_int64(value))
    assert rc == 0, lib.srt_last_error()


def _jitter(sc, spp, seed=5):
    np.random.seed(seed)
    return np.ascontiguousarray(sc.camera.draw_jitter(spp))


def _render(sc, jit, **options):
    """One frame under library options (reset afterwards).  "bvh" acts when a scene is uploaded, and an
    unchanged scene is not uploaded again: force it, and once more when the option is back."""
    for k, v in options.items():
        _set_option(k, v)
    try:
        if "bvh" in options:
            _backend().upload(sc, force=True)
        return _backend().render_scene(sc, jit.shape[0], jitter=jit, seed=1, want_hits=True)
    finally:
        for k in options:
            _set_option(k, 1 if k == "bvh" else -1)
        if "bvh" in options:
            _backend().upload(sc, force=True)


def _against_oracle(sc, jit, out):
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(out.hit_ids, ids)
    assert out.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    assert out.stats["shadow_rays"] == counts["shadow"]  # one shadow test per light per Glossy hit
    np.testing.assert_allclose(out.rgb, ref, rtol=RTOL, atol=ATOL)


@pytest.fixture(scope="module")
def split_tetra(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("plight") / "split_tetra.obj")
    assert PR.write_split_tetrahedron_obj(p) == 12
    return p


# ---- 1. the scenes of test_plight.py on the device ----------------------------------------------------
@pytest.mark.parametrize("name, spp", [("room", 2), ("spot", 2), ("many_lights", 1)])
def test_gpu_scene_against_restatement(name, spp, monkeypatch):
    """The room under a positional light (lit, shadowed, occluders beyond the light; a rotated cuboid
    among the shadow casters), under a spot light whose cone edge crosses the floor, and with the
    positional light at index 32 behind 32 directional ones."""
    PR.patch(monkeypatch)
    sc = {"room": lambda: PR.room(48, 36, 3), "spot": lambda: PR.spot_room(48, 36, 3),
          "many_lights": lambda: PR.many_lights_room(16, 12, 3)}[name]()
    jit = _jitter(sc, spp)
    _against_oracle(sc, jit, _render(sc, jit))
    if name == "room":
        np.random.seed(3)
        img = np.asarray(sc.render(spp))  # the public entry point
        assert img.shape == (36, 48, 3)


def test_gpu_light_just_above_the_floor_leaves_the_fixed_point_range(monkeypatch):
    """Irradiance 100 / 0.02**2 > 2**17: the frame is rendered again with float64 sums (the existing
    retry) and equals the restatement."""
    PR.patch(monkeypatch)
    sc = PR.near_floor_room(_jitter(PR.room(16, 12, 3), 1), 16, 12, 3)
    jit = _jitter(sc, 1)
    out = _render(sc, jit)
    assert out.stats["retries"] >= 1
    _against_oracle(sc, jit, out)
    assert out.rgb.sum(axis=0).max() >= 2.0 ** 17


# ---- 2. fused, per-depth and pipelined paths of the Glossy + sky variant --------------------------------
def _async_frames(sc, jit, W, H, frames=2):
    """`frames` pipelined SRT_RENDER_ASYNC frames of the scene into device buffers; the last one's
    linear RGB, uint8 image and stats."""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    npix = W * H
    dj = B.device_buffer("plight_jit", jit.nbytes)
    N.check(lib, lib.srt_memcpy(ctx, dj, N.ptr(jit), jit.nbytes))
    drgb = B.device_buffer("plight_rgb", 3 * npix * 8)
    du8 = B.device_buffer("plight_u8", 3 * npix)
    a = N.RenderArgs()
    a.spp, a.sample_base, a.n_rows, a.batch_spp = jit.shape[0], 0, H, 0
    a.jitter, a.seed, a.out_rgb, a.out_srgb8, a.out_hit_id = dj, 1, drgb, du8, None
    a.flags = N.RENDER_ASYNC
    cd = B.camera_desc(sc.camera)
    st = N.Stats()
    B.upload(sc)
    for _ in range(frames):
        N.check(lib, lib.srt_render(ctx, ctypes.byref(cd), ctypes.byref(a), None))
    N.check(lib, lib.srt_render_finish(ctx, ctypes.byref(st)))
    rgb = np.empty((3, npix))
    u8 = np.empty((npix, 3), dtype=np.uint8)
    N.check(lib, lib.srt_memcpy(ctx, N.ptr(rgb), drgb, rgb.nbytes))
    N.check(lib, lib.srt_memcpy(ctx, N.ptr(u8), du8, u8.nbytes))
    return rgb, u8.reshape(H, W, 3), st.as_dict()


def test_gpu_fused_per_depth_and_pipelined_paths_agree(monkeypatch):
    """The room (Glossy surfaces and the sky box: the MATS_GLOSSY_SKY | MAT_PLIGHT variant) at 160x120,
    depth 5, 1 spp: the fused single-child path forced on and off give the same bits, and so do two
    pipelined asynchronous frames; the per-depth frame equals the restatement."""
    PR.patch(monkeypatch)
    W, H = 160, 120
    sc = PR.room(W, H, 5)
    jit = _jitter(sc, 1)
    depth = _render(sc, jit, fuse_primary=0)
    fused = _render(sc, jit, fuse_primary=1)
    assert fused.stats["kernel_path"] == "fused" and depth.stats["kernel_path"] == "wavefront"
    _against_oracle(sc, jit, depth)
    assert np.array_equal(fused.hit_ids, depth.hit_ids)
    assert np.array_equal(fused.rgb, depth.rgb) and np.array_equal(fused.srgb8, depth.srgb8)
    assert fused.stats["shadow_rays"] == depth.stats["shadow_rays"]
    rgb, u8, st = _async_frames(sc, jit, W, H)
    assert st["total_rays"] == depth.stats["total_rays"]
    assert np.array_equal(rgb, depth.rgb) and np.array_equal(u8, depth.srgb8)


# ---- 3. the mesh through the BVH and through the linear triangle loop -----------------------------------
def test_gpu_mesh_shadows_the_floor_with_and_without_the_bvh(split_tetra, monkeypatch):
    PR.patch(monkeypatch)
    sc = PR.mesh_room(split_tetra, 48, 36, 3)
    jit = _jitter(sc, 2)
    with_bvh = _render(sc, jit, bvh=1)
    linear = _render(sc, jit, bvh=0)
    _against_oracle(sc, jit, with_bvh)
    _against_oracle(sc, jit, linear)
    assert np.array_equal(with_bvh.hit_ids, linear.hit_ids)
    assert np.array_equal(with_bvh.rgb, linear.rgb) and np.array_equal(with_bvh.srgb8, linear.srgb8)


# ---- 4. hybrid: a user material beside built-in Glossy surfaces ---------------------------------------
def test_gpu_hybrid_scene_with_user_material_under_a_positional_light(monkeypatch):
    """A Tinted sphere (tests/user_classes.py) above the Glossy floor: the built-in hits are shaded on
    the device one level at a time (srt_shade_level's forced-shade kernels with MAT_PLIGHT), the user's
    get_color on the host, through Scene.render's own path, against the reference recursion with the
    patched oracle."""
    import hybrid_ref
    import user_classes as U
    from sightpy import _hybrid
    from sightpy.ray import get_raycolor

    PR.patch(monkeypatch)
    W, H, spp = 48, 36, 2
    sc = PR.tinted_room(W, H, 3)
    assert _hybrid.is_hybrid(sc)
    np.random.seed(11)
    state = np.random.get_state()
    jit = sc.camera.draw_jitter(spp)
    monkeypatch.setitem(U.TRACE, "fn", hybrid_ref.trace)
    ref = hybrid_ref.render_linear(sc, jit)
    monkeypatch.setitem(U.TRACE, "fn", get_raycolor)
    np.random.set_state(state)
    lin = _hybrid.render_linear(sc, spp)  # what Scene.render resolves for a hybrid scene
    got = np.array([np.broadcast_to(np.asarray(c, dtype=np.float64), (W * H,)) for c in (lin.x, lin.y, lin.z)])
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    np.random.set_state(state)
    img = np.asarray(sc.render(spp))
    assert np.array_equal(img, O.srgb_u8(got, H, W))


# ---- 5. a light moved between two renders of one Scene ---------------------------------------------------
def test_gpu_light_moved_between_two_renders_of_one_scene():
    from sightpy import vec3

    sc = PR.room(48, 36, 3)
    jit = _jitter(sc, 2)
    first = _render(sc, jit)
    sc.Light_list[1].pos = vec3(0.3, 0.4, -2.6)
    second = _render(sc, jit)
    assert not np.array_equal(first.rgb, second.rgb)
    for out, pos in ((first, PR.LIGHT_POS), (second, (0.3, 0.4, -2.6))):
        fresh = _render(PR.room(48, 36, 3, pos=pos), jit)
        assert np.array_equal(out.hit_ids, fresh.hit_ids)
        assert np.array_equal(out.rgb, fresh.rgb) and np.array_equal(out.srgb8, fresh.srgb8)
