"""Smooth-shaded, textured triangle meshes on the device: the MAT_VATTR kernel variants (BVH and
linear triangle loop; per-depth, frame, fused and pipelined paths), the forced-shade kernels behind
_hybrid, srt_collider_surface and srt_trace, against the oracle with the interpolation of
tests/vattr_ref.py.  64x48 frames; hit ids exact, linear RGB within 1e-5 relative."""
import ctypes
import os

import numpy as np
import pytest

import sightpy_oracle as O
import vattr_ref as VR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-12
W, H, SPP = 64, 48, 2


def _backend():
    from sightpy import _backend

    return _backend


def _set_option(key, value):
    lib, ctx = _backend().context()
    rc = lib.srt_set_option(ctx, key.encode(), ctypes.c_int64(value))
    assert rc == 0, lib.srt_last_error()


@pytest.fixture(scope="module")
def ico1(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vattr") / "ico1.obj")
    VR.write_smooth_icosphere_obj(p, 1)
    return p


@pytest.fixture(scope="module")
def tetra(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vattr") / "tetra.obj")
    VR.write_tetrahedron_obj(p, radius=0.7)
    return p


def _jitter(sc, seed=5, spp=SPP):
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


def _async_frames(sc, jit, frames=2):
    """`frames` pipelined SRT_RENDER_ASYNC frames of the uploaded scene into device buffers; the last"""
    from sightpy import _native as N

    B = _backend()
    lib, ctx = B.context()
    npix = W * H
    dj = B.device_buffer("vattr_jit", jit.nbytes)
    N.check(lib, lib.srt_memcpy(ctx, dj, N.ptr(jit), jit.nbytes))
    drgb = B.device_buffer("vattr_rgb", 3 * npix * 8)
    du8 = B.device_buffer("vattr_u8", 3 * npix)
    a = N.RenderArgs()
    a.spp, a.sample_base, a.n_rows, a.batch_spp = SPP, 0, H, 0
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


# ---- 6. kernel paths --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths(ico1):
    """The smooth 80-face mesh (BVH) through every kernel path, rendered once: the patched oracle's frame,
    the per-depth kernels, the frame kernel (BVH on and off), the fused path, the linear triangle loop
    (bvh=0), two pipelined asynchronous frames; and the flat mesh through the per-depth and the frame
    kernels."""
    sc = VR.mesh_scene(ico1, W, H, 3, smooth=True)
    jit = _jitter(sc)
    with pytest.MonkeyPatch.context() as mp:
        VR.patch(mp)
        ref = O.render_linear(sc, jit)
    out = {"ref": ref,
           "depth": _render(sc, jit, frame_kernel=0, fuse_primary=0),
           "frame": _render(sc, jit, frame_kernel=1, fuse_primary=0),
           "frame,bvh=0": _render(sc, jit, frame_kernel=1, fuse_primary=0, bvh=0),
           "fused": _render(sc, jit, frame_kernel=0, fuse_primary=1),
           "bvh=0": _render(sc, jit, frame_kernel=0, fuse_primary=0, bvh=0),
           "async": _async_frames(sc, jit)}
    flat = VR.mesh_scene(ico1, W, H, 3, smooth=False)
    out["flat depth"] = _render(flat, jit, frame_kernel=0, fuse_primary=0)
    out["flat frame"] = _render(flat, jit, frame_kernel=1, fuse_primary=0)
    return out


def test_gpu_smooth_mesh_every_kernel_path(paths):
    """Per-depth kernels against the patched oracle; the fused single-child path (the glossy mesh variant
    has one), the linear triangle loop (bvh=0) and two pipelined asynchronous frames bit-identical to
    them; the frame kernel against the oracle, and bit-identical with the BVH on and off."""
    ref, ids, counts = paths["ref"]
    depth = paths["depth"]
    for name in ("depth", "frame"):
        out = paths[name]
        assert np.array_equal(out.hit_ids, ids), name
        assert out.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])], name
        np.testing.assert_allclose(out.rgb, ref, rtol=RTOL, atol=ATOL, err_msg=name)
    assert paths["fused"].stats["kernel_path"] == "fused" and paths["frame"].stats["kernel_path"] == "frame"
    for name in ("fused", "bvh=0"):
        out = paths[name]
        assert np.array_equal(out.hit_ids, ids), name
        assert np.array_equal(out.rgb, depth.rgb) and np.array_equal(out.srgb8, depth.srgb8), name
    a, b = paths["frame"], paths["frame,bvh=0"]
    assert np.array_equal(a.hit_ids, b.hit_ids) and np.array_equal(a.rgb, b.rgb) and np.array_equal(a.srgb8, b.srgb8)
    rgb, u8, st = paths["async"]
    assert st["total_rays"] == depth.stats["total_rays"]
    assert np.array_equal(rgb, depth.rgb) and np.array_equal(u8, depth.srgb8)
    assert not np.allclose(paths["flat depth"].rgb, depth.rgb, rtol=1e-3, atol=1e-6)  # smooth is not flat


def test_gpu_smooth_mesh_frame_kernel_bit_identical_to_per_depth_kernels(paths):
    """All kernel paths bit-identical to one another includes the frame kernel against the per-depth
    kernels: the frame kernel's variants for per-vertex attributes sum a tile's colours in fixed point
    like the per-depth and fused kernels (terms of 2^-44 added as integers, in any order the same bits).
    The flat mesh's frame kernel keeps its float64 sums in LDS and agrees to rounding only (measured
    on an MI355X, 64x48, depth 3, 2 spp: 1.18e-11 relative; before the smooth variants summed in fixed
    point they differed by 8.05e-12)."""
    def worst(a, b):
        nz = b != 0.0
        return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()), int((a != b).sum())

    for kind, f, d in (("smooth", paths["frame"], paths["depth"]), ("flat", paths["flat frame"], paths["flat depth"])):
        print("%s mesh, frame kernel against per-depth kernels: max relative difference %.3e, %d of %d values differ, "
              "uint8 images equal: %s" % ((kind,) + worst(f.rgb, d.rgb) + (d.rgb.size, np.array_equal(f.srgb8, d.srgb8))))
    assert np.array_equal(paths["frame"].rgb, paths["depth"].rgb)
    assert np.array_equal(paths["frame"].srgb8, paths["depth"].srgb8)


def test_gpu_smooth_mesh_frame_kernel_leaves_fixed_point_range_and_falls_back(ico1):
    """A term beyond the fixed-point range (2^17) in the frame kernel's fixed-point sums: the frame is
    rendered again with float64 sums, as on the other paths, and agrees with the per-depth kernels'
    float64 frame to rounding (sums of up to a few terms of 1e7: 1e-9 relative is far above their
    last bits and far below a lost term)."""
    from sightpy import Emissive, Sphere, rgb, vec3

    lamp = Sphere(material=Emissive(color=rgb(1e7, 1e7, 1e7)), center=vec3(0.0, 60.0, -3.0), radius=55.0, shadow=False,
                  max_ray_depth=3)
    sc = VR.mesh_scene(ico1, W, H, 3, smooth=True, extra=lamp)
    jit = _jitter(sc)
    frame = _render(sc, jit, frame_kernel=1, fuse_primary=0)
    assert frame.stats["kernel_path"] == "frame" and frame.stats["retries"] >= 1
    depth = _render(sc, jit, frame_kernel=0, fuse_primary=0)
    assert np.array_equal(frame.hit_ids, depth.hit_ids)
    np.testing.assert_allclose(frame.rgb, depth.rgb, rtol=1e-9, atol=ATOL)
    assert frame.rgb.max() > 1e6


# ---- 7. linear path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("frame_kernel", [0, 1])
def test_gpu_smooth_tetrahedron_linear_triangle_loop(tetra, frame_kernel, monkeypatch):
    """Four triangles: below the BVH threshold, intersected one by one (MAT_TRI)."""
    VR.patch(monkeypatch)
    sc = VR.mesh_scene(tetra, W, H, 3, smooth=True)
    jit = _jitter(sc)
    out = _render(sc, jit, frame_kernel=frame_kernel)
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(out.hit_ids, ids)
    assert out.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    np.testing.assert_allclose(out.rgb, ref, rtol=RTOL, atol=ATOL)


# ---- 8. refractive mesh ---------------------------------------------------------------------------------
def test_gpu_smooth_refractive_mesh_frame_kernel(ico1, monkeypatch):
    """A glass mesh at depth 4 through k_frame: the reflected and refracted children take their
    directions from the interpolated normal.  (One sample per pixel: the oracle's recursion over two
    children per hit is most of this test's time.)"""
    from sightpy import Refractive, vec3

    VR.patch(monkeypatch)
    glass = Refractive(n=vec3(1.5 + 4e-8j, 1.5 + 0.0j, 1.5 + 4e-8j))
    sc = VR.mesh_scene(ico1, W, H, 4, smooth=True, material=glass)
    jit = _jitter(sc, 7, spp=1)
    out = _render(sc, jit, frame_kernel=1)
    assert out.stats["kernel_path"] == "frame"
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(out.hit_ids, ids)
    assert out.stats["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    np.testing.assert_allclose(out.rgb, ref, rtol=RTOL, atol=ATOL)
    depth = _render(sc, jit, frame_kernel=0)  # the per-depth kernels: the same bits
    assert depth.stats["kernel_path"] == "wavefront"
    nz = depth.rgb != 0.0
    print("glass mesh, frame kernel against per-depth kernels: retries %d / %d, max relative difference %.3e, %d values differ"
          % (out.stats["retries"], depth.stats["retries"],
             (np.abs(out.rgb[nz] - depth.rgb[nz]) / np.abs(depth.rgb[nz])).max(), (out.rgb != depth.rgb).sum()))
    assert np.array_equal(out.rgb, depth.rgb) and np.array_equal(out.srgb8, depth.srgb8)


# ---- 9. textured mesh -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["ico1", "tetra"])
def test_gpu_textured_mesh(mesh, ico1, tetra, monkeypatch):
    """texcoords=True with the checkered image (repeat 4) over the vertices' spherical coordinates;
    pixels whose primary hit lies within 8 ulp of a texel boundary may be left out, at most 0.5 %
    (measured on the CPU: none of the 3072 in either scene)."""
    VR.patch(monkeypatch)
    sc = VR.mesh_scene(ico1 if mesh == "ico1" else tetra, W, H, 3, smooth=True, texcoords=True, material=VR.checker())
    jit = _jitter(sc)
    skip = VR.texel_boundary_pixels(sc, jit)
    assert skip.mean() <= 0.005
    out = _render(sc, jit)
    ref, ids, counts = O.render_linear(sc, jit)
    assert np.array_equal(out.hit_ids, ids)
    np.testing.assert_allclose(out.rgb[:, ~skip], ref[:, ~skip], rtol=RTOL, atol=ATOL)
    np.random.seed(3)
    img = np.asarray(sc.render(SPP))  # the public entry point
    assert img.shape == (H, W, 3)


# ---- 10. surface and trace entry points -----------------------------------------------------------------
def test_gpu_collider_surface_and_get_normal_of_flagged_triangles(ico1):
    """srt_collider_surface at 256 points of a flagged triangle: the interpolation (every operation is
    a correctly rounded float64 one in the same order; 1e-14 leaves room for a last-bit difference in
    the square root, the reciprocal and the divisions); an unflagged triangle's uv stays an error."""
    from sightpy import _native as N
    from sightpy.ray import Hit
    from sightpy import vec3

    B = _backend()
    rng = np.random.default_rng(3)
    sc = VR.mesh_scene(ico1, smooth=True, texcoords=True, material=VR.checker())
    for c in VR.mesh_colliders(sc)[::27]:
        w = rng.dirichlet([1.0, 1.0, 1.0], size=256).T
        w[:, :3] = np.eye(3)
        P = O.col3(c.p1) * w[0] + O.col3(c.p2) * w[1] + O.col3(c.p3) * w[2]
        Nn, uv = B.collider_surface(c, vec3(*P))
        np.testing.assert_allclose(Nn, VR.interp_normal(c, P), rtol=1e-14, atol=1e-16)
        u, v = VR.interp_uv(c, P)
        np.testing.assert_allclose(uv, [u, v], rtol=1e-14, atol=1e-16)
        hit = Hit(1.0, 1.0, c.assigned_primitive.material, c, c.assigned_primitive)
        hit.point = vec3(*P)
        n = c.get_Normal(hit)
        assert np.array_equal([n.x, n.y, n.z], Nn)
        gu, gv = c.get_uv(hit)
        assert np.array_equal([gu, gv], uv)
    flat = VR.mesh_colliders(VR.mesh_scene(ico1, smooth=False))[0]
    with pytest.raises(N.SrtError):
        B.collider_surface(flat, vec3(*np.zeros((3, 4))))
    Nn, _ = B.collider_surface(flat, vec3(*np.zeros((3, 4))), uv=False)
    assert np.array_equal(Nn, np.broadcast_to(O.col3(flat.normal), (3, 4)))


def test_gpu_trace_batch_matches_trace_linear(ico1, monkeypatch):
    """srt_trace of 1,024 rays at the smooth, textured mesh against trace_linear."""
    from sightpy import Ray, vec3
    from sightpy._backend import trace_rays

    VR.patch(monkeypatch)
    sc = VR.mesh_scene(ico1, smooth=True, texcoords=True, material=VR.checker())
    rng = np.random.default_rng(17)
    n = 1024
    Oa = rng.uniform(-1.5, 1.5, size=(3, n)) + np.array([[0.35], [1.0], [0.8]])
    tgt = np.array([[0.35], [0.05], [-1.0]]) + rng.normal(scale=0.35, size=(3, n))
    Da = tgt - Oa
    Da /= np.sqrt((Da * Da).sum(0))
    col, st = trace_rays(Ray(vec3(*Oa), vec3(*Da), 0, sc.n, 0, 0, 0), sc, seed=3, return_stats=True)
    ref, counts = O.trace_linear(sc, Oa, Da, O.scene_medium(sc), 0)
    assert st["rays_per_depth"] == [counts["depth"][d] for d in sorted(counts["depth"])]
    np.testing.assert_allclose(np.stack([col.x, col.y, col.z]), ref, rtol=RTOL, atol=ATOL)
    _, ids = O.hit_ids(sc, Oa, Da)
    mesh = np.isin(ids, [i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Triangle_Collider"])
    assert mesh.mean() > 0.3


# ---- 11. hybrid path ------------------------------------------------------------------------------------
def test_gpu_hybrid_scene_with_smooth_mesh_and_user_material(ico1, monkeypatch):
    """The smooth mesh beside a sphere with a user Material: built-in hits shaded one level at a time
    (srt_shade_level's forced-shade kernels with MAT_VATTR), the user's get_color on the host,
    against the reference recursion with the patched oracle."""
    import hybrid_ref
    import user_classes as U
    from sightpy import Sphere, rgb, vec3, _hybrid
    from sightpy.ray import get_raycolor

    VR.patch(monkeypatch)
    ball = Sphere(material=U.Tinted(rgb(0.2, 0.4, 0.9), 0.5), center=vec3(0.9, -0.1, -0.4), radius=0.3, max_ray_depth=3)
    sc = VR.mesh_scene(ico1, W, H, 3, smooth=True, extra=ball)
    assert _hybrid.is_hybrid(sc)
    np.random.seed(11)
    state = np.random.get_state()
    jit = sc.camera.draw_jitter(1)
    monkeypatch.setitem(U.TRACE, "fn", hybrid_ref.trace)
    ref = hybrid_ref.render_linear(sc, jit)
    monkeypatch.setitem(U.TRACE, "fn", get_raycolor)
    np.random.set_state(state)
    lin = _hybrid.render_linear(sc, 1)
    got = np.array([np.broadcast_to(np.asarray(c, dtype=np.float64), (W * H,)) for c in (lin.x, lin.y, lin.z)])
    nz = ref != 0.0
    assert np.all(got[~nz] == 0.0)
    rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
    assert rel.max() <= 1e-5, rel.max()


# ---- several GPUs: the sharded path uploads the same tables ---------------------------------------------
def test_gpu_group_render_of_smooth_textured_mesh(ico1):
    """Scene.render's group path (srt_render_group over $SIGHTPY_DEVICES: row bands, RCCL gather)
    gives the single-context frame."""
    B = _backend()
    sc = VR.mesh_scene(ico1, W, H, 3, smooth=True, texcoords=True, material=VR.checker())
    np.random.seed(9)
    ref = B.render_scene(sc, SPP, seed=3, mt=True)
    np.random.seed(9)
    old = os.environ.get("SIGHTPY_DEVICES")
    os.environ["SIGHTPY_DEVICES"] = str(B.devices()[0])
    try:
        got = B.render_group(sc, SPP, seed=3, mt=True)
    finally:
        if old is None:
            os.environ.pop("SIGHTPY_DEVICES")
        else:
            os.environ["SIGHTPY_DEVICES"] = old
    np.testing.assert_allclose(got.rgb, ref.rgb, rtol=1e-12, atol=1e-12)
    assert np.abs(got.srgb8.astype(int) - ref.srgb8.astype(int)).max() <= 1
    assert got.stats["total_rays"] == ref.stats["total_rays"]
