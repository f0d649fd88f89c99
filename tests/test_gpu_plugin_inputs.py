"""User texture and Light subclasses on the device (reference plugin points textures/texture.py:14-16
and lights.py:12-22, used at glossy.py:30,38-44): a built-in Glossy / Diffuse / Emissive is shaded in
HIP one level at a time from what the user's Python methods returned at each hit
(srt_shade_level_inputs, sightpy/_hybrid.py).  Frames against the reference's own renders of the same
user classes (tests/golden/plugin_*.npz, made by tests/golden/gen_plugin_golden.py), the per-hit path
against the table path bit for bit at the ABI, a user light that restates DirectionalLight against
the whole-device render, the argument checks, and a normal-mapped floor under a user light.
Bars: linear RGB within 1e-5 relative, uint8 within +-1 on fewer than 1 % of the values."""
import ctypes

import numpy as np
import pytest

import plugin_scenes as PS
import scenes
from conftest import golden

pytestmark = pytest.mark.gpu

W, H, DEPTH, SPP, SEED = 48, 36, 3, 2, 11


def _planar3(v, n):
    return np.array([np.broadcast_to(np.asarray(c, dtype=np.float64), (n,)) for c in (v.x, v.y, v.z)])


def _check_frame(lin, img, ref_rgb, ref_u8):
    got = _planar3(lin, ref_rgb.shape[1])
    nz = ref_rgb != 0.0
    assert np.all(got[~nz] == 0.0)
    rel = np.abs(got[nz] - ref_rgb[nz]) / np.abs(ref_rgb[nz])
    print("max relative error", rel.max())
    assert rel.max() <= 1e-5, rel.max()
    d = np.abs(np.asarray(img).astype(int) - ref_u8.astype(int))
    print("u8 max diff", d.max(), "fraction differing", (d > 0).mean())
    assert d.max() <= 1 and (d > 0).mean() < 1e-2


# ---- 1. frames against the reference's renders ------------------------------------------------------
@pytest.mark.parametrize("kind", PS.KINDS)
def test_gpu_plugin_frame_matches_reference(kind):
    from sightpy import _hybrid

    g = golden("plugin_%s_%dx%d_d%d_s%d" % (kind, W, H, DEPTH, SPP))
    assert (int(g["seed"]), int(g["spp"]), int(g["width"]), int(g["height"])) == (SEED, SPP, W, H)
    sc = PS.scene(kind, W, H, DEPTH)
    calls = PS.classes().calls
    for k in calls:
        calls[k] = 0
    np.random.seed(SEED)
    state = np.random.get_state()
    lin = _hybrid.render_linear(sc, SPP)
    np.random.set_state(state)
    img = sc.render(SPP)
    print("user calls", dict(calls))
    if kind in ("texture", "both"):
        assert calls["get_color"] >= 2  # primaries and reflections both ran the user's code
    if kind in ("light", "both"):
        assert calls["get_distance"] >= 2 and calls["get_irradiance"] >= 2
    _check_frame(lin, img, g["rgb"], g["srgb8"])


# ---- 2. the per-hit path equals the table path, at the ABI -------------------------------------------
N_RAYS = 193  # three waves and one lane


def _same_color_classes():
    from sightpy.textures.texture import image, solid_color

    class SameSolid(solid_color):
        def get_color(self, hit):
            return self.color

    class SameImage(image):
        def get_color(self, hit):
            return super().get_color(hit)

    return SameSolid, SameImage


def _identity_scene(case, flagged):
    """example1 with the collider under test (and its material, for 'emissive' / 'diffuse'), its
    texture a user subclass returning the same colour when `flagged`.  -> scene, collider index."""
    from sightpy import Diffuse, Emissive, rgb

    SameSolid, SameImage = _same_color_classes()
    sc = scenes.example1(16, 12, 3)
    ci = 2 if case == "glossy_floor" else 0
    prim = sc.collider_list[ci].assigned_primitive
    if case == "emissive":
        prim.material = Emissive(color=rgb(1.5, 0.7, 0.2))
    elif case == "diffuse":
        prim.material = Diffuse(diff_color=rgb(0.6, 0.3, 0.7), diffuse_rays=5)
    m = prim.material
    attr = "texture_color" if case == "emissive" else "diff_texture"
    if flagged:
        old = getattr(m, attr)
        if case == "glossy_floor":
            new = SameImage.__new__(SameImage)
            new.__dict__.update(old.__dict__)
        else:
            new = SameSolid(old.color)
        setattr(m, attr, new)
    return sc, ci


def _rays_at(sc, case):
    """N_RAYS rays from the camera at points of the gold sphere / of the floor in front of it."""
    rng = np.random.default_rng(4)
    eye = sc.camera.look_from
    O = np.repeat(np.array([[eye.x], [eye.y], [eye.z]], dtype=np.float64), N_RAYS, axis=1)
    if case == "glossy_floor":
        P = np.stack([rng.uniform(-0.5, 0.5, N_RAYS), np.full(N_RAYS, -0.5), rng.uniform(-1.5, -0.5, N_RAYS)])
    else:
        P = np.array([[-0.75], [0.1], [-3.0]]) + rng.uniform(-0.3, 0.3, (3, N_RAYS))
    D = P - O
    D /= np.sqrt((D * D).sum(0))
    return np.ascontiguousarray(O), np.ascontiguousarray(D)


def _level(sc, ids, O, D, t, o, inputs="plain", depth=0, dfl=0, seed=77, cap=None):
    """srt_shade_level (inputs == "plain") or srt_shade_level_inputs (a HitInputs or None = NULL) on
    the uploaded `sc`: (rc, out_rgb, children in a canonical order)."""
    from sightpy import _backend as B, _native as N

    lib, ctx = B.context()
    B.upload(sc)
    n = O.shape[1]
    cap = cap or 8 * n
    local = np.zeros((3, n))
    a = N.TraceArgs()
    a.n = n
    a.origin, a.dir, a.medium = N.ptr(O), N.ptr(D), None
    a.depth, a.diffuse_reflections, a.seed = depth, dfl, seed
    a.out_rgb = N.ptr(local)
    arrs = {"origin": np.zeros((3, cap)), "dir": np.zeros((3, cap)), "weight": np.zeros((3, cap)),
            "parent": np.zeros(cap, np.int32), "medium": np.zeros(cap, np.int32),
            "depth": np.zeros(cap, np.int32), "diffuse_reflections": np.zeros(cap, np.int32)}
    kids = N.Children()
    kids.cap = cap
    for k, v in arrs.items():
        setattr(kids, k, N.ptr(v))
    if isinstance(inputs, str):
        rc = lib.srt_shade_level(ctx, ctypes.byref(a), N.ptr(ids), N.ptr(t), N.ptr(o), ctypes.byref(kids), None)
    else:
        rc = lib.srt_shade_level_inputs(ctx, ctypes.byref(a), N.ptr(ids), N.ptr(t), N.ptr(o),
                                        ctypes.byref(inputs) if inputs is not None else None, ctypes.byref(kids), None)
    if rc != 0:
        return rc, lib.srt_last_error().decode(), None
    nk = int(kids.n)
    # (the queue shards hand the children back in append order: compared in one canonical order)
    rows = np.concatenate([arrs["parent"][None, :nk].astype(np.float64), arrs["depth"][None, :nk],
                           arrs["diffuse_reflections"][None, :nk], arrs["medium"][None, :nk], arrs["origin"][:, :nk],
                           arrs["dir"][:, :nk], arrs["weight"][:, :nk]])
    order = np.lexsort(rows[::-1])
    return 0, local, rows[:, order]


@pytest.mark.parametrize("case", ["glossy_sphere", "glossy_floor", "emissive", "diffuse"])
def test_gpu_hit_albedo_equals_table_path(case):
    from sightpy import Hit, _backend as B, _hybrid, _native as N, vec3

    sc_a, ci = _identity_scene(case, False)
    sc_b, _ = _identity_scene(case, True)
    assert not _hybrid.is_hybrid(sc_a) and _hybrid.is_hybrid(sc_b)
    O, D = _rays_at(sc_a, case)
    t, ids, o = B.nearest_hits(sc_a, vec3(*O), vec3(*D))
    assert (ids == ci).all()
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    rc, rgb_a, kids_a = _level(sc_a, ids, O, D, t, o)
    assert rc == 0, rgb_a
    # the flagged scene: the same tables but the flag and the zeroed table colour
    L = B.upload(sc_b)
    m = L.materials[L.colliders["material"][ci]]
    assert m["flags"] & N.MF_HIT_ALBEDO and m["tex"] == -1 and L.device_index[ci] == ci
    coll = sc_b.collider_list[ci]
    mat = coll.assigned_primitive.material
    hit = Hit(t, o, mat, coll, coll.assigned_primitive)
    hit.point = vec3(*O) + vec3(*D) * t
    albedo = _hybrid._rows(_hybrid.user_texture(mat).get_color(hit), N_RAYS)
    B.upload(sc_b)
    inp = N.HitInputs()
    inp.albedo, inp.n_lights = N.ptr(albedo), 0
    rc, rgb_b, kids_b = _level(sc_b, ids, O, D, t, o, inputs=inp)
    assert rc == 0, rgb_b
    assert np.isfinite(rgb_a).all()
    if case == "diffuse":
        assert kids_a.shape[1] == 5 * N_RAYS and not rgb_a.any()
    elif case == "emissive":
        assert kids_a.shape[1] == 0 and rgb_a.all()
    else:
        assert kids_a.shape[1] == N_RAYS and rgb_a.any()
    assert np.array_equal(rgb_a, rgb_b)
    assert kids_a.shape == kids_b.shape and np.array_equal(kids_a, kids_b)


# ---- 3. a user light that restates DirectionalLight --------------------------------------------------
def _ex1_with_cuboid():
    """example1 plus user_classes.glass_scene's rotated cuboid as a Glossy shadow caster."""
    from sightpy import Cuboid, Glossy, rgb, vec3

    sc = scenes.example1(W, H, DEPTH)
    grey = Glossy(diff_color=rgb(0.6, 0.6, 0.55), n=vec3(1.4 + 0.2j, 1.4 + 0.2j, 1.4 + 0.2j), roughness=0.3,
                  spec_coeff=0.3, diff_coeff=0.8)
    cb = Cuboid(material=grey, center=vec3(0.25, -0.1, -1.8), width=0.5, height=0.8, length=0.4, shadow=True,
                max_ray_depth=DEPTH)
    cb.rotate(θ=30, u=vec3(0, 1, 0))
    sc.add(cb)
    return sc


@pytest.mark.parametrize("build", ["example1", "cuboid"])
def test_gpu_user_light_restating_directional(build):
    from sightpy import _backend as B, _hybrid

    make = (lambda: scenes.example1(W, H, DEPTH)) if build == "example1" else _ex1_with_cuboid
    ref_sc = make()
    np.random.seed(SEED)
    state = np.random.get_state()
    ref = B.render_scene(ref_sc, SPP, mt=True)
    sc = make()
    lt = sc.Light_list[0]
    sc.Light_list[0] = PS.classes().PlainDirectional(lt.Ldir, lt.color)
    assert _hybrid.is_hybrid(sc)
    np.random.set_state(state)
    lin = _hybrid.render_linear(sc, SPP)
    np.random.set_state(state)
    img = sc.render(SPP)
    _check_frame(lin, img, ref.rgb, ref.srgb8.reshape(H, W, 3))


# ---- 4. argument checks ------------------------------------------------------------------------------
def test_gpu_hit_inputs_argument_checks():
    from sightpy import Ray, _backend as B, _native as N, vec3

    lib, ctx = B.context()
    # a plain scene: in = NULL is srt_shade_level
    sc, ci = _identity_scene("glossy_sphere", False)
    O, D = _rays_at(sc, "glossy_sphere")
    t, ids, o = B.nearest_hits(sc, vec3(*O), vec3(*D))
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    rc, rgb_a, kids_a = _level(sc, ids, O, D, t, o)
    rc2, rgb_n, kids_n = _level(sc, ids, O, D, t, o, inputs=None)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(rgb_a, rgb_n) and np.array_equal(kids_a, kids_n)
    # ... a wrong light count names the cause
    inp = N.HitInputs()
    dist, irr = np.zeros((1, N_RAYS)), np.zeros((1, 3, N_RAYS))
    inp.n_lights, inp.light_dist, inp.light_irr = 1, N.ptr(dist), N.ptr(irr)
    rc, msg, _ = _level(sc, ids, O, D, t, o, inputs=inp)
    assert rc == N.ERR_ARG and "n_lights" in msg and "SRT_LIGHT_USER" in msg
    with pytest.raises(N.SrtError, match="n_lights"):
        N.check(lib, rc)
    # a scene with a user light: its arrays missing
    sc_l = scenes.example1(16, 12, 3)
    sc_l.Light_list += [PS.falloff()]
    inp = N.HitInputs()
    inp.n_lights = 1
    rc, msg, _ = _level(sc_l, ids, O, D, t, o, inputs=inp)
    assert rc == N.ERR_ARG and "light_dist" in msg
    rc, msg, _ = _level(sc_l, ids, O, D, t, o, inputs=None)
    assert rc == N.ERR_ARG and "n_lights" in msg
    # a flagged material without albedo
    sc_b, _ = _identity_scene("glossy_sphere", True)
    inp = N.HitInputs()
    rc, msg, _ = _level(sc_b, ids, O, D, t, o, inputs=inp)
    assert rc == N.ERR_ARG and "albedo" in msg and "SRT_MF_HIT_ALBEDO" in msg
    rc, msg, _ = _level(sc_b, ids, O, D, t, o, inputs=None)
    assert rc == N.ERR_ARG and "albedo" in msg
    # every other entry point refuses the flagged scene (uploaded directly), before any launch
    rc, msg, _ = _level(sc_b, ids, O, D, t, o)
    assert rc == N.ERR_ARG and "needs per-hit inputs" in msg
    ray = Ray(vec3(*O), vec3(*D), 0, sc_b.n, 0, 0, 0)
    with pytest.raises(N.SrtError, match="needs per-hit inputs"):
        B.trace_rays(ray, sc_b)
    with pytest.raises(N.SrtError, match="needs per-hit inputs"):
        B.trace_rays(ray, sc_b, hits=(ids, t, o))
    with pytest.raises(N.SrtError, match="needs per-hit inputs"):
        B.render_scene(sc_b, 1, mt=True)
    with pytest.raises(N.SrtError, match="needs per-hit inputs"):
        B.render_scene(sc_l, 1, seed=3)
    # and a plain scene renders again afterwards
    out = B.render_scene(scenes.example1(16, 12, 3), 1, mt=True)
    assert np.isfinite(out.rgb).all() and out.rgb.any()


# ---- 5. a normal map under a user light --------------------------------------------------------------
def test_gpu_normal_map_under_user_light(monkeypatch):
    from sightpy import _backend as B, _hybrid, vec3

    def build():
        sc = scenes.features(32, 24, 3)
        sc.Light_list[:] = [PS.falloff()]
        return sc

    sc = build()
    floor = sc.collider_list[0].assigned_primitive.material
    assert floor.normalmap is not None
    np.random.seed(5)
    state = np.random.get_state()
    plain = _planar3(_hybrid.render_linear(sc, 1), 32 * 24)

    sc = build()
    floor = sc.collider_list[0].assigned_primitive.material
    light = sc.Light_list[0]
    seen, current = [], {}
    orig_inputs, orig_irr = _hybrid.hit_inputs, light.get_irradiance

    def noting(scene, material, hit, n):
        current["material"], current["hit"] = material, hit
        return orig_inputs(scene, material, hit, n)

    def recording(dist_light, NdotL):
        seen.append((current["material"], current["hit"], np.array(NdotL, dtype=np.float64, copy=True)))
        return orig_irr(dist_light, NdotL)

    monkeypatch.setattr(_hybrid, "hit_inputs", noting)
    light.get_irradiance = recording
    np.random.set_state(state)
    rec = _planar3(_hybrid.render_linear(sc, 1), 32 * 24)
    assert np.array_equal(plain, rec)
    assert np.isfinite(rec).all() and rec.any()
    on_floor = [s for s in seen if s[0] is floor]
    assert on_floor and sum(len(np.atleast_1d(s[2])) for s in on_floor) >= 64
    L = light.get_L()
    for material, hit, ndotl in on_floor:
        Nm = B.material_normal(material, hit)  # srt_material_normal
        want = np.maximum(vec3(Nm[0], Nm[1], Nm[2]).dot(L), 0.0)
        assert np.array_equal(ndotl, want)
