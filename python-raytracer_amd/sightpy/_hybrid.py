"""Scenes holding user subclasses of `Collider`, `Material`, `texture` or `Light`: the reference's
duck-typed plugin dispatch (`ray.py:122-148` calls `intersect` and `get_color` on whatever the lists
hold, `glossy.py:30,38-44` the texture's `get_color(hit)` and the lights' `get_L` / `get_distance` /
`get_irradiance`; contracts at `geometry/collider.py:12-14`, `materials/material.py:42-44`,
`textures/texture.py:14-16` and `lights.py:12-22`).

A user class's Python methods cannot run inside a kernel, so such a scene is traced by the
reference's own recursion structure, driven from the host one batch level at a time, with every
step the device can take on the device:

  * intersect: built-in colliders on the device (`srt_intersect_collider`), a user collider's own
    `intersect(O, D)` (its code, on its batch);
  * nearest hit and the tie rule: as ray.py:127-135 (every collider at the nearest distance shades
    its rays, the colours added);
  * get_color: a user material's own `get_color(scene, ray, hit)` (its recursion through
    `get_raycolor` comes back here); a built-in material on a built-in collider shades its rays on
    the device one level deep (`srt_shade_level`: the colour it adds before its children, and the
    children with the factor their colour is multiplied by), and the children are traced by this
    same recursion, so they can hit user colliders;
  * a user texture on a built-in Glossy / Diffuse / Emissive, a user Light in Light_list: the
    material is still shaded on the device, one level at a time (`srt_shade_level_inputs`: shading
    normal, shadow rays, Lambert and Cook-Torrance terms, Fresnel weights, children).  Only the
    user's own methods run here, on the level's batch, as the reference runs them:
    `texture.get_color(hit)` (its `hit.get_uv()` is a device entry point), and for each user light
    `get_distance(hit.point)` and `get_irradiance(dist_light, NdotL)` with `NdotL =
    maximum(N.dot(L), 0)` of the material's device normal (glossy.py:41; that dot product is the
    callback's argument, nothing else of the material is computed on the host).  Their values go to
    the device per hit.  `get_L()` must be one direction (a vec3 of scalars): a per-ray light
    direction is refused.  Per-hit inputs exist only in this host-driven path.  (The built-in
    `PositionalLight` / `SpotLight` need none of this: the device computes their direction, distance
    and irradiance per hit, also in a scene with user colliders or materials; beside a user texture or
    user Light they are refused, `_check`.)

Scenes made only of built-in classes never come here: they render in the device kernels whole.

What the device cannot do for a user class is refused (NotImplementedError) rather than computed
on the CPU, with or without user textures and lights in the scene: a built-in material on a user collider (the device shaders take the surface from the
built-in colliders' device code), and a user collider casting shadows (`shadow=True`) in a scene
with built-in Glossy materials (their shadow rays, glossy.py:54-67, are traced on the device
against the device's colliders; a built-in collider with a user material is one of them).  Monte-Carlo materials (Diffuse, `mc=True` Refractive) shaded on
the device here draw from the device stream keyed by each level's ray index: valid samples, but not
the ones a whole-device render of the same pixel draws.
"""
from functools import reduce

import numpy as np

from .utils.constants import FARAWAY
from .utils.vector3 import vec3, rgb, extract

__all__ = ["device_collider", "device_material", "device_texture", "device_light", "on_device", "is_hybrid", "raycolor", "shade_level",
           "render_linear", "nearest_distance"]

_SURFACE_METHODS = ("intersect", "get_Normal", "get_uv")


def _builtin_colliders():
    from .geometry.sphere import Sphere_Collider
    from .geometry.plane import Plane_Collider
    from .geometry.cuboid import Cuboid_Collider
    from .geometry.triangle import Triangle_Collider

    return (Sphere_Collider, Plane_Collider, Cuboid_Collider, Triangle_Collider)


def _builtin_materials():
    from .materials import Glossy, Refractive, ThinFilmInterference, Diffuse, Emissive
    from .backgrounds.skybox import SkyBox_Material

    return (Glossy, Refractive, ThinFilmInterference, Diffuse, Emissive, SkyBox_Material)


def device_collider(c):
    """A built-in collider (or a subclass of one that keeps its intersect / get_Normal / get_uv):
    its intersection and surface run in the device code."""
    for base in _builtin_colliders():
        if isinstance(c, base):
            t = type(c)
            return all(getattr(t, m, None) is getattr(base, m, None) for m in _SURFACE_METHODS)
    return False


def device_material(m):
    """A built-in material (or a subclass of one that keeps its get_color)."""
    from .materials.material import Material

    return isinstance(m, _builtin_materials()) and type(m).get_color is Material.get_color


def device_texture(t):
    """A `solid_color` or `image` (or a subclass of one that keeps its get_color): the device reads
    its colour from the scene tables."""
    from .textures.texture import solid_color, image

    for base in (solid_color, image):
        if isinstance(t, base):
            return type(t).get_color is base.get_color
    return False


_LIGHT_METHODS = ("get_L", "get_distance", "get_irradiance")


def device_light(l):
    """A `DirectionalLight`, `PointLight`, `PositionalLight` or `SpotLight` (or a subclass of one that
    keeps get_L / get_distance / get_irradiance): a record of the device's light table."""
    from .lights import DirectionalLight, PointLight, PositionalLight, SpotLight

    for base in (DirectionalLight, PointLight, SpotLight, PositionalLight):  # (a SpotLight is a PositionalLight)
        if isinstance(l, base):
            t = type(l)
            return all(getattr(t, m, None) is getattr(base, m, None) for m in _LIGHT_METHODS)
    return False


def material_texture(m):
    """The colour texture of a built-in Glossy / Diffuse / Emissive, else None."""
    from .materials import Glossy, Diffuse, Emissive

    if isinstance(m, (Glossy, Diffuse)):
        return getattr(m, "diff_texture", None)
    if isinstance(m, Emissive):
        return getattr(m, "texture_color", None)
    return None


def user_texture(m):
    """The user texture a built-in material holds (its colour arrives per hit), else None."""
    if not device_material(m):
        return None
    t = material_texture(m)
    return t if t is not None and not device_texture(t) else None


def needs_inputs(scene):
    """Whether a built-in material holds a user texture or Light_list a user Light."""
    return (any(user_texture(c.assigned_primitive.material) is not None for c in scene.collider_list)
            or not all(device_light(l) for l in scene.Light_list))


def on_device(c):
    """The collider and its material both lower to the device tables."""
    return device_collider(c) and device_material(c.assigned_primitive.material)


def is_hybrid(scene):
    """Whether `scene` holds a user Collider / Material / texture / Light subclass (cached per
    collider list and light list)."""
    key = (id(scene.collider_list), len(scene.collider_list), tuple(id(l) for l in scene.Light_list))
    cached = getattr(scene, "_hybrid_key", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    res = not all(on_device(c) for c in scene.collider_list) or needs_inputs(scene)
    if res:
        _check(scene)
    scene._hybrid_key = (key, res)
    return res


def _check(scene):
    from .materials import Glossy
    from .lights import PositionalLight

    if needs_inputs(scene) and any(isinstance(l, PositionalLight) and device_light(l) for l in scene.Light_list):
        raise NotImplementedError(
            "a PositionalLight / SpotLight in a scene that needs per-hit inputs (a user texture on a built-in "
            "material, or a user Light): the per-hit-input shaders have no positional-light path")

    for c in scene.collider_list:
        m = c.assigned_primitive.material
        if not device_collider(c) and device_material(m):
            raise NotImplementedError(
                "built-in material %s on the user collider %s: the device shaders take the hit's surface from "
                "the built-in colliders; give the collider a user Material" % (type(m).__name__, type(c).__name__))
    shadowing = [c for c in scene.shadowed_collider_list if not device_collider(c)]
    glossy = [c for c in scene.collider_list if on_device(c) and isinstance(c.assigned_primitive.material, Glossy)]
    if shadowing and glossy:
        raise NotImplementedError(
            "the user collider %s casts shadows (shadow=True) on built-in Glossy materials, whose shadow rays "
            "(glossy.py:54-67) are traced on the device; add its primitive with shadow=False"
            % type(shadowing[0]).__name__)


def _intersect(c, ray):
    """(distance, orientation) arrays of collider c for the batch (collider.py:12-14 contract)."""
    if device_collider(c):
        from ._backend import intersect_collider

        out = intersect_collider(c, ray.origin, ray.dir)
        return out[0], out[1]
    d, o = c.intersect(ray.origin, ray.dir)
    n = len(ray)
    return (np.broadcast_to(np.asarray(d, dtype=np.float64), (n,)),
            np.broadcast_to(np.asarray(o, dtype=np.float64), (n,)))


def nearest_distance(ray, scene):
    """reduce(np.minimum, distances) over every collider (ray.py:125-129)."""
    return reduce(np.minimum, [_intersect(c, ray)[0] for c in scene.collider_list])


def raycolor(ray, scene):
    """get_raycolor (ray.py:122-148) of a batch in a scene with user classes."""
    from .ray import Hit

    inters = [_intersect(c, ray) for c in scene.collider_list]
    distances, orientations = zip(*inters)
    nearest = reduce(np.minimum, distances)
    color = rgb(0.0, 0.0, 0.0)
    for coll, dis, orient in zip(scene.collider_list, distances, orientations):
        hit_check = (nearest != FARAWAY) & (dis == nearest)
        if np.any(hit_check):
            material = coll.assigned_primitive.material
            hit = Hit(extract(hit_check, dis), extract(hit_check, orient), material, coll, coll.assigned_primitive)
            cc = material.get_color(scene, ray.extract(hit_check), hit)
            color += cc.place(hit_check)
    return color


def _rows(v, n):
    """A user method's result (a scalar, or a vec3 of scalars or arrays) as float64 (3, n)."""
    comps = (v.x, v.y, v.z) if hasattr(v, "x") else (v, v, v)
    return np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(c, dtype=np.float64).reshape(-1)
                                                          if np.ndim(c) else np.asarray(c, dtype=np.float64), (n,))
                                          for c in comps]))


def hit_inputs(scene, material, hit, n):
    """What the user's texture / Light methods return at `hit` (hit.point set), for
    srt_shade_level_inputs: (albedo (3, n) or None, light_dist (k, n), light_irr (k, 3, n)) over the
    scene's k user lights in Light_list order.  The lights are consulted for a Glossy only, as in the
    reference (glossy.py:37-44); other materials never read their rows."""
    from .materials import Glossy

    tex = user_texture(material)
    albedo = _rows(tex.get_color(hit), n) if tex is not None else None
    users = [l for l in scene.Light_list if not device_light(l)]
    dist = np.zeros((len(users), n))
    irr = np.zeros((len(users), 3, n))
    if users and isinstance(material, Glossy):
        N = material.get_Normal(hit)
        if not hasattr(N, "x"):
            N = vec3(N[0], N[1], N[2])
        for k, l in enumerate(users):
            NdotL = np.maximum(N.dot(l.get_L()), 0.0)
            d = l.get_distance(hit.point)
            dist[k] = np.broadcast_to(np.asarray(d, dtype=np.float64).reshape(-1) if np.ndim(d) else d, (n,))
            irr[k] = _rows(l.get_irradiance(d, NdotL), n)
    return albedo, dist, irr


def shade_level(scene, material, ray, hit):
    """A built-in material's get_color in a scene with user classes: its own colour from the
    device (srt_shade_level; srt_shade_level_inputs when the scene holds a user texture or Light,
    whose methods run here on this batch), plus each child's colour (this recursion) times its factor."""
    import ctypes

    from . import _backend as B, _native as N
    from .ray import Ray

    lib, ctx = B.context()
    n = len(ray)
    uniq, inv = B._media_of(ray.n, n)
    L = B.upload(scene, extra_media=uniq)
    remap = np.array([L.media_keys.index(k) for k in uniq], dtype=np.int32)
    med = np.ascontiguousarray(remap[inv])
    dev = L.device_index[scene.collider_list.index(hit.collider)]
    O, D = B._planar(ray.origin, n), B._planar(ray.dir, n)
    local = np.empty((3, n))
    a = N.TraceArgs()
    a.n = n
    a.origin, a.dir, a.medium = N.ptr(O), N.ptr(D), N.ptr(med)
    a.depth, a.diffuse_reflections = int(ray.depth), int(ray.diffuse_reflections)
    a.seed = int(B._default_seed()) & (2**64 - 1)
    a.out_rgb = N.ptr(local)
    ids = np.full(n, dev, dtype=np.int32)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(hit.distance, dtype=np.float64), (n,)))
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(hit.orientation, dtype=np.float64), (n,)))
    inputs = None
    if needs_inputs(scene):
        albedo, ldist, lirr = hit_inputs(scene, material, hit, n)
        inputs = N.HitInputs()
        inputs.albedo = N.ptr(albedo)
        inputs.n_lights = len(ldist)
        inputs.light_dist, inputs.light_irr = (N.ptr(ldist), N.ptr(lirr)) if len(ldist) else (None, None)
    cap = 2 * n  # (a refractive hit's two children; a Diffuse fan-out asks for more, below)
    for _ in range(2):
        arrs = {"origin": np.empty((3, cap)), "dir": np.empty((3, cap)), "weight": np.empty((3, cap)),
                "parent": np.empty(cap, np.int32), "medium": np.empty(cap, np.int32),
                "depth": np.empty(cap, np.int32), "diffuse_reflections": np.empty(cap, np.int32)}
        kids = N.Children()
        kids.cap = cap
        for k, v in arrs.items():
            setattr(kids, k, N.ptr(v))
        if inputs is None:
            rc = lib.srt_shade_level(ctx, ctypes.byref(a), N.ptr(ids), N.ptr(t), N.ptr(o), ctypes.byref(kids), None)
        else:
            rc = lib.srt_shade_level_inputs(ctx, ctypes.byref(a), N.ptr(ids), N.ptr(t), N.ptr(o),
                                            ctypes.byref(inputs), ctypes.byref(kids), None)
        if rc != 0 and kids.n > cap:
            cap = int(kids.n)  # room for them all, then once more
            continue
        N.check(lib, rc)
        break
    else:  # (the count the first attempt reported did not hold them: never read truncated children)
        raise RuntimeError("srt_shade_level: %d children exceed the room made for them twice" % int(kids.n))
    color = [local[0].copy(), local[1].copy(), local[2].copy()]
    nk = int(kids.n)
    if nk:
        media = np.array([[complex(v) for v in L.media_keys[m]] for m in range(len(L.media_keys))])
        depth, dfl = arrs["depth"][:nk], arrs["diffuse_reflections"][:nk]
        # the reference's batches carry one depth and one diffuse count: one batch per pair
        for dv, fv in sorted(set(zip(depth.tolist(), dfl.tolist()))):
            sel = np.nonzero((depth == dv) & (dfl == fv))[0]
            mk = media[arrs["medium"][:nk][sel]]
            child = Ray(vec3(*(arrs["origin"][k, sel] for k in range(3))), vec3(*(arrs["dir"][k, sel] for k in range(3))),
                        dv, vec3(mk[:, 0], mk[:, 1], mk[:, 2]), 0, 0, fv)
            cc = raycolor(child, scene)
            par = arrs["parent"][:nk][sel]
            for k, comp in enumerate((cc.x, cc.y, cc.z)):
                np.add.at(color[k], par, arrs["weight"][k, sel] * np.broadcast_to(comp, sel.shape))
    return rgb(color[0], color[1], color[2])


def render_linear(scene, samples_per_pixel):
    """Scene.render's linear colour (scene.py:71-118) for a scene with user classes: numpy's stream
    drawn in the reference's order (spp get_ray draws, then the sizing draw), every sample's batch
    through raycolor, averaged."""
    rays = [scene.camera.get_ray(scene.n) for _ in range(samples_per_pixel)]
    scene.camera.get_ray(scene.n)  # the reference's sizing draw (scene.py:81)
    color = rgb(0.0, 0.0, 0.0)
    for r in rays:
        color += raycolor(r, scene)
    return color / samples_per_pixel
