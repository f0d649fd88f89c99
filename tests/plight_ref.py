"""Expected values for PositionalLight / SpotLight (tests/test_plight.py, tests/test_gpu_plight.py):
Glossy.get_color (glossy.py:25-110) restated in numpy with a light direction, distance and irradiance
per hit, from the oracle's own helpers (`intersect` with array D, `shading_normal`, `_tex_color`,
`raycolor`), installed over the oracle's module-level `shade_glossy` for the length of one test (its
`shade` calls it by global name).  This restatement is the definition the device shader follows.

Per light at the hits P (3, n) (un-nudged, as glossy.py:40 passes hit.point), float64, in this order:
    d = pos - P;  dist = sqrt(d.d);  L = d * (1.0 / dist);  NdotL = maximum(N.L, 0)
    irradiance = color * NdotL / dist ** 2.0 * intensity
    SpotLight: c = (-L).axis;  s = clip((c - cos_outer) / (cos_inner - cos_outer), 0, 1);
               irradiance = irradiance * (s * s * (3.0 - 2.0 * s))
    H = normalize(L + V)
    shadow rays from the nudged point along L (one direction per hit: the colliders' array-D
    intersection); seelight = (nearest over the shadow casters) >= dist
A DirectionalLight in the same Light_list is shaded as the oracle shades it.

While `RECORD` is a list, every positional light of every shaded batch appends a dict of its
intermediate arrays (dist, nearest, seelight, NdotL, s), so a test can assert which cases its scene
reaches.
"""
import numpy as np

import sightpy_oracle as O
from sightpy import Scene, Sphere, Plane, Cuboid, Glossy, TriangleMesh, image, rgb, vec3
from sightpy.lights import PositionalLight, SpotLight

RECORD = None


def shade_glossy(scene, m, c, r, t, orient, counts):
    P = r.O + r.D * t
    Nn = O.shading_normal(m, c, P, orient)
    diff = O._tex_color(m.diff_texture, c, P) * m.diff_coeff
    color = O.col3(scene.ambient_color) * diff
    V = r.D * -1.0
    nudged = P + Nn * 0.000001
    for light in scene.Light_list:
        positional = isinstance(light, PositionalLight)
        s = None
        if positional:
            d = O.col3(light.pos) - P
            dist = np.sqrt(O.dot(d, d))
            L = d * (1.0 / dist)
            NdotL = np.maximum(O.dot(Nn, L), 0.0)
            lv = O.col3(light.color) * NdotL / dist ** 2.0 * light.intensity
            if isinstance(light, SpotLight):
                cs = O.dot(L * -1.0, O.col3(light.axis))
                s = np.clip((cs - light.cos_outer) / (light.cos_inner - light.cos_outer), 0.0, 1.0)
                lv = lv * (s * s * (3.0 - 2.0 * s))
        else:
            L = O.col3(light.Ldir)
            dist = O.SKYBOX_DISTANCE
            NdotL = np.maximum(O.dot(Nn, L), 0.0)
            lv = O.col3(light.color) * NdotL
        H = O.normalize(L + V)
        ln = None
        if scene.shadowed_collider_list:
            for sc in scene.shadowed_collider_list:
                dd = O.intersect(sc, nudged, L, scalar_D=not positional)[0]
                ln = dd if ln is None else np.minimum(ln, dd)
            seelight = ln >= dist
            counts["shadow"] = counts.get("shadow", 0) + len(r)
        else:
            seelight = 1.0
        if positional and RECORD is not None:
            RECORD.append({"dist": dist, "nearest": ln, "seelight": np.broadcast_to(seelight, dist.shape),
                           "NdotL": NdotL, "s": s, "lv": lv})
        color = color + diff * lv * seelight
        if m.roughness != 0.0:
            F0 = np.abs((r.n - O.col3(m.n)) / (r.n + O.col3(m.n))) ** 2
            cos_t = np.clip(O.dot(V, H), 0.0, 1.0)
            F = F0 + (1.0 - F0) * (1.0 - cos_t) ** 5
            a = 2.0 / (m.roughness ** 2.0) - 2.0
            Dp = np.power(np.clip(O.dot(Nn, H), 0.0, 1.0), a) * (a + 2.0) / (2.0 * np.pi)
            color = color + F * Dp / (4.0 * np.clip(O.dot(Nn, V) * NdotL, 0.001, 1.0)) * seelight * lv * m.spec_coeff
    if r.depth < c.assigned_primitive.max_ray_depth:
        F0 = np.abs((scene.n - m.n) / (scene.n + m.n)) ** 2
        F0 = O.col3(F0)
        cos_t = np.clip(O.dot(V, Nn), 0.0, 1.0)
        F = F0 + (1.0 - F0) * (1.0 - cos_t) ** 5
        child = r.child(nudged, O.reflect(r.D, Nn), r.n, r.depth + 1, r.dfl, 1)
        color = color + O.raycolor(scene, child, counts) * F
    return color


def patch(monkeypatch):
    """Install the restatement over the oracle's shade_glossy until the test ends."""
    monkeypatch.setattr(O, "shade_glossy", shade_glossy)


def recorded(fn):
    """fn() with the positional lights' intermediate arrays recorded: (fn's result, the records)."""
    global RECORD
    RECORD = []
    try:
        out = fn()
        return out, RECORD
    finally:
        RECORD = None


def cat(records, key):
    return np.concatenate([np.ravel(r[key]) for r in records if r[key] is not None])


# ---- scenes -----------------------------------------------------------------------------------------
LIGHT_POS = (0.1, 0.0, -3.0)  # between the sphere and the cuboid, below their tops


def _materials():
    gold = Glossy(diff_color=rgb(1.0, 0.572, 0.184), n=vec3(0.15 + 3.58j, 0.4 + 2.37j, 1.54 + 1.91j),
                  roughness=0.0, spec_coeff=0.2, diff_coeff=0.8)
    blue = Glossy(diff_color=rgb(0.1, 0.2, 0.7), n=vec3(1.5 + 0.2j, 1.5 + 0.2j, 1.5 + 0.2j), roughness=0.2,
                  spec_coeff=0.4, diff_coeff=0.8)
    floor = Glossy(diff_color=image("checkered_floor.png", repeat=80.0), n=vec3(1.2 + 0.3j, 1.2 + 0.3j, 1.1 + 0.3j),
                   roughness=0.2, spec_coeff=0.3, diff_coeff=0.9)
    return gold, blue, floor


def _stage(width, height, depth):
    """Camera, ambient colour and a DirectionalLight (first in Light_list)."""
    sc = Scene(ambient_color=rgb(0.05, 0.05, 0.05))
    angle = -np.pi / 2 * 0.3
    sc.add_Camera(look_from=vec3(2.5 * np.sin(angle), 0.8, 2.5 * np.cos(angle) - 1.5),
                  look_at=vec3(0.0, -0.1, -3.0), screen_width=width, screen_height=height)
    sc.add_DirectionalLight(Ldir=vec3(0.52, 0.45, -0.5), color=rgb(0.15, 0.15, 0.15))
    return sc


def _objects(sc, depth, extra=None):
    """A sphere, a rotated cuboid (both shadow casters), `extra`, the floor, the sky box."""
    gold, blue, floor = _materials()
    sc.add(Sphere(material=gold, center=vec3(-0.75, 0.1, -3.0), radius=0.6, max_ray_depth=depth))
    cb = Cuboid(material=blue, center=vec3(1.0, 0.0, -3.0), width=0.7, height=1.0, length=0.7, max_ray_depth=depth,
                shadow=True)
    cb.rotate(θ=30, u=vec3(0, 1, 0))
    sc.add(cb)
    if extra is not None:
        sc.add(extra)
    sc.add(Plane(material=floor, center=vec3(0, -0.5, -3.0), width=120.0, height=120.0, u_axis=vec3(1.0, 0, 0),
                 v_axis=vec3(0, 0, -1.0), max_ray_depth=depth))
    sc.add_Background("stormydays.png")
    return sc


def room(width=48, height=36, depth=3, pos=LIGHT_POS, intensity=1.0, extra=None):
    """Floor, sphere, rotated shadow-casting cuboid, sky box; a DirectionalLight, then a PositionalLight
    between the objects: for hits on one side of it a shadow caster lies beyond the light."""
    sc = _stage(width, height, depth)
    sc.add_PositionalLight(pos=vec3(*pos), color=rgb(0.9, 0.8, 0.6), intensity=intensity)
    return _objects(sc, depth, extra)


def spot_room(width=48, height=36, depth=3):
    """room() with the PositionalLight replaced by a SpotLight above the objects shining down: its
    cone's edge (20 to 35 degrees from the axis) crosses the floor."""
    sc = _stage(width, height, depth)
    sc.add_SpotLight(pos=vec3(0.1, 1.2, -3.0), direction=vec3(0.1, -1.0, 0.05), color=rgb(0.9, 0.8, 0.6),
                     inner_deg=20.0, outer_deg=35.0, intensity=4.0)
    return _objects(sc, depth)


def many_lights_room(width=16, height=12, depth=3):
    """32 directional lights, then the positional light at index 32 (the shader's loop past its 32-bit
    seelight mask)."""
    sc = _stage(width, height, depth)
    for k in range(31):
        a = 2.0 * np.pi * k / 31
        sc.add_DirectionalLight(Ldir=vec3(np.cos(a), 0.6 + 0.01 * k, np.sin(a)), color=rgb(0.02, 0.02, 0.02))
    sc.add_PositionalLight(pos=vec3(*LIGHT_POS), color=rgb(0.9, 0.8, 0.6), intensity=1.0)
    assert len(sc.Light_list) == 33 and isinstance(sc.Light_list[32], PositionalLight)
    return _objects(sc, depth)


def near_floor_room(jit, width=16, height=12, depth=3):
    """The positional light 0.02 above the floor at the default intensity: 100 / 0.02**2 > 2**17, beyond
    the range of the device's fixed-point colour sums.  A frame this small has few floor hits, so the
    light stands over the one of sample 0 (jitter `jit`) nearest the camera: that hit is 0.02 from it."""
    sc = room(width, height, depth)
    Oa, Da = O.primary_rays(sc.camera, jit[0])
    near, ids = O.hit_ids(sc, Oa, Da)
    floor = next(i for i, c in enumerate(sc.collider_list) if type(c).__name__ == "Plane_Collider")
    k = np.flatnonzero(ids == floor)
    k = k[np.argmin(near[k])]
    P = Oa[:, k] + Da[:, k] * near[k]
    return room(width, height, depth, pos=(P[0], -0.48, P[2]), intensity=100.0)


def write_split_tetrahedron_obj(path, radius=0.45):
    """A tetrahedron whose four faces are split in three at a raised centre point: 12 triangles (the
    BVH is built from 8)."""
    V = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    V = list(radius * V / np.linalg.norm(V, axis=1, keepdims=True))
    faces = [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]
    F = []
    for a, b, c in faces:
        m = (V[a] + V[b] + V[c]) / 3.0
        V.append(m * 1.6)
        k = len(V) - 1
        F += [(a, b, k), (b, c, k), (c, a, k)]
    with open(path, "w") as fh:
        for p in V:
            fh.write("v %.17g %.17g %.17g\n" % tuple(p))
        for a, b, c in F:
            fh.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))
    return len(F)


def mesh_room(obj_path, width=48, height=36, depth=3):
    """room() with the 12-triangle mesh hanging under the light, shadowing the floor."""
    _, blue, _ = _materials()
    mesh = TriangleMesh(obj_path, center=vec3(0.1, -0.05, -2.6), material=blue, max_ray_depth=depth)
    return room(width, height, depth, pos=(0.1, 0.9, -2.6), intensity=2.0, extra=mesh)


def tinted_room(width=48, height=36, depth=3):
    """A user material (tests/user_classes.py Tinted) on a sphere above the built-in Glossy floor, under
    a positional light: a hybrid scene whose built-in hits are shaded on the device one level at a time."""
    import user_classes as U

    ball = Sphere(material=U.Tinted(rgb(0.2, 0.4, 0.9), 0.5), center=vec3(0.1, 0.0, -2.2), radius=0.3, max_ray_depth=depth)
    return room(width, height, depth, pos=(0.1, 0.9, -2.6), intensity=2.0, extra=ball)
