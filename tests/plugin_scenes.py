"""User subclasses of sightpy's `texture` and `Light`, written the way a reference user writes them
(numpy on vec3 batches; contracts at reference textures/texture.py:14-16 and lights.py:12-22, used at
glossy.py:30,38-44), and three scenes holding them in example1's setting.  `sp` is the sightpy module
to build with: this package by default; tests/golden/gen_plugin_golden.py passes the reference's
module, so the fixtures come from the reference itself running the same classes.  Nothing here is
library code."""
import numpy as np

_CLASSES = {}


def classes(sp=None):
    """The user classes defined against `sp`'s base classes (one set per module): a namespace with
    Bands, Checker3D, Falloff, PlainDirectional and `calls`, the count of each user method's calls."""
    if sp is None:
        import sightpy as sp
    if id(sp) in _CLASSES:
        return _CLASSES[id(sp)]
    import importlib

    texture = importlib.import_module(sp.__name__ + ".textures.texture").texture
    lights = importlib.import_module(sp.__name__ + ".lights")
    SKYBOX_DISTANCE = importlib.import_module(sp.__name__ + ".utils.constants").SKYBOX_DISTANCE
    vec3, rgb = sp.vec3, sp.rgb
    calls = {"get_color": 0, "get_L": 0, "get_distance": 0, "get_irradiance": 0}

    def mix(a, b, s):
        return rgb(a.x + (b.x - a.x) * s, a.y + (b.y - a.y) * s, a.z + (b.z - a.z) * s)

    class Bands(texture):
        """Stripes along v of the primitive's uv (hit.get_uv())."""

        def __init__(self, a, b, count=7.0):
            self.a, self.b, self.count = a, b, count

        def get_color(self, hit):
            calls["get_color"] += 1
            u, v = hit.get_uv()
            return mix(self.a, self.b, np.floor(v * self.count + 0.3) % 2.0)

    class Checker3D(texture):
        """A solid checker of the hit point; `by="distance"`: rings of hit.distance instead, for
        materials under which the reference leaves hit.point unset (Emissive.get_color,
        emissive.py:21-23, calls the texture without computing the point)."""

        def __init__(self, a, b, scale=1.7, by="point"):
            self.a, self.b, self.scale, self.by = a, b, scale, by

        def get_color(self, hit):
            calls["get_color"] += 1
            f = self.scale
            if self.by == "distance":
                s = np.floor(hit.distance * f + 0.25) % 2.0
            else:
                p = hit.point
                s = (np.floor(p.x * f + 0.25) + np.floor(p.y * f + 0.25) + np.floor(p.z * f + 0.25)) % 2.0
            return mix(self.a, self.b, s)

    class Falloff(lights.Light):
        """A lamp at `pos` shining along one direction: the distance to it per hit (so it casts
        shadows only of what lies nearer than itself), irradiance falling off with the distance."""

        def __init__(self, pos, color, Ldir, k=6.0):
            super().__init__(pos, color)
            self.Ldir = Ldir.normalize()
            self.k = k

        def get_L(self):
            calls["get_L"] += 1
            return self.Ldir

        def get_distance(self, M):
            calls["get_distance"] += 1
            return np.sqrt((self.pos - M).dot(self.pos - M))

        def get_irradiance(self, dist_light, NdotL):
            calls["get_irradiance"] += 1
            return self.color * NdotL * self.k / (1.0 + dist_light ** 2.0)

    class PlainDirectional(lights.Light):
        """DirectionalLight (lights.py:38-52) restated by a user, from the Light base class."""

        def __init__(self, Ldir, color):
            self.Ldir = Ldir
            self.color = color

        def get_L(self):
            return self.Ldir

        def get_distance(self, M):
            return SKYBOX_DISTANCE

        def get_irradiance(self, dist_light, NdotL):
            return self.color * NdotL

    class NS:
        pass

    ns = NS()
    ns.Bands, ns.Checker3D, ns.Falloff, ns.PlainDirectional, ns.calls = Bands, Checker3D, Falloff, PlainDirectional, calls
    _CLASSES[id(sp)] = ns
    return ns


KINDS = ("texture", "light", "both")


def falloff(sp=None):
    """The user light of the 'light' and 'both' scenes."""
    if sp is None:
        import sightpy as sp
    return classes(sp).Falloff(sp.vec3(-1.5, 2.0, -1.0), sp.rgb(0.9, 0.8, 0.6), sp.vec3(-0.3, 0.8, 0.5))


def scene(kind, width=48, height=36, depth=3, sp=None):
    """example1's setting.  'texture': Bands on the gold sphere's Glossy, Checker3D on the floor's
    rough Glossy and (by distance) in a small Emissive sphere, under the built-in DirectionalLight;
    'light': the built-in textures under [DirectionalLight, Falloff]; 'both': the user textures under
    both lights."""
    if sp is None:
        import sightpy as sp
    C = classes(sp)
    vec3, rgb = sp.vec3, sp.rgb
    user_tex = kind in ("texture", "both")
    gold_c = C.Bands(rgb(1.0, 0.572, 0.184), rgb(0.2, 0.3, 0.8)) if user_tex else rgb(1.0, 0.572, 0.184)
    floor_c = (C.Checker3D(rgb(0.9, 0.9, 0.85), rgb(0.15, 0.1, 0.1)) if user_tex
               else sp.image("checkered_floor.png", repeat=80.0))
    lamp_c = C.Checker3D(rgb(2.0, 1.6, 0.4), rgb(0.3, 0.9, 1.5), scale=9.0, by="distance") if user_tex else rgb(2.0, 1.6, 0.4)
    gold = sp.Glossy(diff_color=gold_c, n=vec3(0.15 + 3.58j, 0.4 + 2.37j, 1.54 + 1.91j), roughness=0.0,
                     spec_coeff=0.2, diff_coeff=0.8)
    blue = sp.Glossy(diff_color=rgb(0.0, 0, 0.1), n=vec3(1.3 + 1.91j, 1.3 + 1.91j, 1.4 + 2.91j), roughness=0.2,
                     spec_coeff=0.5, diff_coeff=0.3)
    floor = sp.Glossy(diff_color=floor_c, n=vec3(1.2 + 0.3j, 1.2 + 0.3j, 1.1 + 0.3j), roughness=0.2, spec_coeff=0.3,
                      diff_coeff=0.9)
    lamp = sp.Emissive(color=lamp_c)
    sc = sp.Scene(ambient_color=rgb(0.05, 0.05, 0.05))
    angle = -np.pi / 2 * 0.3
    sc.add_Camera(look_from=vec3(2.5 * np.sin(angle), 0.25, 2.5 * np.cos(angle) - 1.5),
                  look_at=vec3(0.0, 0.25, -3.0), screen_width=width, screen_height=height)
    sc.add_DirectionalLight(Ldir=vec3(0.52, 0.45, -0.5), color=rgb(0.15, 0.15, 0.15))
    if kind in ("light", "both"):
        sc.Light_list += [falloff(sp)]
    sc.add(sp.Sphere(material=gold, center=vec3(-0.75, 0.1, -3.0), radius=0.6, max_ray_depth=depth))
    sc.add(sp.Sphere(material=blue, center=vec3(1.25, 0.1, -3.0), radius=0.6, max_ray_depth=depth))
    sc.add(sp.Sphere(material=lamp, center=vec3(0.25, -0.3, -2.2), radius=0.2, max_ray_depth=depth, shadow=False))
    sc.add(sp.Plane(material=floor, center=vec3(0, -0.5, -3.0), width=120.0, height=120.0, u_axis=vec3(1.0, 0, 0),
                    v_axis=vec3(0, 0, -1.0), max_ray_depth=depth))
    sc.add_Background("stormydays.png")
    return sc
