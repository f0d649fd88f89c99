"""Lights (reference `sightpy/lights.py:6-52`).  Lights only affect Glossy materials.

`DirectionalLight` is lowered to the device light table.  The reference `PointLight.get_L`
references undefined names (lights.py:30-31), so rendering a scene with a point light raises
NameError as soon as a Glossy surface is shaded (glossy.py:38 calls get_L for every light).  Here
the point light is lowered as a record and the device raises the same way: a Glossy hit under a
point light sets an error bit and the render fails with SRT_ERR_NAME -> NameError.  Scenes whose
rays never hit a Glossy surface render as in the reference (the light is never consulted).
`PointLight` and `Scene.add_PointLight` stay exactly that; the light at a position that works is
`PositionalLight` below.

`PositionalLight` is the light the reference's `PointLight` was meant to be (lights.py:25-37): its
direction, distance and irradiance depend on the hit point, so `get_L` takes the hit points `M`
(a vec3 batch).  `SpotLight` is a `PositionalLight` whose irradiance falls to zero between two cone
angles, so its `get_irradiance` takes the light direction at the hits too.  The methods below are
the definition of both lights; the device shader (csrc/rt_device.h shade_glossy, SRT_LIGHT_POSITIONAL)
evaluates the same float64 operations in the same order per hit, and a user `Material.get_color`
may call them on its own batch.  A subclass that overrides one of the three methods is a user light
(`_hybrid.device_light`), to which the rule of one direction for every hit applies.
"""
import numpy as np

from .utils.constants import SKYBOX_DISTANCE

__all__ = ["Light", "PointLight", "DirectionalLight", "PositionalLight", "SpotLight"]


class Light:
    def __init__(self, pos, color):
        self.pos = pos
        self.color = color


class PointLight(Light):
    def get_L(self):
        # lights.py:30-31: `(self.pos - M) * (1.0 / (dist_light))` with M, dist_light undefined
        raise NameError("name 'M' is not defined")

    def get_distance(self, M):
        return np.sqrt((self.pos - M).dot(self.pos - M))

    def get_irradiance(self, dist_light, NdotL):
        return self.color * NdotL / (dist_light ** 2.0) * 100


class DirectionalLight(Light):
    def __init__(self, Ldir, color):
        self.Ldir = Ldir
        self.color = color

    def get_L(self):
        return self.Ldir

    def get_distance(self, M):
        return SKYBOX_DISTANCE

    def get_irradiance(self, dist_light, NdotL):
        return self.color * NdotL


class PositionalLight(Light):
    """A light at `pos` shining equally in every direction; the irradiance falls with the square of
    the distance: color * NdotL / dist**2 * intensity."""

    def __init__(self, pos, color, intensity=100.0):
        self.pos = pos
        self.color = color
        self.intensity = float(intensity)

    def get_distance(self, M):
        return np.sqrt((self.pos - M).dot(self.pos - M))

    def get_L(self, M):
        return (self.pos - M) * (1.0 / self.get_distance(M))

    def get_irradiance(self, dist_light, NdotL):
        return self.color * NdotL / dist_light ** 2.0 * self.intensity


class SpotLight(PositionalLight):
    """A PositionalLight shining along `direction`: full irradiance within `inner_deg` of the axis,
    none beyond `outer_deg`, a smoothstep in between (angles from the axis, inner < outer <= 90)."""

    def __init__(self, pos, direction, color, inner_deg, outer_deg, intensity=100.0):
        if not (0.0 <= inner_deg < outer_deg <= 90.0):
            raise ValueError("SpotLight needs 0 <= inner_deg < outer_deg <= 90, got %r and %r" % (inner_deg, outer_deg))
        PositionalLight.__init__(self, pos, color, intensity)
        self.axis = direction.normalize()
        if not np.isfinite(self.axis.dot(self.axis)) or self.axis.dot(self.axis) == 0.0:
            raise ValueError("SpotLight direction must be a non-zero vector")
        self.cos_inner = float(np.cos(np.radians(inner_deg)))
        self.cos_outer = float(np.cos(np.radians(outer_deg)))

    def cone_factor(self, L):
        """s*s*(3 - 2*s) of the light direction L at the hits (pointing from the hit to the light)."""
        c = (-L).dot(self.axis)
        s = np.clip((c - self.cos_outer) / (self.cos_inner - self.cos_outer), 0.0, 1.0)
        return s * s * (3.0 - 2.0 * s)

    def get_irradiance(self, dist_light, NdotL, L):
        return PositionalLight.get_irradiance(self, dist_light, NdotL) * self.cone_factor(L)
