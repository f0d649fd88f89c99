"""Scene assembly and the render entry point (reference `sightpy/scene.py:28-166`).

`Scene` keeps the reference's assembly API.  `render()` is the drop-in boundary: instead of the
reference's `multiprocessing.Pool` over samples (scene.py:80-116) it lowers the scene to flat
device tables once, generates the camera jitter of numpy's global RNG in the reference's order on
the GPU (so a seeded render consumes the same random stream), and runs the whole
samples x depths wavefront plus the sRGB resolve on the GPU(s) through `libsightpy_hip.so`.
"""
import time

import numpy as np
from PIL import Image

from .camera import Camera
from .utils.constants import *
from .utils.vector3 import vec3, rgb
from . import lights
from .backgrounds.skybox import SkyBox
from .backgrounds.panorama import Panorama

__all__ = ["Scene"]


class Scene:
    def __init__(self, ambient_color=rgb(0.01, 0.01, 0.01), n=vec3(1.0, 1.0, 1.0)):
        self.scene_primitives = []
        self.collider_list = []
        self.shadowed_collider_list = []
        self.Light_list = []
        self.importance_sampled_list = []
        self.ambient_color = ambient_color
        self.n = n
        self.last_stats = None
        self._history = None  # _backend.TemporalHistory of render(denoise={"temporal": True})

    def add_Camera(self, look_from, look_at, **kwargs):
        self.camera = Camera(look_from, look_at, **kwargs)

    def add_PointLight(self, pos, color):
        self.Light_list += [lights.PointLight(pos, color)]

    def add_PositionalLight(self, pos, color, intensity=100.0):
        self.Light_list += [lights.PositionalLight(pos, color, intensity)]

    def add_SpotLight(self, pos, direction, color, inner_deg, outer_deg, intensity=100.0):
        self.Light_list += [lights.SpotLight(pos, direction, color, inner_deg, outer_deg, intensity)]

    def add_DirectionalLight(self, Ldir, color):
        self.Light_list += [lights.DirectionalLight(Ldir.normalize(), color)]

    def add(self, primitive, importance_sampled=False):
        self.scene_primitives += [primitive]
        self.collider_list += primitive.collider_list
        if importance_sampled == True:
            self.importance_sampled_list += [primitive]
        if primitive.shadow == True:
            self.shadowed_collider_list += primitive.collider_list

    def add_Background(self, img, light_intensity=0.0, blur=0.0, spherical=False):
        if spherical == False:
            primitive = SkyBox(img, light_intensity=light_intensity, blur=blur)
        else:
            primitive = Panorama(img, light_intensity=light_intensity, blur=blur)
        self.scene_primitives += [primitive]
        self.collider_list += primitive.collider_list

    def render(self, samples_per_pixel, progress_bar=False, batch_size=None, rng="numpy", seed=None, denoise=False):
        """Render `samples_per_pixel` samples and return a PIL RGB image.

        rng="numpy" (default) draws the primary-ray jitter from numpy's global legacy RNG exactly
        as the reference does (including the extra sizing draw at scene.py:81), so seeded renders
        match the reference: the stream is generated on the GPU inside the render (rt_mt.h,
        bit-equal to np.random.rand) and numpy's global state is advanced past it.
        rng="numpy-host" draws the same stream with numpy on the host.  rng="device" generates
        independent jitter on the GPU (Philox keyed by pixel and sample).  `batch_size` bounds the
        samples per device pass.

        With several GPUs ($SIGHTPY_DEVICES, e.g. "0,1,2,3" or "all") the frame is split into row
        bands dealt round-robin over the GPUs (at most 8 bands per GPU: e.g. 27-row bands at 1080p
        on 8 GPUs, 2-row bands for a Diffuse fan-out scene; rt_device.h shard_band_height) and
        gathered over RCCL (the reference's
        multiprocessing.Pool over samples, scene.py:80-116, is replaced); the image does not depend
        on the number of GPUs.

        A scene holding user subclasses of Collider, Material, texture or Light is rendered by the
        host-driven recursion of `_hybrid.py` (their methods on the host, every built-in step on the
        device; a user texture's colour and a user light's distance and irradiance reach the device
        shaders per hit).

        `denoise` (no reference counterpart): True filters the frame on the GPU before it is resolved
        -- the first-hit normal, albedo, position and depth images of the scene (`get_aovs`) guide an
        edge-avoiding a-trous wavelet filter over the linear RGB (srt_denoise) -- which makes a frame
        of few samples usable; a dict overrides the filter's `levels` (0..8) and `sigma_color`,
        `sigma_normal`, `sigma_albedo`, `sigma_plane` (an unknown key or a bad value raises ValueError
        before anything runs).  The samples are drawn and traced exactly as without it, and numpy's
        RNG is left in the same state.  Not available for a scene with user subclasses
        (NotImplementedError).

        The dict's `"variance": True` and `"demodulate": True` (independent, both off by default) select the
        half-frame mode (srt_denoise_var): the same samples are traced as two half-frames, samples
        0 .. spp//2 - 1 and the rest.  `variance` takes a per-pixel noise estimate from their difference and
        weighs colour differences against it (`"sigma_lum"`, default 1, in place of `sigma_color`): an edge
        the guides do not see survives where the frame is clean, and strong noise is still averaged.
        `demodulate` filters colour / albedo and multiplies the albedo back, which keeps texture detail.
        Half-frames, guides and the filter's planes stay in device memory; only the uint8 image is copied
        out.  Needs spp >= 2 (ValueError) and a single GPU (NotImplementedError with several selected).

        `"temporal": True` (off by default; it selects the half-frame mode too, and `variance` / `demodulate` keep
        their meaning) is for the frames of an animation: before the filter runs, each half-frame is blended with
        its own history -- the accumulated half-frames of the earlier frames of this scene, reprojected through the
        previous frame's camera and accepted where collider id, normal and plane distance agree
        (srt_temporal_accumulate; `"max_history"`, default 32, bounds the accumulated length, `"temporal_normal"`
        0.1 and `"temporal_plane"` 0.02 are the two acceptance thresholds).  With `demodulate` the history holds
        colour / albedo.  The history lives in device memory with the scene; `reset_history()` drops it, as does
        a frame of another size.  Moving objects are reprojected as if static (their history is rejected where
        the geometry changed) unless `"motion": True` is given too (a bool, off by default, ignored without
        `temporal`): each pixel is then first mapped back by the rigid motion of the collider it sees, derived
        from the collider tables of this frame and the one before (_motion.collider_motion), so a translated or
        rotated Sphere, Plane, Cuboid or Triangle keeps its history; `last_stats["denoise"]` then holds
        `motion_moved` and `motion_unknown`, the colliders that moved and those no rigid motion explains (a
        changed size, a deformed mesh, a reordered or edited collider list: no history for them).  The first
        frame, the frame after `reset_history()` and the frame after one rendered without `motion` run without
        a table.  The guides are first-hit only: a moving object's shadow and its reflections in other objects
        still lag.
        """
        from . import _backend as B
        from . import _hybrid

        dn = B.denoise_params(denoise)
        if dn is not None and "variance" in dn:
            return self._render_denoised_halves(samples_per_pixel, batch_size, rng, seed, dn)
        if dn is not None:
            return self._render_denoised(samples_per_pixel, batch_size, rng, seed, dn)
        print("Rendering...")
        t0 = time.time()
        if rng not in ("numpy", "numpy-host", "device"):
            raise ValueError("rng must be 'numpy', 'numpy-host' or 'device'")
        H, W = int(self.camera.screen_height), int(self.camera.screen_width)
        if _hybrid.is_hybrid(self):
            # user Collider / Material / texture / Light subclasses: the reference's recursion driven
            # from the host, the built-in steps on the device (_hybrid.py); numpy's stream as the
            # reference draws it
            from .utils.colour_functions import sRGB_linear_to_sRGB

            lin = _hybrid.render_linear(self, samples_per_pixel)
            color = sRGB_linear_to_sRGB(lin.to_array())
            u8 = [(255 * np.clip(c, 0, 1).reshape((H, W))).astype(np.uint8) for c in color]
            print("Render Took", time.time() - t0)
            return Image.fromarray(np.stack(u8, axis=-1), "RGB")
        ndev = len(B.devices())
        if ndev > 1 and rng != "numpy-host" and H >= 8 * ndev:
            out = B.render_group(self, samples_per_pixel, seed=seed, batch_size=batch_size, want_rgb=False,
                                 mt=(rng == "numpy"))
        else:
            jitter = None
            if rng == "numpy-host":
                jitter = self.camera.draw_jitter(samples_per_pixel)
                self.camera.draw_jitter(1)  # reference draws one more get_ray for sizing (scene.py:81)
            # only the uint8 image leaves the GPU (the linear RGB stays there: 8x fewer PCIe bytes), as
            # 4-byte pixels -- PIL's layout of an RGB image -- into pinned memory of the image's own,
            # which the returned image maps (no host copy)
            blk = B.image_block(4 * W * H)
            out = B.render_scene(self, samples_per_pixel, jitter=jitter, seed=seed, batch_size=batch_size,
                                 want_rgb=False, mt=(rng == "numpy"), pinned_u8=True, rgbx=True, out_u8=blk)
            self.last_stats = out.stats
            print("Render Took", time.time() - t0)
            return B.rgb_image(out.srgb8, W, H, mapped=blk is not None)
        self.last_stats = out.stats
        print("Render Took", time.time() - t0)
        return Image.fromarray(out.srgb8, "RGB")

    def _render_denoised(self, samples_per_pixel, batch_size, rng, seed, params):
        """render(denoise=...): the frame as render() traces it with the linear RGB kept, the guide
        images, the filter; the image is the filter's own resolve (srt_denoise out_srgb8)."""
        from . import _backend as B
        from . import _hybrid

        if rng not in ("numpy", "numpy-host", "device"):
            raise ValueError("rng must be 'numpy', 'numpy-host' or 'device'")
        if _hybrid.is_hybrid(self):
            raise NotImplementedError("denoise: a scene with user Collider / Material / texture / Light subclasses "
                                      "is shaded through the host; its guide images are not computed on the device")
        print("Rendering...")
        t0 = time.time()
        H, W = int(self.camera.screen_height), int(self.camera.screen_width)
        ndev = len(B.devices())
        ctx = None
        if ndev > 1 and rng != "numpy-host" and H >= 8 * ndev:
            # the gathered frame is filtered on the group's first GPU
            out = B.render_group(self, samples_per_pixel, seed=seed, batch_size=batch_size, want_rgb=True,
                                 mt=(rng == "numpy"))
            import ctypes

            ctx = ctypes.c_void_p(B.group()[1][0])
        else:
            jitter = None
            if rng == "numpy-host":
                jitter = self.camera.draw_jitter(samples_per_pixel)
                self.camera.draw_jitter(1)  # reference draws one more get_ray for sizing (scene.py:81)
            out = B.render_scene(self, samples_per_pixel, jitter=jitter, seed=seed, batch_size=batch_size,
                                 want_rgb=True, mt=(rng == "numpy"))
        aovs = B.render_aovs(self, ctx=ctx)
        blk = B.image_block(4 * W * H)
        ms = []
        _, u8 = B.denoise(out.rgb, aovs, W, H, rgbx=True, out_u8=blk, timings=ms, ctx=ctx, **params)
        self.last_stats = dict(out.stats, denoise=dict(params, ms_aov_kernel=aovs["ms_kernel"], ms_levels=ms[:-1],
                                                            ms_filter=ms[-1]))
        print("Render Took", time.time() - t0)
        return B.rgb_image(u8, W, H, mapped=blk is not None)

    def _render_denoised_halves(self, samples_per_pixel, batch_size, rng, seed, params):
        """render(denoise={"variance" / "demodulate" / "temporal": True, ...}): the frame as two half-frames
        (_backend.render_halves), the guide images, with `temporal` srt_temporal_accumulate against the scene's
        history, and srt_denoise_var, all in device memory of the context; the image is the filter's own resolve
        into the pinned image block."""
        from . import _backend as B
        from . import _hybrid

        if rng not in ("numpy", "numpy-host", "device"):
            raise ValueError("rng must be 'numpy', 'numpy-host' or 'device'")
        if int(samples_per_pixel) < 2:
            raise ValueError("denoise: variance / demodulate / temporal split the frame into two half-frames and need "
                             "samples_per_pixel >= 2, not %r" % (samples_per_pixel,))
        if _hybrid.is_hybrid(self):
            raise NotImplementedError("denoise: a scene with user Collider / Material / texture / Light subclasses "
                                      "is shaded through the host; its guide images are not computed on the device")
        if len(B.devices()) > 1:
            raise NotImplementedError("denoise: variance / demodulate / temporal render on one GPU; %d are selected "
                                      "($SIGHTPY_DEVICES)" % len(B.devices()))
        print("Rendering...")
        t0 = time.time()
        H, W = int(self.camera.screen_height), int(self.camera.screen_width)
        temporal = params.get("temporal", False)
        motion = params.get("motion", False)
        filt = {k: v for k, v in params.items() if k not in B.N.TEMPORAL_DEFAULTS and k != "motion"}
        extra = {}
        with B.DeviceArrays() as pool:
            A, Bh, ka, kb, stats = B.render_halves(self, samples_per_pixel, rng=rng, seed=seed, batch_size=batch_size,
                                                   pool=pool)
            aovs = B.render_aovs_device(self, pool, hit_id=temporal)
            if temporal:
                # the half-frames are accumulated in place against this scene's history before the filter sees them
                if self._history is None:
                    self._history = B.TemporalHistory()
                mt = []
                rows = self._history.accumulate(A, Bh, aovs, B.camera_desc(self.camera), W, H,
                                                demodulate=params["demodulate"], timings=mt, colliders=aovs["colliders"],
                                                motion=motion, posed=aovs.get("posed", ()),
                                                max_history=params["max_history"],
                                                normal_max=params["temporal_normal"], plane_max=params["temporal_plane"])
                extra["ms_temporal"] = mt[0]
                if motion:
                    # rows of the motion table that moved, and that no rigid motion explains (0, 0 without a table)
                    extra["motion_moved"], extra["motion_unknown"] = rows
            blk = B.image_block(4 * W * H)
            ms = []
            _, _, u8 = B.denoise_var(A, Bh, ka, kb, aovs, W, H, want_rgb=False, rgbx=True, out_u8=blk, timings=ms,
                                     **filt)
        self.last_stats = dict(stats, denoise=dict(params, ka=ka, kb=kb, ms_aov_kernel=aovs["ms_kernel"],
                                                   ms_levels=ms[:-2], ms_filter=ms[-2], ms_prepare=ms[-1], **extra))
        print("Render Took", time.time() - t0)
        return B.rgb_image(u8, W, H, mapped=blk is not None)

    def reset_history(self):
        """Drop the temporal history of render(denoise={"temporal": True}): the next such frame starts anew."""
        if self._history is not None:
            self._history.reset()

    def get_aovs(self):
        """The first-hit guide images a denoiser needs (no reference counterpart), computed on the GPU
        from one pixel-centre pinhole ray per pixel -- no random numbers are drawn: a dict of
        "hit_id" (n,) int32 (index into collider_list, -1 = nothing hit), "depth" (n,) (1e39 = nothing
        hit), "position", "normal" and "albedo" (3, n), n = screen_width * screen_height, row-major.
        Pixels that see the background have normal, albedo and position (0, 0, 0)."""
        from . import _backend as B
        from . import _hybrid

        if _hybrid.is_hybrid(self):
            raise NotImplementedError("get_aovs: a scene with user Collider / Material / texture / Light subclasses "
                                      "is shaded through the host; its guide images are not computed on the device")
        aovs = B.render_aovs(self)
        aovs.pop("ms_kernel")
        return aovs

    def get_distances(self):
        """Grey depth map of one primary sample (reference scene.py:142-166)."""
        from ._backend import primary_rays, nearest_hits

        print("Rendering...")
        t0 = time.time()
        from . import _hybrid

        jitter = self.camera.draw_jitter(1)[0]
        O, D = primary_rays(self.camera, jitter)
        if _hybrid.is_hybrid(self):
            from .ray import Ray

            t = _hybrid.nearest_distance(Ray(vec3(*O), vec3(*D), 0, self.n, 0, 0, 0), self)
        else:
            t, _, _ = nearest_hits(self, O, D)
        g = np.where(t <= 10, t, 10) / 10
        print("Render Took", time.time() - t0)
        h, w = self.camera.screen_height, self.camera.screen_width
        u8 = (255 * np.clip(g, 0, 1).reshape((h, w))).astype(np.uint8)
        return Image.fromarray(np.stack([u8, u8, u8], axis=-1), "RGB")


def get_raycolor_tuple(x):
    """Reference scene.py:16-17 (Pool worker shim); kept for API compatibility."""
    from .ray import get_raycolor

    return get_raycolor(*x)


def batch_rays(rays, batch_size):
    """Reference scene.py:20-25: concatenate per-sample Ray batches in groups of batch_size."""
    from .ray import Ray

    return [Ray.concatenate(rays[i:i + batch_size]) for i in range(0, len(rays), batch_size)]
