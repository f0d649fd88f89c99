"""Device backend: one libsightpy_hip.so context per process, scene upload cache, entry points used
by the public API (Scene.render, get_raycolor, get_distances, Collider.intersect, Camera.get_ray).

There is deliberately no CPU path here: if the HIP library or a GPU is missing every entry point
raises `BackendUnavailable`.
"""
import ctypes
import os

import numpy as np

from . import _native as N
from ._lower import lower_scene, camera_desc, collider_record, POSE_IDENTITY
from ._motion import collider_motion, count_rows, pose_motion
from .utils.vector3 import vec3

_STATE = {"lib": None, "ctx": None, "device": None, "resident": {}, "buffers": {}, "pinned": {}, "group": None}
# how often upload() called srt_upload_scene, srt_pose_colliders and srt_deform_colliders
_STATE.update({"uploads": 0, "pose_calls": 0, "deform_calls": 0})


class Resident:
    """What upload() knows to be resident in one context (_STATE["resident"], by the context's address)."""

    def __init__(self):
        self.forget()
        self.per_hit_inputs = False  # the scene is shaded with per-hit inputs (a user texture / Light, _hybrid.py)

    def forget(self):
        """Nothing is known to be resident (per_hit_inputs stays until an upload sets it)."""
        self.scene = None      # Lowered.signature() of the uploaded tables
        self.poses = ()        # _pose_sig() of the poses of the device-posed meshes (TriangleMesh.set_pose)
        self.verts = {}        # {(first, count): (mesh key, version)} of the ranges not in their loaded shape
        self.topology = set()  # the ranges registered with srt_deform_topology since the upload


def resident(ctx):
    """The residency record of `ctx`."""
    return _STATE["resident"].setdefault(_addr(ctx), Resident())


def forget_resident(ctx=None):
    """Forget what is resident in `ctx` (default: in every context): the next upload() there uploads."""
    for res in _STATE["resident"].values() if ctx is None else [resident(ctx)]:
        res.forget()


class RenderResult:
    def __init__(self, srgb8, rgb, hit_ids, stats):
        self.srgb8 = srgb8
        self.rgb = rgb
        self.hit_ids = hit_ids
        self.stats = stats


def library():
    if _STATE["lib"] is None:
        _STATE["lib"] = N.load_library()
    return _STATE["lib"]


def _env_options(lib, ctx):
    """Options every context of this process takes from the environment (the process context and
    the contexts of a multi-GPU group alike)."""
    if os.environ.get("SIGHTPY_FRAME_KERNEL") is not None:  # A/B switch: 0 = per-depth wavefront kernels
        N.check(lib, lib.srt_set_option(ctx, b"frame_kernel", int(os.environ["SIGHTPY_FRAME_KERNEL"])))
    if os.environ.get("SIGHTPY_DETERMINISTIC") is not None:  # 0: f64 atomics instead of fixed-point sums
        N.check(lib, lib.srt_set_option(ctx, b"deterministic", int(os.environ["SIGHTPY_DETERMINISTIC"])))
    # any library option: SIGHTPY_OPTIONS="key=value,key=value" (srt_set_option; e.g. A/B runs of the
    # whole test suite on another generator or kernel strategy)
    for kv in os.environ.get("SIGHTPY_OPTIONS", "").split(","):
        if kv.strip():
            k, v = kv.split("=")
            N.check(lib, lib.srt_set_option(ctx, k.strip().encode(), int(v)))


def _device_spec():
    """$SIGHTPY_DEVICES as a list of ints, or None (unset / empty / "all")."""
    spec = os.environ.get("SIGHTPY_DEVICES", "").strip()
    if not spec or spec == "all":
        return None
    return [int(v) for v in spec.split(",") if v.strip()]


def context():
    """The process's device context: device = $SIGHTPY_DEVICE, else a one-entry $SIGHTPY_DEVICES,
    else $LOCAL_RANK, else 0."""
    if _STATE["ctx"] is None:
        lib = library()
        n = ctypes.c_int(0)
        rc = lib.srt_device_count(ctypes.byref(n))
        if rc != 0 or n.value < 1:
            raise N.BackendUnavailable(
                "no HIP device visible (%s); sightpy on MI355X has no CPU fallback"
                % lib.srt_last_error().decode(errors="replace")
            )
        spec = _device_spec()
        if os.environ.get("SIGHTPY_DEVICE") is not None:
            dev = int(os.environ["SIGHTPY_DEVICE"])
        elif spec is not None and len(spec) == 1:
            dev = spec[0]
        else:
            dev = int(os.environ.get("LOCAL_RANK", "0"))
        if not 0 <= dev < n.value:
            raise ValueError("sightpy: device %d requested, %d visible" % (dev, n.value))
        ctx = ctypes.c_void_p()
        N.check(lib, lib.srt_create(dev, ctypes.byref(ctx)))
        _env_options(lib, ctx)
        _STATE["ctx"] = ctx
        _STATE["device"] = dev
    return _STATE["lib"], _STATE["ctx"]


def devices():
    """GPUs Scene.render uses: $SIGHTPY_DEVICES ("0,1,2,3" or "all"), else the one context device
    ($SIGHTPY_DEVICE, else $LOCAL_RANK, else 0)."""
    spec = os.environ.get("SIGHTPY_DEVICES", "").strip()
    if not spec:
        return [int(os.environ.get("SIGHTPY_DEVICE", os.environ.get("LOCAL_RANK", "0")))]
    if spec == "all":
        n = ctypes.c_int(0)
        N.check(library(), library().srt_device_count(ctypes.byref(n)))
        return list(range(n.value))
    return _device_spec()


def group():
    """Contexts of the multi-GPU group over devices() (srt_comm_init_all: one RCCL communicator in
    this process, rank q on devices()[q]), created once."""
    devs = devices()
    g = _STATE["group"]
    if g is not None and g[0] == devs:
        return library(), g[1]
    lib = library()
    arr = (ctypes.c_int * len(devs))(*devs)
    ctxs = (ctypes.c_void_p * len(devs))()
    N.check(lib, lib.srt_comm_init_all(len(devs), arr, ctxs))
    for q in range(len(devs)):
        _env_options(lib, ctypes.c_void_p(ctxs[q]))
    _STATE["group"] = (devs, ctxs)
    return lib, ctxs


def _pose_sig(posed, identity=False):
    """What srt_pose_colliders would be called with for a Lowered's `posed` list, as a comparable value."""
    return tuple((p["first"], p["count"], (POSE_IDENTITY if identity else p["pose"]).tobytes()) for p in posed)


def _vert_version(p):
    """The vertex array a Lowered.posed entry wants resident, as a comparable value; None: the loaded shape."""
    return None if p.get("deform") is None else (p["key"], p["vver"])


def plan_upload(res, L, force=False):
    """The library calls that make the Lowered `L` resident where the record `res` (a Resident) is, in order:
    ("upload", signature), ("topology", range) per range, ("deform", [range, ...]), ("pose",).  Reads `res`,
    changes nothing and calls nothing.  The poses of device-posed meshes are no part of the tables and are compared on their own:
    when only they changed, the plan is one pose call.  Neither are the vertex arrays of deformed meshes
    (TriangleMesh.set_vertices): when the version resident for a mesh is not the one wanted, a deform call for
    those meshes (their topology registered first, once per upload), which leaves them in the identity pose, so a
    pose call follows if any pose is another."""
    want, identity = _pose_sig(L.posed), _pose_sig(L.posed, identity=True)
    wanted = {(p["first"], p["count"]): _vert_version(p) for p in L.posed if p.get("deform") is not None}
    verts, topology, poses = res.verts, res.topology, res.poses
    steps = []
    # a deformed range resident that no deformed mesh of this scene claims: the tables are another shape's than the
    # signature says (the mesh went back to its loaded shape without an array to restore it from -- invalidate() --
    # or this is another scene with the same tables, a fresh Scene of the same OBJ for one): only an upload restores it
    sig = L.signature()
    if force or set(verts) - set(wanted) or sig != res.scene:
        steps.append(("upload", sig))
        verts, topology, poses = {}, set(), identity  # (every mesh in its rest pose, at its loaded vertices)
    changed = [rng for rng, version in wanted.items() if verts.get(rng) != version]
    if changed:
        steps += [("topology", rng) for rng in changed if rng not in topology]
        steps.append(("deform", changed))
        if want != identity:
            poses = ()  # (the deformed ranges are back in the identity pose)
    if want != poses:
        steps.append(("pose",))
    return steps


def upload(scene, extra_media=(), force=False, ctx=None):
    """Lower `scene` and make it resident in `ctx` (default: the process context) by the calls of plan_upload():
    none when the identical tables, poses and vertices are already there (_STATE["uploads"], ["pose_calls"] and
    ["deform_calls"] count the calls of each kind).  What a call is about to rewrite is forgotten before it and
    recorded after it returned success, so after a call that raised the next upload() makes it again."""
    lib = library()
    if ctx is None:
        ctx = context()[1]
    L = lower_scene(scene, extra_media)
    want, identity = _pose_sig(L.posed), _pose_sig(L.posed, identity=True)
    if want != identity and len(devices()) > 1:
        raise NotImplementedError("a posed TriangleMesh (set_pose) renders on one GPU; %d are selected "
                                  "($SIGHTPY_DEVICES)" % len(devices()))
    if any(p.get("deform") is not None for p in L.posed) and len(devices()) > 1:
        raise NotImplementedError("a deformed TriangleMesh (set_vertices) renders on one GPU; %d are selected "
                                  "($SIGHTPY_DEVICES)" % len(devices()))
    res = resident(ctx)
    by_range = {(p["first"], p["count"]): p for p in L.posed}
    for step in plan_upload(res, L, force):
        if step[0] == "upload":
            res.forget()
            N.check(lib, lib.srt_upload_scene(ctx, ctypes.byref(L.desc())))
            _STATE["uploads"] += 1
            res.scene, res.poses = step[1], identity
            # the library refuses every whole-frame entry point on such a scene, srt_render_prefetch included
            res.per_hit_inputs = bool((L.materials["flags"] & N.MF_HIT_ALBEDO).any()
                                      or (L.lights["type"] == N.LIGHT_USER).any())
        elif step[0] == "topology":
            rng, d = step[1], by_range[step[1]]["deform"]
            corners = np.ascontiguousarray(d["corners"], dtype=np.int32)
            flags = np.ascontiguousarray(d["recompute"], dtype=np.uint8)
            center = np.ascontiguousarray(d["center"], dtype=np.float64)
            N.check(lib, lib.srt_deform_topology(ctx, rng[0], rng[1], len(d["verts"]), N.ptr(corners), N.ptr(center),
                                                 N.ptr(flags)))
            res.topology.add(rng)
        elif step[0] == "deform":
            for rng in step[1]:
                res.verts.pop(rng, None)
            first, count = (np.array(v, dtype=np.int32) for v in zip(*step[1]))
            verts = [np.ascontiguousarray(by_range[rng]["deform"]["verts"], dtype=np.float64) for rng in step[1]]
            ptrs = (ctypes.c_void_p * len(verts))(*[N.ptr(v) for v in verts])
            N.check(lib, lib.srt_deform_colliders(ctx, len(first), N.ptr(first), N.ptr(count), ptrs))
            _STATE["deform_calls"] += 1
            for rng in step[1]:
                res.verts[rng] = _vert_version(by_range[rng])
            if want != identity:
                res.poses = ()  # (the deformed ranges are back in the identity pose)
        else:
            res.poses = ()
            first = np.array([p["first"] for p in L.posed], dtype=np.int32)
            count = np.array([p["count"] for p in L.posed], dtype=np.int32)
            poses = np.ascontiguousarray([p["pose"] for p in L.posed], dtype=np.float64)
            N.check(lib, lib.srt_pose_colliders(ctx, len(first), N.ptr(first), N.ptr(count), N.ptr(poses)))
            _STATE["pose_calls"] += 1
            res.poses = want
    return L


def pinned_buffer(name, nbytes):
    """A named pinned host allocation of the context (srt_host_alloc), grown on demand and kept across
    calls, as a uint8 numpy array: the device copies into it at full PCIe rate (a pageable destination
    goes through the runtime's staging copies)."""
    lib, ctx = context()
    cur = _STATE["pinned"].get(name)
    if cur is None or cur[1] < nbytes:
        if cur is not None:
            N.check(lib, lib.srt_host_free(ctx, cur[0]))
            del _STATE["pinned"][name]
        p = ctypes.c_void_p()
        N.check(lib, lib.srt_host_alloc(ctx, max(int(nbytes), 8), ctypes.byref(p)))
        cur = (p, int(nbytes))
        _STATE["pinned"][name] = cur
    return np.ctypeslib.as_array(ctypes.cast(cur[0], ctypes.POINTER(ctypes.c_uint8)), (cur[1],))[:nbytes]


class _HostBlock:
    """A pinned host allocation of the context lent to numpy as the base of one array (and through it
    to a PIL image mapping that array): when the last of them is gone the allocation goes back to a
    small pool for the next image (image_block)."""

    __slots__ = ("ptr", "nbytes")

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes

    @property
    def __array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            _STATE["blocks_out"] -= 1
            if _STATE["ctx"] is None:
                return
            if sum(len(v) for v in _STATE["blocks"].values()) < _BLOCKS_FREE_MAX:
                _STATE["blocks"].setdefault(self.nbytes, []).append(self.ptr)
            else:
                _STATE["lib"].srt_host_free(_STATE["ctx"], ctypes.c_void_p(self.ptr))
        except Exception:  # (interpreter shutdown: the process frees it)
            pass


_STATE["blocks"] = {}      # nbytes -> free pinned allocations (pointers), _BLOCKS_FREE_MAX in all
_STATE["blocks_out"] = 0   # allocations lent to live arrays
_BLOCKS_FREE_MAX = 4
_BLOCKS_OUT_MAX = 16


def image_block(nbytes):
    """A uint8 array of `nbytes` in pinned host memory of its own, for an output that outlives the call
    (Scene.render's image maps it: the device copies the frame into it at full PCIe rate and PIL takes
    it without a copy), or None when _BLOCKS_OUT_MAX such arrays are alive already (the caller then
    copies out of the shared pinned buffer)."""
    lib, ctx = context()
    if _STATE["blocks_out"] >= _BLOCKS_OUT_MAX:
        return None
    free = _STATE["blocks"].get(nbytes)
    if free:
        ptr = free.pop()
    else:
        p = ctypes.c_void_p()
        N.check(lib, lib.srt_host_alloc(ctx, max(int(nbytes), 8), ctypes.byref(p)))
        ptr = p.value
    _STATE["blocks_out"] += 1
    return np.asarray(_HostBlock(ptr, int(nbytes)))


def rgb_image(rgbx, width, height, mapped):
    """PIL RGB image of 4-byte pixels (R, G, B, 255: PIL's own layout of mode RGB).  `mapped`: the image
    maps `rgbx` (which it keeps alive; read-only, so PIL copies it before any change), else the pixels
    are copied into a new image.  Either way the image equals Image.fromarray(rgbx[..., :3], "RGB")."""
    from PIL import Image

    if mapped:
        try:
            im = Image.frombuffer("RGBX", (width, height), rgbx, "raw", "RGBX", 0, 1)
            core = im.im
            core.setmode("RGB")
            img = im._new(core)
            img.readonly = 1
            if img.mode == "RGB" and img.size == (width, height):
                return img
        except Exception:  # (a Pillow without these internals: the copy below)
            pass
    img = Image.new("RGB", (width, height), None)
    img.frombytes(rgbx, "raw", "RGBX")
    return img


def device_buffer(name, nbytes):
    """A named device allocation of the context, grown on demand (kept across calls)."""
    lib, ctx = context()
    cur = _STATE["buffers"].get(name)
    if cur is not None and cur[1] >= nbytes:
        return cur[0]
    if cur is not None:
        N.check(lib, lib.srt_device_free(ctx, cur[0]))
        del _STATE["buffers"][name]
    p = ctypes.c_void_p()
    N.check(lib, lib.srt_device_alloc(ctx, max(int(nbytes), 8), ctypes.byref(p)))
    _STATE["buffers"][name] = (p, int(nbytes))
    return p


def release_buffer(name):
    """Free a named device allocation of the context."""
    cur = _STATE["buffers"].pop(name, None)
    if cur is not None:
        lib, ctx = context()
        N.check(lib, lib.srt_device_free(ctx, cur[0]))


def _addr(p):
    """The address in a ctypes pointer or an int."""
    return p.value if isinstance(p, ctypes.c_void_p) else int(p)


class DeviceArrays:
    """Device allocations of a context for the length of a `with` block (srt_device_alloc), freed at its end on
    every path."""

    def __init__(self, ctx=None):
        self.lib = library()
        self.ctx = context()[1] if ctx is None else ctx
        self.ptrs = []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        N.check(self.lib, self.lib.srt_device_alloc(self.ctx, max(int(nbytes), 8), ctypes.byref(p)))
        self.ptrs.append(p)
        return p

    def doubles(self, count):
        return self.alloc(8 * int(count))

    def fetch(self, p, shape, dtype=np.float64):
        """A host copy of the device array at `p`."""
        out = np.empty(shape, dtype=dtype)
        N.check(self.lib, self.lib.srt_memcpy(self.ctx, N.ptr(out), p, out.nbytes))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        ptrs, self.ptrs = self.ptrs, []
        for p in ptrs:
            self.lib.srt_device_free(self.ctx, p)
        return False


def numpy_uniforms(n_out, n_skip=0, out=None):
    """`np.random.rand(n_out)` computed on the GPU (then `n_skip` more draws), advancing numpy's
    global RandomState exactly as the host draws would (srt_mt19937_uniforms).

    Returns the doubles in a device buffer (a ctypes pointer, valid until the next call) when `out`
    is None, else writes the host array `out`."""
    lib, ctx = context()
    name, key, pos, has_gauss, gauss = np.random.get_state()
    if name != "MT19937":
        raise ValueError("numpy's global generator is not MT19937")
    key = np.ascontiguousarray(key, dtype=np.uint32)
    if out is None:
        release_buffer("uniforms")  # sized per call, not kept at the largest request ever made
    dst = device_buffer("uniforms", 8 * n_out) if out is None else N.ptr(out)
    key_out = np.empty(624, dtype=np.uint32)
    pos_out = ctypes.c_int32(0)
    N.check(lib, lib.srt_mt19937_uniforms(ctx, N.ptr(key), int(pos), int(n_out), int(n_skip), dst, N.ptr(key_out),
                                          ctypes.byref(pos_out)))
    np.random.set_state((name, key_out, pos_out.value, has_gauss, gauss))
    return dst


def _planar(v, n=None):
    """vec3 (scalars or arrays) -> C-contiguous float64 (3, n)."""
    comps = [np.asarray(c, dtype=np.float64) for c in (v.x, v.y, v.z)]
    if n is None:
        n = max([c.size for c in comps])
    return np.ascontiguousarray(np.stack([np.broadcast_to(c.reshape(-1) if c.ndim else c, (n,)) for c in comps]))


def _default_seed():
    """Seed for the device RNG derived from numpy's global RNG state WITHOUT consuming it (the
    reference's render consumes only the camera draws from the parent's stream)."""
    key, pos = np.random.get_state()[1:3]
    return (int(key[pos % 624]) << 32 | int(key[(pos + 397) % 624])) ^ (int(pos) * 0x9E3779B97F4A7C15) & (2**64 - 1)


def render_scene(scene, spp, jitter=None, seed=None, batch_size=None, rows=None, want_rgb=True, want_hits=False,
                 jitter_device=None, mt=False, pinned_u8=False, rgbx=False, prefetch=None, out_u8=None,
                 sample_base=0, rgb_device=None, want_u8=True):
    """Scene.render on the device.  `jitter` (spp, 4, H*W) from numpy or None for the device RNG;
    `jitter_device`: the same uniforms already in device memory (numpy_uniforms); `mt=True`: the
    jitter is numpy's global stream generated on the device (the reference's draws, including the
    sizing draw of scene.py:81), and numpy's global state is advanced past it.  `pinned_u8`: the
    uint8 image lands in the context's pinned host buffer (a view, valid until the next such call)
    instead of a new array.  Without `want_rgb` the linear RGB is resolved and kept in HBM
    (SRT_RENDER_RGB_LOCAL), as the reference keeps it internal.  `rgbx`: the image as 4-byte pixels
    (R, G, B, 255; SRT_RENDER_RGBX), srgb8 of shape (rows, W, 4).  `prefetch` (whole frames with
    `mt`): the jitter's generation is queued on the GPU (srt_render_prefetch) before the scene is
    lowered and uploaded, so the two overlap (default on; $SIGHTPY_PREFETCH=0 turns it off).
    `out_u8`: a host uint8 array of the image's size to write the image into (image_block).
    `sample_base`: the frame's index of this call's first sample (its samples are sample_base .. sample_base +
    spp - 1 of a longer frame: their Monte-Carlo keys and device-RNG jitter; `jitter` / `jitter_device` hold this
    call's samples only).  `rgb_device`: a device pointer (3 * npix doubles) that receives the linear RGB in place
    of a host array (result.rgb is None); `want_u8=False`: no uint8 image (result.srgb8 is None)."""
    lib, ctx = context()
    if prefetch is None:
        prefetch = os.environ.get("SIGHTPY_PREFETCH", "1") != "0"
    cam = scene.camera
    W, H = int(cam.screen_width), int(cam.screen_height)
    rows_arr = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    nrows = H if rows_arr is None else len(rows_arr)
    npix = nrows * W
    cd = camera_desc(cam)
    a = N.RenderArgs()
    a.spp = int(spp)
    a.sample_base = int(sample_base)
    a.n_rows = nrows
    a.batch_spp = int(batch_size or 0)
    a.rows = N.ptr(rows_arr)
    j = None
    if jitter_device is not None:
        a.jitter = _addr(jitter_device)
    elif jitter is not None:
        j = np.ascontiguousarray(jitter, dtype=np.float64)
        if j.shape != (spp, 4, npix):
            raise ValueError("jitter must have shape (spp, 4, %d)" % npix)
        a.jitter = N.ptr(j)
    a.seed = int(seed if seed is not None else _default_seed()) & (2**64 - 1)
    state = None
    if mt:
        if j is not None or jitter_device is not None:
            raise ValueError("mt=True draws the jitter itself")
        state = N.MtState.from_numpy()
        a.mt = ctypes.pointer(state)
    if rgb_device is not None:
        want_rgb = True
    a.flags = (0 if want_rgb else N.RENDER_RGB_LOCAL) | (N.RENDER_RGBX if rgbx else 0)
    # (the prefetch runs before this frame's scene replaces the resident one: not while that one is a
    # per-hit-inputs scene, on which the library refuses it)
    if mt and prefetch and rows_arr is None and nrows == H and not resident(ctx).per_hit_inputs:
        N.check(lib, lib.srt_render_prefetch(ctx, ctypes.byref(cd), ctypes.byref(a)))
    upload(scene)
    rgb = np.empty((3, npix)) if want_rgb and rgb_device is None else None
    ch = 4 if rgbx else 3
    if not want_u8:
        u8 = None
    elif out_u8 is not None:
        if out_u8.dtype != np.uint8 or out_u8.size != ch * npix or not out_u8.flags.c_contiguous:
            raise ValueError("out_u8 must be a contiguous uint8 array of %d bytes" % (ch * npix))
        u8 = out_u8.reshape(npix, ch)
    else:
        u8 = (pinned_buffer("render_u8", ch * npix) if pinned_u8 else np.empty(ch * npix, dtype=np.uint8)).reshape(npix, ch)
    hits = np.empty((spp, npix), dtype=np.int32) if want_hits else None
    a.out_rgb = N.ptr(rgb) if rgb_device is None else _addr(rgb_device)
    a.out_srgb8 = N.ptr(u8)
    a.out_hit_id = N.ptr(hits)
    st = N.Stats()
    N.check(lib, lib.srt_render(ctx, ctypes.byref(cd), ctypes.byref(a), ctypes.byref(st)))
    if state is not None:
        state.to_numpy()
    return RenderResult(None if u8 is None else u8.reshape(nrows, W, ch), rgb, hits, st.as_dict())


def render_group(scene, spp, seed=None, batch_size=None, want_rgb=True, mt=True):
    """Scene.render on every GPU of devices(): each renders its row bands (SRT_RENDER_SHARDED; at
    most shard_kmax bands per GPU, rt_device.h shard_band_height: 27 rows at 1080p on 8 GPUs) and
    the tiles are gathered to the first over RCCL (srt_render_group).  `mt`: numpy's stream as in
    render_scene (else the device RNG)."""
    lib, ctxs = group()
    for q in range(len(ctxs)):
        upload(scene, ctx=ctypes.c_void_p(ctxs[q]))
    cam = scene.camera
    W, H = int(cam.screen_width), int(cam.screen_height)
    cd = camera_desc(cam)
    a = N.RenderArgs()
    a.spp, a.sample_base, a.n_rows, a.batch_spp = int(spp), 0, H, int(batch_size or 0)
    a.seed = int(seed if seed is not None else _default_seed()) & (2**64 - 1)
    state = None
    if mt:
        state = N.MtState.from_numpy()
        a.mt = ctypes.pointer(state)
    rgb = np.empty((3, W * H)) if want_rgb else None
    u8 = np.empty((W * H, 3), dtype=np.uint8)
    a.out_rgb, a.out_srgb8 = N.ptr(rgb), N.ptr(u8)
    a.flags = 0 if want_rgb else N.RENDER_RGB_LOCAL  # (every GPU keeps its rows of the linear RGB)
    st = N.Stats()
    N.check(lib, lib.srt_render_group(ctxs, len(ctxs), ctypes.byref(cd), ctypes.byref(a), ctypes.byref(st)))
    if state is not None:
        state.to_numpy()
    return RenderResult(u8.reshape(H, W, 3), rgb, None, st.as_dict())


def _media_of(ray_n, count):
    """Per-ray complex IOR triples -> (unique triples, index per ray)."""
    comps = [np.asarray(c) for c in (ray_n.x, ray_n.y, ray_n.z)]
    cols = [np.broadcast_to(c.astype(np.complex128), (count,)) for c in comps]
    tri = np.stack(cols, axis=1)
    uniq, inv = np.unique(tri, axis=0, return_inverse=True)
    return [tuple(complex(v) for v in row) for row in uniq], inv.reshape(-1).astype(np.int32)


def trace_rays(ray, scene, seed=None, return_stats=False, hits=None):
    """get_raycolor(ray, scene) on the device: colour of every ray of the batch.  `hits`:
    (collider index per ray, distance, orientation) -- Material.get_color at those hits
    (srt_shade) instead of the nearest-hit search of the first depth."""
    lib, ctx = context()
    n = len(ray)
    uniq, inv = _media_of(ray.n, n)
    L = upload(scene, extra_media=uniq)
    remap = np.array([L.media_keys.index(k) for k in uniq], dtype=np.int32)
    med = np.ascontiguousarray(remap[inv])
    O = _planar(ray.origin, n)
    D = _planar(ray.dir, n)
    out = np.empty((3, n))
    a = N.TraceArgs()
    a.n = n
    a.origin, a.dir, a.medium = N.ptr(O), N.ptr(D), N.ptr(med)
    a.depth = int(ray.depth)
    a.diffuse_reflections = int(ray.diffuse_reflections)
    a.seed = int(seed if seed is not None else _default_seed()) & (2**64 - 1)
    a.out_rgb = N.ptr(out)
    st = N.Stats()
    if hits is None:
        N.check(lib, lib.srt_trace(ctx, ctypes.byref(a), ctypes.byref(st)))
    else:
        ids = np.ascontiguousarray(np.broadcast_to(np.asarray(hits[0], dtype=np.int32), (n,)))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(hits[1], dtype=np.float64), (n,)))
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(hits[2], dtype=np.float64), (n,)))
        N.check(lib, lib.srt_shade(ctx, ctypes.byref(a), N.ptr(ids), N.ptr(t), N.ptr(o), ctypes.byref(st)))
    col = vec3(out[0], out[1], out[2])
    return (col, st.as_dict()) if return_stats else col


def nearest_hits(scene, O, D):
    """Nearest hit over scene.collider_list: (t, collider index or -1, orientation)."""
    lib, ctx = context()
    upload(scene)
    Oa = _planar(O)
    n = Oa.shape[1]
    Da = _planar(D, n)
    t = np.empty(n)
    ids = np.empty(n, dtype=np.int32)
    orient = np.empty(n)
    N.check(lib, lib.srt_nearest(ctx, N.ptr(Oa), N.ptr(Da), n, N.ptr(t), N.ptr(ids), N.ptr(orient)))
    return t, ids, orient


def intersect_collider(collider, O, D):
    """Collider.intersect(O, D) -> (2, N) [distance; orientation] on the device."""
    lib, ctx = context()
    rec = np.ascontiguousarray(collider_record(collider))
    Oa = _planar(O)
    n = Oa.shape[1]
    Da = _planar(D, n)
    out = np.empty((2, n))
    N.check(lib, lib.srt_intersect_collider(ctx, N.ptr(rec.reshape(1)), N.ptr(Oa), N.ptr(Da), n, N.ptr(out)))
    return out


def collider_surface(collider, P, normal=True, uv=True, primitive_uv=False):
    """Collider.get_Normal (3, n) and get_uv (2, n) at points P on the device
    (srt_collider_surface); `primitive_uv` applies the owning Cuboid/SkyBox's (4, 3) divide."""
    lib, ctx = context()
    rec = np.ascontiguousarray(collider_record(collider))
    if getattr(getattr(collider, "assigned_primitive", None), "uv_cube_cross", False):
        rec["flags"] |= N.CF_UV_CROSS
    Pa = _planar(P)
    n = Pa.shape[1]
    Nout = np.empty((3, n)) if normal else None
    uvout = np.empty((2, n)) if uv else None
    N.check(lib, lib.srt_collider_surface(ctx, N.ptr(rec.reshape(1)), N.ptr(Pa), n, N.ptr(Nout), N.ptr(uvout),
                                          int(bool(primitive_uv))))
    return Nout, uvout


def material_normal(material, hit):
    """Material.get_Normal(hit) on the device (srt_material_normal): the collider normal, or the
    material's normal map through the collider's inverse_basis_matrix, times hit.orientation (3, n)."""
    from ._lower import texture_record

    lib, ctx = context()
    c = hit.collider
    rec = np.ascontiguousarray(collider_record(c))
    if getattr(getattr(c, "assigned_primitive", None), "uv_cube_cross", False):
        rec["flags"] |= N.CF_UV_CROSS  # (the primitive's uv, as hit.get_uv() takes it)
    Pa = _planar(hit.point)
    n = Pa.shape[1]
    orient = np.ascontiguousarray(np.broadcast_to(np.asarray(hit.orientation, dtype=np.float64).reshape(-1)
                                                  if np.ndim(hit.orientation) else hit.orientation, (n,)))
    tex, texels = None, None
    if material.normalmap is not None:
        if not hasattr(c, "inverse_basis_matrix"):
            raise AttributeError("'%s' object has no attribute 'inverse_basis_matrix'" % type(c).__name__)
        tex, texels = texture_record(material.normalmap_u8, material.repeat, linear=False)
        tex = np.ascontiguousarray(tex).reshape(1)
    out = np.empty((3, n))
    N.check(lib, lib.srt_material_normal(ctx, N.ptr(rec.reshape(1)), N.ptr(tex), N.ptr(texels),
                                         0 if texels is None else texels.size, N.ptr(Pa), N.ptr(orient), n,
                                         N.ptr(out)))
    return out


def texture_lookup(u8, repeat, u, v, linear=True):
    """image.get_color at (u, v) on the device (srt_texture_lookup): rgb (3, n)."""
    from ._lower import texture_record

    lib, ctx = context()
    rec, texels = texture_record(u8, repeat, linear)
    uv = np.ascontiguousarray(np.stack(np.broadcast_arrays(np.asarray(u, dtype=np.float64),
                                                           np.asarray(v, dtype=np.float64))).reshape(2, -1))
    n = uv.shape[1]
    out = np.empty((3, n))
    N.check(lib, lib.srt_texture_lookup(ctx, N.ptr(rec.reshape(1)), N.ptr(texels), texels.size, N.ptr(uv), n,
                                        N.ptr(out)))
    return out


def denoise_params(spec):
    """Scene.render's `denoise` argument -> the filter's parameters (N.DENOISE_DEFAULTS overridden by a
    dict), or None for no denoising.  ValueError for an unknown key or a value srt_denoise would refuse.
    With "variance" or "demodulate" on, the dict also holds N.DENOISE_VAR_DEFAULTS' keys (the half-frame mode,
    srt_denoise_var); otherwise it holds srt_denoise's parameters alone.  With "temporal" on (which selects the
    half-frame mode too) it also holds N.TEMPORAL_DEFAULTS' keys (srt_temporal_accumulate), and "motion": True when
    that key is given as True (per-collider motion, _motion.py; absent otherwise)."""
    if spec is None or spec is False:
        return None
    params = dict(N.DENOISE_DEFAULTS)
    if spec is True:
        return params
    known = sorted(list(params) + list(N.DENOISE_VAR_DEFAULTS) + list(N.TEMPORAL_DEFAULTS) + ["motion"])
    if not isinstance(spec, dict):
        raise ValueError("denoise must be a bool or a dict of %s" % known)
    extra = dict(N.DENOISE_VAR_DEFAULTS)
    temporal = dict(N.TEMPORAL_DEFAULTS)
    motion = False
    for k, v in spec.items():
        if k not in params and k not in extra and k not in temporal and k != "motion":
            raise ValueError("denoise: unknown key %r (known: %s)" % (k, ", ".join(known)))
        if k in ("variance", "demodulate", "temporal", "motion"):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError("denoise: %s must be a bool, not %r" % (k, v))
            if k == "motion":
                motion = bool(v)
            else:
                (temporal if k == "temporal" else extra)[k] = bool(v)
        elif k == "max_history":
            if isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= 2**31 - 1:
                raise ValueError("denoise: max_history must be an integer >= 1, not %r" % (v,))
            temporal[k] = int(v)
        elif k in ("temporal_normal", "temporal_plane"):
            if isinstance(v, bool) or not float(v) >= 0.0 or float(v) == float("inf"):
                raise ValueError("denoise: %s must be a finite number >= 0, not %r" % (k, v))
            temporal[k] = float(v)
        elif k == "sigma_lum":
            if isinstance(v, bool) or not float(v) > 0.0 or float(v) == float("inf"):
                raise ValueError("denoise: %s must be a positive number, not %r" % (k, v))
            extra[k] = float(v)
        elif k == "levels":
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= N.DENOISE_MAX_LEVELS:
                raise ValueError("denoise: levels must be an integer in 0..%d, not %r" % (N.DENOISE_MAX_LEVELS, v))
            params[k] = int(v)
        else:
            if isinstance(v, bool) or not float(v) > 0.0 or float(v) == float("inf"):
                raise ValueError("denoise: %s must be a positive number, not %r" % (k, v))
            params[k] = float(v)
    if extra["variance"] or extra["demodulate"] or temporal["temporal"]:
        params.update(extra)
    if temporal["temporal"]:
        params.update(temporal)
        if motion:
            params["motion"] = True
    return params


def render_aovs(scene, ctx=None):
    """The first-hit guide images of `scene` (srt_render_aovs), one pixel-centre pinhole ray per pixel:
    {"hit_id" (n,) int32, "depth" (n,), "position" / "normal" / "albedo" (3, n), "ms_kernel"}.  Draws
    nothing from numpy's RNG.  `ctx`: another context than the process's (a multi-GPU group's first)."""
    lib = library()
    if ctx is None:
        ctx = context()[1]
    upload(scene, ctx=ctx)
    cd = camera_desc(scene.camera)
    n = int(scene.camera.screen_width) * int(scene.camera.screen_height)
    res = {"hit_id": np.empty(n, dtype=np.int32), "depth": np.empty(n), "position": np.empty((3, n)),
           "normal": np.empty((3, n)), "albedo": np.empty((3, n))}
    out = N.AovOut()
    for k, v in res.items():
        setattr(out, k, N.ptr(v))
    N.check(lib, lib.srt_render_aovs(ctx, ctypes.byref(cd), ctypes.byref(out)))
    res["ms_kernel"] = float(out.ms_kernel)
    return res


def denoise(rgb, aovs, width, height, levels=N.DENOISE_DEFAULTS["levels"],
            sigma_color=N.DENOISE_DEFAULTS["sigma_color"], sigma_normal=N.DENOISE_DEFAULTS["sigma_normal"],
            sigma_albedo=N.DENOISE_DEFAULTS["sigma_albedo"], sigma_plane=N.DENOISE_DEFAULTS["sigma_plane"],
            want_u8=True, rgbx=False, out_u8=None, timings=None, ctx=None):
    """The a-trous filter of srt_denoise over the linear RGB `rgb` (3, n) with the guides `aovs`
    ("normal", "albedo", "position" (3, n), "depth" (n,); render_aovs' dict or the caller's own arrays).
    Returns (filtered rgb (3, n), uint8 image (height, width, 3 or 4) or None).  `out_u8`: a host uint8
    array to write the image into; `timings`: a list that receives each level's kernel time and then the whole
    chain's (first launch to the end of the resolve), ms by HIP events;
    `ctx`: another context than the process's."""
    lib = library()
    if ctx is None:
        ctx = context()[1]
    W, H = int(width), int(height)
    n = W * H
    planes = {}
    for k, rows in (("rgb", 3), ("normal", 3), ("albedo", 3), ("position", 3), ("depth", 1)):
        v = np.ascontiguousarray(rgb if k == "rgb" else aovs[k], dtype=np.float64)
        if v.size != rows * n:
            raise ValueError("denoise: %s must hold %d x %d values" % (k, rows, n))
        planes[k] = v
    a = N.DenoiseArgs()
    for k, v in planes.items():
        setattr(a, k, N.ptr(v))
    a.levels = int(levels)
    a.flags = N.DENOISE_RGBX if rgbx else 0
    a.sigma_color, a.sigma_normal = float(sigma_color), float(sigma_normal)
    a.sigma_albedo, a.sigma_plane = float(sigma_albedo), float(sigma_plane)
    out = np.empty((3, n))
    ch = 4 if rgbx else 3
    u8 = None
    if out_u8 is not None:
        if out_u8.dtype != np.uint8 or out_u8.size != ch * n or not out_u8.flags.c_contiguous:
            raise ValueError("out_u8 must be a contiguous uint8 array of %d bytes" % (ch * n))
        u8 = out_u8.reshape(n, ch)
    elif want_u8:
        u8 = np.empty((n, ch), dtype=np.uint8)
    ms = np.zeros(max(a.levels, 0) + 1) if timings is not None else None
    a.out_rgb, a.out_srgb8, a.ms_levels = N.ptr(out), N.ptr(u8), N.ptr(ms)
    N.check(lib, lib.srt_denoise(ctx, W, H, ctypes.byref(a)))
    if timings is not None:
        timings.extend(float(v) for v in ms)
    return out, (None if u8 is None else u8.reshape(H, W, ch))


def render_aovs_device(scene, pool, hit_id=False):
    """render_aovs' normal, albedo, position and depth images left in device memory of `pool` (a DeviceArrays):
    {"normal", "albedo", "position", "depth": device pointers, "ms_kernel"}; with `hit_id` also "hit_id", the
    int32 plane, and "colliders", the lowered collider table (host, N.COLLIDER_DTYPE) whose indices it holds."""
    L = upload(scene, ctx=pool.ctx)
    cd = camera_desc(scene.camera)
    n = int(scene.camera.screen_width) * int(scene.camera.screen_height)
    res = {k: pool.doubles(rows * n) for k, rows in (("normal", 3), ("albedo", 3), ("position", 3), ("depth", 1))}
    if hit_id:
        res["hit_id"] = pool.alloc(4 * n)
    out = N.AovOut()
    for k, p in res.items():
        setattr(out, k, p.value)
    N.check(pool.lib, pool.lib.srt_render_aovs(pool.ctx, ctypes.byref(cd), ctypes.byref(out)))
    res["ms_kernel"] = float(out.ms_kernel)
    if hit_id:
        res["colliders"] = L.colliders
        res["posed"] = L.posed
    return res


def _sum_stats(a, b):
    """The stats of a frame rendered as two calls."""
    out = dict(a)
    for k in ("total_rays", "shadow_rays", "passes", "ms_wall", "ms_device", "ms_trace_kernels", "ms_primary_kernel",
              "retries"):
        out[k] = a[k] + b[k]
    ra, rb = a["rays_per_depth"], b["rays_per_depth"]
    out["rays_per_depth"] = [(ra[d] if d < len(ra) else 0) + (rb[d] if d < len(rb) else 0)
                             for d in range(max(len(ra), len(rb)))]
    return out


def render_halves(scene, spp, rng="numpy", seed=None, batch_size=None, pool=None):
    """The frame Scene.render(spp) traces, as two half-frames: samples 0 .. ka-1 (ka = spp // 2) and
    ka .. spp-1 of that very frame -- the same jitter, the same Monte-Carlo keys (sample_base = ka for the
    second call) -- each averaged over its own samples.  numpy's global RNG is left where the plain render leaves
    it.  rng="numpy": the whole stream (every sample's jitter, then the sizing draw) is generated once on the
    device and each call reads its slice.
    Returns (A, B, ka, kb, stats): with `pool` (a DeviceArrays) A and B are device pointers to (3, n) doubles in
    it, without it host arrays."""
    if rng not in ("numpy", "numpy-host", "device"):
        raise ValueError("rng must be 'numpy', 'numpy-host' or 'device'")
    spp = int(spp)
    if spp < 2:
        raise ValueError("half-frames need at least 2 samples per pixel, not %d" % spp)
    ka = spp // 2
    kb = spp - ka
    cam = scene.camera
    n = int(cam.screen_width) * int(cam.screen_height)
    own = DeviceArrays() if pool is None else None
    p = own if pool is None else pool
    try:
        A, B = p.doubles(3 * n), p.doubles(3 * n)
        halves = ((A, 0, ka), (B, ka, kb))
        kw = dict(batch_size=batch_size, want_u8=False)
        if rng == "numpy":
            # (the seed of the Monte-Carlo draws comes from numpy's state before the jitter, as in render_scene(mt=True))
            kw["seed"] = seed if seed is not None else _default_seed()
            try:
                j = numpy_uniforms(spp * 4 * n, n_skip=4 * n)  # the sizing draw's numbers are skipped (scene.py:81)
                st = [render_scene(scene, k, jitter_device=j.value + 8 * 4 * n * s0, sample_base=s0, rgb_device=dst, **kw)
                      .stats for dst, s0, k in halves]
            finally:
                release_buffer("uniforms")
        elif rng == "numpy-host":
            jitter = cam.draw_jitter(spp)
            cam.draw_jitter(1)  # reference draws one more get_ray for sizing (scene.py:81)
            kw["seed"] = seed if seed is not None else _default_seed()  # (after the draws, as the plain render's)
            st = [render_scene(scene, k, jitter=jitter[s0:s0 + k], sample_base=s0, rgb_device=dst, **kw).stats
                  for dst, s0, k in halves]
        else:
            kw["seed"] = seed if seed is not None else _default_seed()
            st = [render_scene(scene, k, sample_base=s0, rgb_device=dst, **kw).stats for dst, s0, k in halves]
        stats = _sum_stats(st[0], st[1])
        if pool is not None:
            return A, B, ka, kb, stats
        return own.fetch(A, (3, n)), own.fetch(B, (3, n)), ka, kb, stats
    finally:
        if own is not None:
            own.__exit__()


def denoise_var(rgb_a, rgb_b, spp_a, spp_b, aovs, width, height, variance=False, demodulate=False,
                levels=N.DENOISE_DEFAULTS["levels"], sigma_color=N.DENOISE_DEFAULTS["sigma_color"],
                sigma_lum=N.DENOISE_VAR_DEFAULTS["sigma_lum"], sigma_normal=N.DENOISE_DEFAULTS["sigma_normal"],
                sigma_albedo=N.DENOISE_DEFAULTS["sigma_albedo"], sigma_plane=N.DENOISE_DEFAULTS["sigma_plane"],
                want_rgb=True, want_variance=False, want_u8=True, rgbx=False, out_u8=None, timings=None, ctx=None):
    """srt_denoise_var: the a-trous filter over a frame given as two half-frames `rgb_a` (mean of `spp_a`
    samples) and `rgb_b` (mean of `spp_b`), with the per-pixel variance of their difference steering the colour
    weight (`variance`, sigma_lum) and / or on the albedo-demodulated colour (`demodulate`); with neither it is
    denoise() of their sample-weighted mean.  The half-frames and the guides `aovs` ("normal", "albedo",
    "position", "depth") are numpy arrays or device pointers (ctypes.c_void_p / int: used in place).
    Returns (filtered rgb (3, n) or None, the last level's variance (n,) or None, uint8 image or None).
    `timings` receives each level's kernel time, the whole chain's (prepare to the end of the resolve) and the
    prepare kernel's, ms by HIP events."""
    lib = library()
    if ctx is None:
        ctx = context()[1]
    W, H = int(width), int(height)
    n = W * H
    a = N.DenoiseVarArgs()
    keep = []
    for field, v, rows in (("rgb_a", rgb_a, 3), ("rgb_b", rgb_b, 3), ("normal", aovs["normal"], 3),
                           ("albedo", aovs["albedo"], 3), ("position", aovs["position"], 3), ("depth", aovs["depth"], 1)):
        if isinstance(v, (ctypes.c_void_p, int)):
            setattr(a, field, _addr(v))
            continue
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.size != rows * n:
            raise ValueError("denoise_var: %s must hold %d x %d values" % (field, rows, n))
        keep.append(v)
        setattr(a, field, N.ptr(v))
    a.spp_a, a.spp_b, a.levels = int(spp_a), int(spp_b), int(levels)
    a.flags = (N.DENOISE_RGBX if rgbx else 0) | (N.DENOISE_VARIANCE if variance else 0) | \
              (N.DENOISE_DEMODULATE if demodulate else 0)
    a.sigma_color, a.sigma_lum, a.sigma_normal = float(sigma_color), float(sigma_lum), float(sigma_normal)
    a.sigma_albedo, a.sigma_plane = float(sigma_albedo), float(sigma_plane)
    out = np.empty((3, n)) if want_rgb else None
    var = np.empty(n) if want_variance else None
    ch = 4 if rgbx else 3
    u8 = None
    if out_u8 is not None:
        if out_u8.dtype != np.uint8 or out_u8.size != ch * n or not out_u8.flags.c_contiguous:
            raise ValueError("out_u8 must be a contiguous uint8 array of %d bytes" % (ch * n))
        u8 = out_u8.reshape(n, ch)
    elif want_u8:
        u8 = np.empty((n, ch), dtype=np.uint8)
    ms = np.zeros(max(a.levels, 0) + 2) if timings is not None else None
    a.out_rgb, a.out_variance, a.out_srgb8, a.ms_levels = N.ptr(out), N.ptr(var), N.ptr(u8), N.ptr(ms)
    N.check(lib, lib.srt_denoise_var(ctx, W, H, ctypes.byref(a)))
    if timings is not None:
        timings.extend(float(v) for v in ms)
    return out, var, (None if u8 is None else u8.reshape(H, W, ch))


def temporal_accumulate(rgb_a, rgb_b, aovs, width, height, history=None, prev_cam=None, demodulate=False,
                        max_history=N.TEMPORAL_DEFAULTS["max_history"], normal_max=N.TEMPORAL_DEFAULTS["temporal_normal"],
                        plane_max=N.TEMPORAL_DEFAULTS["temporal_plane"], out=None, timings=None, ctx=None, motion=None):
    """srt_temporal_accumulate: the half-frames `rgb_a`, `rgb_b` of the current frame blended with the reprojected
    history of the earlier frames, each half with its own.  `aovs`: the current guides ("hit_id" int32, "position",
    "normal", "depth", and "albedo" with `demodulate`).  `history`: None for a first frame, else the previous
    call's {"a", "b", "len"} (its "hist_a", "hist_b", "len" results) with that frame's guides {"hit_id", "position",
    "normal"}, and `prev_cam` that frame's CameraDesc (xs / ys are not read).  Arrays are numpy arrays or device
    pointers (ctypes.c_void_p / int: used in place).  `out`: None for new host arrays, else the device pointers
    {"a", "b", "hist_a", "hist_b", "len"} to write ("a" / "b" may be `rgb_a` / `rgb_b`; "hist_*" / "len" must not
    be the history's).  Returns {"a", "b", "hist_a", "hist_b" (3, n), "len" (n,)}, or `out` itself.
    `motion`: None, or the per-collider table (rows, 12) that maps a current point of collider hit_id to its place
    in the previous frame (_motion.collider_motion) -- a numpy array, or (device pointer, rows).
    `timings` receives the kernel's time, ms by HIP events."""
    lib = library()
    if ctx is None:
        ctx = context()[1]
    W, H = int(width), int(height)
    n = W * H
    a = N.TemporalArgs()
    keep = []

    def put(field, v, rows, dtype=np.float64):
        if isinstance(v, (ctypes.c_void_p, int)):
            setattr(a, field, _addr(v))
            return
        v = np.ascontiguousarray(v, dtype=dtype)
        if v.size != rows * n:
            raise ValueError("temporal_accumulate: %s must hold %d x %d values" % (field, rows, n))
        keep.append(v)
        setattr(a, field, N.ptr(v))

    put("rgb_a", rgb_a, 3)
    put("rgb_b", rgb_b, 3)
    put("hit_id", aovs["hit_id"], 1, np.int32)
    for k, rows in (("position", 3), ("normal", 3), ("depth", 1)):
        put(k, aovs[k], rows)
    if demodulate:
        put("albedo", aovs["albedo"], 3)
    if history is not None:
        if prev_cam is None:
            raise ValueError("temporal_accumulate: a history needs the camera of its frame (prev_cam)")
        put("hist_a", history["a"], 3)
        put("hist_b", history["b"], 3)
        put("hist_len", history["len"], 1)
        put("hist_hit_id", history["hit_id"], 1, np.int32)
        put("hist_position", history["position"], 3)
        put("hist_normal", history["normal"], 3)
        a.prev_cam = ctypes.pointer(prev_cam)
    if motion is not None:
        if isinstance(motion, tuple):
            a.motion, a.n_motion = _addr(motion[0]), int(motion[1])
        else:
            motion = np.ascontiguousarray(motion, dtype=np.float64)
            if motion.ndim != 2 or motion.shape[1] != 12 or not len(motion):
                raise ValueError("temporal_accumulate: motion must hold rows of 12 values, not %r" % (motion.shape,))
            keep.append(motion)
            a.motion, a.n_motion = N.ptr(motion), len(motion)
    a.max_history = int(max_history)
    a.flags = N.TEMPORAL_DEMODULATE if demodulate else 0
    a.normal_max, a.plane_max = float(normal_max), float(plane_max)
    fields = (("a", "out_a", 3), ("b", "out_b", 3), ("hist_a", "out_hist_a", 3), ("hist_b", "out_hist_b", 3),
              ("len", "out_len", 1))
    if out is None:
        res = {k: np.empty((3, n) if rows == 3 else n) for k, _, rows in fields}
        for k, field, _ in fields:
            setattr(a, field, N.ptr(res[k]))
    else:
        res = out
        for k, field, _ in fields:
            setattr(a, field, _addr(out[k]))
    ms = ctypes.c_double(0.0)
    a.ms_kernel = ctypes.pointer(ms)
    N.check(lib, lib.srt_temporal_accumulate(ctx, W, H, ctypes.byref(a)))
    if timings is not None:
        timings.append(float(ms.value))
    return res


class TemporalHistory:
    """What srt_temporal_accumulate carries from one frame of a sequence to the next, in device memory of the
    process context (device_buffer / release_buffer): two sets of the accumulated half-frames and their lengths
    ("a", "b" (3, n), "len" (n,)) and of the frame's guides ("hit_id" int32, "position", "normal"), swapped every
    frame -- the call reads one set and writes the other -- and the previous frame's camera.  With `motion` also a
    copy of that frame's lowered collider table (host), from which the next frame's motion table is derived.
    reset(), and a frame of another size, drop everything."""

    PLANES = (("a", 24), ("b", 24), ("len", 8), ("hit_id", 4), ("position", 24), ("normal", 24))  # bytes per pixel

    def __init__(self):
        self.size = None      # (W, H) of the buffers
        self.cur = 0          # the set holding the previous frame
        self.prev_cam = None  # that frame's CameraDesc; None: no history
        self.prev_colliders = None  # that frame's collider table if it was rendered with `motion`, else None
        self.prev_posed = []        # ... and its device-posed meshes (Lowered.posed)

    def _name(self, k, s):
        return "temporal_%x_%s%d" % (id(self), k, s)

    def reset(self):
        if self.size is not None:
            for s in (0, 1):
                for k, _ in self.PLANES:
                    release_buffer(self._name(k, s))
            release_buffer(self._name("motion", 0))
        self.size, self.prev_cam, self.cur, self.prev_colliders, self.prev_posed = None, None, 0, None, []

    def _set(self, s, n):
        return {k: device_buffer(self._name(k, s), bytes_pp * n) for k, bytes_pp in self.PLANES}

    def accumulate(self, rgb_a, rgb_b, aovs, cam_desc, width, height, demodulate=False, timings=None, colliders=None,
                   motion=False, posed=(), **params):
        """One frame: the device half-frames `rgb_a`, `rgb_b` are accumulated in place against the history, which
        then becomes this frame's (`aovs`: device guides with "hit_id"; `cam_desc`: the frame's CameraDesc;
        `params`: temporal_accumulate's max_history / normal_max / plane_max).  `motion` with `colliders`, the
        frame's lowered collider table: the table of _motion.collider_motion against the previous frame's is
        passed on -- when that frame left one, which a first frame, a frame after reset() and a frame rendered
        without `motion` do not: this frame then runs without a table.  A copy is kept either way (the caller's
        objects change in place).  `posed`: the frame's device-posed meshes (Lowered.posed), whose table records
        stay in the rest pose: their rows come from the pose pair of the two frames (_motion.pose_motion).
        Returns None, or (moved, unknown) rows of the table that was used ((0, 0):
        none was)."""
        lib, ctx = context()
        W, H = int(width), int(height)
        n = W * H
        if self.size != (W, H):
            self.reset()
            self.size = (W, H)
        prev, nxt = self._set(self.cur, n), self._set(1 - self.cur, n)
        table, counts = None, None
        if motion:
            if colliders is None:
                raise ValueError("TemporalHistory.accumulate: motion needs the frame's collider table")
            counts = (0, 0)
            if self.prev_cam is not None and self.prev_colliders is not None:
                rows = collider_motion(self.prev_colliders, colliders)
                pose_motion(rows, self.prev_posed, posed)
                if len(rows):
                    counts = count_rows(rows)
                    dev = device_buffer(self._name("motion", 0), rows.nbytes)
                    N.check(lib, lib.srt_memcpy(ctx, dev, N.ptr(rows), rows.nbytes))
                    table = (dev, len(rows))
        temporal_accumulate(rgb_a, rgb_b, aovs, W, H, history=prev if self.prev_cam is not None else None,
                            prev_cam=self.prev_cam, demodulate=demodulate, timings=timings,
                            out={"a": rgb_a, "b": rgb_b, "hist_a": nxt["a"], "hist_b": nxt["b"], "len": nxt["len"]},
                            motion=table, **params)
        self.prev_colliders = np.array(colliders, copy=True) if motion else None
        self.prev_posed = [dict(p, pose=p["pose"].copy(), deform=None) for p in posed] if motion else []
        for k, bytes_pp in self.PLANES[3:]:  # this frame's guides are the next frame's history guides
            N.check(lib, lib.srt_memcpy(ctx, nxt[k], _addr(aovs[k]), bytes_pp * n))
        cam = N.CameraDesc()
        ctypes.memmove(ctypes.byref(cam), ctypes.byref(cam_desc), ctypes.sizeof(cam))
        cam.xs = cam.ys = None
        self.prev_cam, self.cur = cam, 1 - self.cur
        return counts

    def __del__(self):
        try:
            if _STATE["ctx"] is not None:
                self.reset()
        except Exception:  # (interpreter shutdown: the process frees it)
            pass


def primary_rays(camera, jitter):
    """Camera.get_ray geometry for one sample; jitter (4, H*W).  Returns (origin, dir) vec3."""
    lib, ctx = context()
    cd = camera_desc(camera)
    n = int(camera.screen_width) * int(camera.screen_height)
    J = np.ascontiguousarray(jitter, dtype=np.float64).reshape(4, n)
    O = np.empty((3, n))
    D = np.empty((3, n))
    N.check(lib, lib.srt_primary_rays(ctx, ctypes.byref(cd), N.ptr(J), N.ptr(O), N.ptr(D)))
    return vec3(O[0], O[1], O[2]), vec3(D[0], D[1], D[2])
