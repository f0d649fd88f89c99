"""Expected values for the denoiser (tests/test_denoise.py, tests/test_gpu_denoise.py): the first-hit
guide images restated over the oracle's own functions, and the edge-avoiding a-trous filter restated in
numpy.  csrc/rt_denoise.h states the same definitions; nothing here reads it.

Guides of pixel p (planar, n = width * height, row-major), from the pixel-centre pinhole ray
(oracle primary_rays with the uniforms (0.5, 0.5, 0, 0)):
    hit_id    first collider at the nearest distance, -1 for a miss
    depth     that distance (FARAWAY for a miss)
    position  O + D * t
    normal    collider_normal(c, P) * orientation   (normal maps ignored)
    albedo    Glossy: diff_texture colour * diff_coeff; Diffuse: diff_texture colour; Emissive:
              texture_color colour; Refractive, ThinFilmInterference: (1, 1, 1)
A miss and a hit on the SkyBox / Panorama are background: normal, albedo and position are zero.

Filter level l = 0 .. levels-1, s = 2**l, c -> c':
    h = (1/16, 1/4, 3/8, 1/4, 1/16);  sigma_c(l) = sigma_color * 2**-l
    for dy in -2..2 (outer), dx in -2..2 (inner), q = p + s*(dx, dy):
        w = h[dy+2]*h[dx+2] * exp(-(|c_p-c_q|^2/sigma_c(l)^2 + |n_p-n_q|^2/sigma_normal^2
                                    + |a_p-a_q|^2/sigma_albedo^2 + (|n_p.(x_q-x_p)|/t_p)^2/sigma_plane^2))
        w = 0 if q is outside the image, p or q is background, or c_q has a non-finite component
        the centre tap always has w = h[2]*h[2]
    c'_p = sum(w*c_q) / sum(w)
A background pixel, and a pixel whose own colour is not finite, keep their colour.
"""
import numpy as np

import sightpy_oracle as O

DEFAULTS = {"levels": 4, "sigma_color": 1.0, "sigma_normal": 0.35, "sigma_albedo": 0.1, "sigma_plane": 0.02}
H5 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
GUIDES = ("normal", "albedo", "position", "depth")


def _albedo(m, c, P):
    kind = type(m).__name__
    if kind == "Glossy":
        return O._tex_color(m.diff_texture, c, P) * m.diff_coeff
    if kind == "Diffuse":
        return O._tex_color(m.diff_texture, c, P)
    if kind == "Emissive":
        return O._tex_color(m.texture_color, c, P)
    if kind in ("Refractive", "ThinFilmInterference"):
        return np.ones((3, 1))
    raise TypeError("denoise_ref: no albedo for material %s" % kind)


def aovs(scene):
    """{"hit_id", "depth", "position", "normal", "albedo"} of `scene` from the oracle."""
    cam = scene.camera
    n = int(cam.screen_width) * int(cam.screen_height)
    j = np.stack([np.full(n, 0.5), np.full(n, 0.5), np.zeros(n), np.zeros(n)])
    Oa, Da = O.primary_rays(cam, j)
    Oa = np.broadcast_to(Oa, (3, n))
    near, ids = O.hit_ids(scene, Oa, Da)
    dists = O.nearest(scene, Oa, Da)[1]
    out = {"hit_id": ids, "depth": near.copy(), "position": np.zeros((3, n)), "normal": np.zeros((3, n)),
           "albedo": np.zeros((3, n))}
    for ci in np.unique(ids[ids >= 0]):
        c = scene.collider_list[ci]
        m = c.assigned_primitive.material
        if type(m).__name__ == "SkyBox_Material":
            continue
        sel = ids == ci
        P = Oa[:, sel] + Da[:, sel] * near[sel]
        out["position"][:, sel] = P
        out["normal"][:, sel] = O.collider_normal(c, P) * dists[ci][1][sel]
        out["albedo"][:, sel] = _albedo(m, c, P)
    return out


def _sq(d):
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def atrous(rgb, guides, W, H, levels=DEFAULTS["levels"], sigma_color=DEFAULTS["sigma_color"],
           sigma_normal=DEFAULTS["sigma_normal"], sigma_albedo=DEFAULTS["sigma_albedo"],
           sigma_plane=DEFAULTS["sigma_plane"]):
    """The filtered linear RGB (3, W*H) of `rgb` (3, W*H) under `guides` ("normal", "albedo",
    "position" (3, W*H), "depth" (W*H,))."""
    n = W * H
    c = np.array(rgb, dtype=np.float64).reshape(3, H, W)
    nm = np.asarray(guides["normal"], dtype=np.float64).reshape(3, H, W)
    al = np.asarray(guides["albedo"], dtype=np.float64).reshape(3, H, W)
    xs = np.asarray(guides["position"], dtype=np.float64).reshape(3, H, W)
    tp = np.asarray(guides["depth"], dtype=np.float64).reshape(H, W)
    bg = (nm[0] == 0.0) & (nm[1] == 0.0) & (nm[2] == 0.0)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sn2, sa2, sp2 = sigma_normal * sigma_normal, sigma_albedo * sigma_albedo, sigma_plane * sigma_plane
    for l in range(levels):
        s = 2 ** l
        sc = sigma_color * 2.0 ** -l
        sc2 = sc * sc
        fin = np.isfinite(c).all(axis=0)
        sw = np.zeros((H, W))
        acc = np.zeros((3, H, W))
        with np.errstate(all="ignore"):
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = yy + s * dy, xx + s * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, nq, aq, xq = c[:, qy, qx], nm[:, qy, qx], al[:, qy, qx], xs[:, qy, qx]
                    hh = H5[dy + 2] * H5[dx + 2]
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), hh)
                    else:
                        tc = _sq(c - cq) / sc2
                        tn = _sq(nm - nq) / sn2
                        ta = _sq(al - aq) / sa2
                        e = np.abs(nm[0] * (xq[0] - xs[0]) + nm[1] * (xq[1] - xs[1]) + nm[2] * (xq[2] - xs[2])) / tp
                        tpl = (e * e) / sp2
                        w = hh * np.exp(-(tc + tn + ta + tpl))
                        w = np.where(inside & ~bg[qy, qx] & fin[qy, qx], w, 0.0)
                    sw = sw + w
                    acc = acc + np.where(w != 0.0, w * cq, 0.0)
            keep = bg | ~fin
            c = np.where(keep, c, acc / sw)
    return c.reshape(3, n)


def tonemapped_error(a, ref):
    """E(a) = mean((f(a) - f(ref))^2), f(x) = x / (1 + x)."""
    f = lambda x: x / (1.0 + x)
    return float(np.mean((f(np.asarray(a)) - f(np.asarray(ref))) ** 2))


# ---- what the CPU and the GPU suite share: tolerances, comparisons, the random frames ---------------------
RTOL, ATOL = 1e-5, 1e-12
LEVELS = (0, 1, 2, 3, 4, 5)


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=RTOL, atol=ATOL, equal_nan=True)


def same_aovs(got, ref, skip=None):
    """`skip` (bool, n): pixels left out of the albedo comparison (vattr_ref.texel_boundary_pixels)."""
    assert np.array_equal(got["hit_id"], ref["hit_id"])
    close(got["depth"], ref["depth"])
    for k in ("position", "normal"):
        close(got[k], ref[k])
    keep = slice(None) if skip is None else ~skip
    close(got["albedo"][:, keep], ref["albedo"][:, keep])
    # the background mark is an exactly zero normal, and only the background carries it
    bg = (ref["normal"] == 0.0).all(axis=0)
    assert np.array_equal((got["normal"] == 0.0).all(axis=0), bg)
    for k in ("position", "albedo"):
        assert not got[k][:, bg].any()


def random_frame(W, H, seed):
    """Smooth guides with noise (so that the weights are neither all one nor all zero), a noisy colour,
    and a block of background pixels."""
    rng = np.random.default_rng(seed)
    n = W * H
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    nrm = np.stack([0.2 * np.sin(xx / 7.0), 0.2 * np.cos(yy / 5.0), np.ones((H, W))]).reshape(3, n)
    nrm = nrm + 0.05 * rng.standard_normal((3, n))
    nrm /= np.sqrt((nrm * nrm).sum(axis=0))
    alb = 0.5 + 0.03 * rng.standard_normal((3, n))
    pos = np.stack([xx * 0.1, yy * 0.1, 0.02 * np.sin(xx / 3.0) + 2.0]).reshape(3, n) + 0.001 * rng.standard_normal((3, n))
    depth = 2.0 + 0.1 * rng.random(n)
    rgb = 0.5 + 0.4 * rng.random((3, n))
    bg = ((yy >= H // 3) & (yy <= H // 3 + 2) & (xx >= W // 2) & (xx <= W // 2 + 9)).reshape(n)
    if n > 1:
        nrm[:, bg], alb[:, bg], pos[:, bg], depth[bg] = 0.0, 0.0, 0.0, 1.0e39
    return rgb, {"normal": nrm, "albedo": alb, "position": pos, "depth": depth}, bg


SHAPES = ((1, 1), (5, 3), (70, 9))
