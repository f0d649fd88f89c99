"""Expected values for the variance-guided, albedo-demodulated denoiser (tests/test_denoise_var.py,
tests/test_gpu_denoise_var.py), restated in numpy.  csrc/rt_denoise.h states the same definition; nothing
here reads it.  Everything is float64, in the order written.

Inputs: half-frames A (mean of ka samples) and B (mean of kb samples), planar (3, n), spp = ka + kb; the
guides of tests/denoise_ref.py; lum(x) = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b.

Prepare:
    c = (ka*A + kb*B) / spp
    ok = the pixel is not background and every component of A and B is finite
    demodulate and ok:  d = max(albedo, 1e-3) per channel, uA = A/d, uB = B/d, u = c/d
    otherwise:          uA = A, uB = B, u = c
    v = ((ka*kb) / (spp*spp)) * (lum(uA) - lum(uB))**2 where ok, else 0
Level l (step 2**l) with `variance`: denoise_ref's level on u, whose colour term becomes
        |lum(u_p) - lum(u_q)| / (sigma_lum * sqrt(g_p) + 1e-8)                 (the same at every level)
    level 0:  g_p = sum(k*v_q) / sum(k), k = (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), over q = p + (dx, dy), dy in
              -1..1 (outer), dx in -1..1 (inner), q inside the image and not background
    l >= 1:   g_p = v_p, the level's own v (a 3x3 estimate at every level would carry a noisy neighbour's
              variance one pixel further into a noise-free region per level)
    u'_p = sum(w*u_q) / sum(w);  v'_p = sum(w^2*v_q) / sum(w)^2;  a pixel copied through keeps its v
  without `variance`: denoise_ref's level itself (sigma_color * 2**-l).
Finish: with `demodulate`, c' = u' * d where prepare divided; everywhere else c' = u'.
"""
import numpy as np

import denoise_ref as DR

DEFAULTS = dict(DR.DEFAULTS, sigma_lum=1.0)
K3 = (0.25, 0.5, 0.25)


def lum(x):
    return (0.2126 * x[0] + 0.7152 * x[1]) + 0.0722 * x[2]


def mean_of_halves(A, B, ka, kb):
    """c = (ka*A + kb*B) / spp."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (float(ka) * A + float(kb) * B) / (float(ka) + float(kb))


def prepare(A, B, ka, kb, guides, demodulate):
    """(u (3, n), v (n,), d (3, n) or None, ok (n,))."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    nm = np.asarray(guides["normal"], dtype=np.float64).reshape(3, -1)
    al = np.asarray(guides["albedo"], dtype=np.float64).reshape(3, -1)
    ka, kb = float(ka), float(kb)
    spp = ka + kb
    bg = (nm[0] == 0.0) & (nm[1] == 0.0) & (nm[2] == 0.0)
    ok = ~bg & np.isfinite(A).all(axis=0) & np.isfinite(B).all(axis=0)
    with np.errstate(all="ignore"):
        c = (ka * A + kb * B) / spp
        d = None
        uA, uB, u = A, B, c
        if demodulate:
            d = np.maximum(al, 1e-3)
            uA, uB, u = np.where(ok, A / d, A), np.where(ok, B / d, B), np.where(ok, c / d, c)
        dl = lum(uA) - lum(uB)
        v = np.where(ok, ((ka * kb) / (spp * spp)) * (dl * dl), 0.0)
    return u, v, d, ok


def _var3x3(v, bg, H, W):
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    gs, gw = np.zeros((H, W)), np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = yy + dy, xx + dx
            use = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            use = use & ~bg[qy, qx]
            kk = K3[dy + 1] * K3[dx + 1]
            gs = gs + np.where(use, kk * v[qy, qx], 0.0)
            gw = gw + np.where(use, kk, 0.0)
    with np.errstate(all="ignore"):
        return gs / gw  # (0/0 on background pixels, which are copied through)


def atrous_var(u, v, guides, W, H, levels, sigma_lum, sigma_normal, sigma_albedo, sigma_plane):
    """The levels with `variance`: (u' (3, n), v' (n,))."""
    n = W * H
    c = np.array(u, dtype=np.float64).reshape(3, H, W)
    v = np.array(v, dtype=np.float64).reshape(H, W)
    nm = np.asarray(guides["normal"], dtype=np.float64).reshape(3, H, W)
    al = np.asarray(guides["albedo"], dtype=np.float64).reshape(3, H, W)
    xs = np.asarray(guides["position"], dtype=np.float64).reshape(3, H, W)
    tp = np.asarray(guides["depth"], dtype=np.float64).reshape(H, W)
    bg = (nm[0] == 0.0) & (nm[1] == 0.0) & (nm[2] == 0.0)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sn2, sa2, sp2 = sigma_normal * sigma_normal, sigma_albedo * sigma_albedo, sigma_plane * sigma_plane
    for l in range(levels):
        s = 2 ** l
        fin = np.isfinite(c).all(axis=0)
        sw, sv = np.zeros((H, W)), np.zeros((H, W))
        acc = np.zeros((3, H, W))
        with np.errstate(all="ignore"):
            den = sigma_lum * np.sqrt(_var3x3(v, bg, H, W) if l == 0 else v) + 1e-8
            lp = lum(c)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = yy + s * dy, xx + s * dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    cq, nq, aq, xq, vq = c[:, qy, qx], nm[:, qy, qx], al[:, qy, qx], xs[:, qy, qx], v[qy, qx]
                    hh = DR.H5[dy + 2] * DR.H5[dx + 2]
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), hh)
                    else:
                        tc = np.abs(lp - lum(cq)) / den
                        tn = DR._sq(nm - nq) / sn2
                        ta = DR._sq(al - aq) / sa2
                        e = np.abs(nm[0] * (xq[0] - xs[0]) + nm[1] * (xq[1] - xs[1]) + nm[2] * (xq[2] - xs[2])) / tp
                        tpl = (e * e) / sp2
                        w = hh * np.exp(-(tc + tn + ta + tpl))
                        w = np.where(inside & ~bg[qy, qx] & fin[qy, qx], w, 0.0)
                    sw = sw + w
                    acc = acc + np.where(w != 0.0, w * cq, 0.0)
                    sv = sv + np.where(w != 0.0, (w * w) * vq, 0.0)
            keep = bg | ~fin
            c = np.where(keep, c, acc / sw)
            v = np.where(keep, v, sv / (sw * sw))
    return c.reshape(3, n), v.reshape(n)


def denoise_var(A, B, ka, kb, guides, W, H, variance=False, demodulate=False, levels=DEFAULTS["levels"],
                sigma_color=DEFAULTS["sigma_color"], sigma_lum=DEFAULTS["sigma_lum"],
                sigma_normal=DEFAULTS["sigma_normal"], sigma_albedo=DEFAULTS["sigma_albedo"],
                sigma_plane=DEFAULTS["sigma_plane"]):
    """(c' (3, n), the last level's v (n,) or None without `variance`)."""
    u, v, d, ok = prepare(A, B, ka, kb, guides, demodulate)
    if variance:
        u, v = atrous_var(u, v, guides, W, H, levels, sigma_lum, sigma_normal, sigma_albedo, sigma_plane)
    else:
        u = DR.atrous(u, guides, W, H, levels=levels, sigma_color=sigma_color, sigma_normal=sigma_normal,
                      sigma_albedo=sigma_albedo, sigma_plane=sigma_plane)
        v = None
    if demodulate:
        with np.errstate(all="ignore"):
            u = np.where(ok, u * d, u)
    return u, v


# ---- what the CPU and the GPU suite share ---------------------------------------------------------------
MODES = ((True, False), (False, True), (True, True))  # (variance, demodulate); (False, False) is srt_denoise
SIGMAS = dict(sigma_color=0.6, sigma_lum=3.0, sigma_normal=0.3, sigma_albedo=0.2, sigma_plane=0.05)


def random_halves(W, H, seed):
    """denoise_ref.random_frame's guides with two noisy half-frames around its colour: (A, B, guides, bg)."""
    rgb, guides, bg = DR.random_frame(W, H, seed)
    rng = np.random.default_rng(seed + 1000)
    A = rgb + 0.1 * rng.standard_normal(rgb.shape)
    B = rgb + 0.1 * rng.standard_normal(rgb.shape)
    return A, B, guides, (guides["normal"] == 0.0).all(axis=0)  # (random_frame leaves a 1 x 1 frame's pixel alone)


def step_and_noise_frame(seed=7):
    """The adaptivity frame, 64 x 16 on one flat surface: columns 0..31 hold a noise-free step (A == B: 0.4 in
    columns < 16, 0.6 from column 16), columns 32..63 hold 0.5 plus independent normal noise of sd 0.5 in A and
    in B.  (A, B, guides, W, H)."""
    W, H = 64, 16
    n = W * H
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(seed)
    clean = np.where(xx < 16, 0.4, 0.6).reshape(n)
    A = np.empty((3, n))
    B = np.empty((3, n))
    noisy = (xx >= 32).reshape(n)
    for ch in range(3):
        A[ch] = np.where(noisy, 0.5 + 0.5 * rng.standard_normal(n), clean)
        B[ch] = np.where(noisy, 0.5 + 0.5 * rng.standard_normal(n), clean)
    guides = {"normal": np.stack([np.zeros(n), np.zeros(n), np.ones(n)]), "albedo": np.ones((3, n)),
              "position": np.stack([xx.reshape(n).astype(np.float64), yy.reshape(n).astype(np.float64), np.zeros(n)]),
              "depth": np.full(n, 100.0)}
    return A, B, guides, W, H


def awkward_halves():
    """70 x 9 random half-frames with one inf pixel in A only, one nan pixel in B only and one pixel with a zero
    albedo channel, beside random_frame's block of background pixels: (A, B, guides, bg, {"inf", "nan", "zero"})."""
    W, H = 70, 9
    A, B, guides, bg = random_halves(W, H, 3)
    pix = {"inf": 2 * W + 5, "nan": 6 * W + 66, "zero": 4 * W + 20}
    assert not bg[list(pix.values())].any()
    A[1, pix["inf"]] = np.inf
    B[2, pix["nan"]] = np.nan
    guides["albedo"][0, pix["zero"]] = 0.0
    return A, B, guides, bg, pix


def fixture_error_ratios(g, g0, guides, sigma_lum=DEFAULTS["sigma_lum"], levels=(2, 3, 4)):
    """On the half-frame fixture `g` (denoise_var_cornell_64x64) and the 64-sample `ref` of `g0`
    (denoise_cornell_64x64), E(filtered) / E(unfiltered mean) by levels, E = denoise_ref.tonemapped_error:
    ({levels: the variance + demodulate mode}, {levels: srt_denoise's filter on the same mean})."""
    W, H = int(g["width"]), int(g["height"])
    ka, kb = int(g["spp_a"]), int(g["spp_b"])
    c = mean_of_halves(g["half_a"], g["half_b"], ka, kb)
    e0 = DR.tonemapped_error(c, g0["ref"])
    new = {l: DR.tonemapped_error(denoise_var(g["half_a"], g["half_b"], ka, kb, guides, W, H, variance=True,
                                              demodulate=True, levels=l, sigma_lum=sigma_lum)[0], g0["ref"]) / e0
           for l in levels}
    old = {l: DR.tonemapped_error(DR.atrous(c, guides, W, H, levels=l), g0["ref"]) / e0 for l in levels}
    return new, old


# The restatement's figures on step_and_noise_frame() with levels 3 and the defaults (sigma_lum 1.0), on the CPU:
#   mean squared error against 0.5 over columns >= 40: 0.019780534034691617 (the unfiltered mean: 0.1241;
#   srt_denoise's filter with its defaults: 0.0022 -- it averages everything, the step included)
#   largest deviation from the input: 1.1e-16 over columns 0..30, 3.0e-2 in column 31
MSE_NOISY_COLUMNS = 0.019780534034691617


def check_adaptivity(run_var, run_plain):
    """Columns 0..30 of the noise-free half come back as they went in (zero variance gives zero weight to every
    differing tap; column 31's 3x3 variance already sees column 32), the noisy half is filtered as far as the
    restatement filters it, and srt_denoise's filter with its defaults blurs the step the guides cannot see.
    run_var(A, B, guides, W, H) -> c' with `variance` and levels 3; run_plain(c, guides, W, H) -> srt_denoise's."""
    A, B, guides, W, H = step_and_noise_frame()
    c = mean_of_halves(A, B, 1, 1).reshape(3, H, W)
    out = run_var(A, B, guides, W, H).reshape(3, H, W)
    dev = np.abs(out - c).max(axis=(0, 1))
    mse = float(np.mean((out[:, :, 40:] - 0.5) ** 2))
    plain = run_plain(c.reshape(3, -1), guides, W, H).reshape(3, H, W)
    moved = float(np.abs(plain - c)[:, :, 15:17].max())
    print("largest deviation from the input, columns 0..30:", dev[:31].max(), "31:", dev[31],
          "| mse over columns >= 40:", mse, "| srt_denoise moves column 15 / 16 by", moved)
    assert dev[:31].max() <= 1e-12
    assert mse <= MSE_NOISY_COLUMNS * 1.05
    assert moved > 0.01
