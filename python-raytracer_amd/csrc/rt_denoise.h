// rt_denoise.h -- denoising a Monte-Carlo frame: the first-hit guide images (k_aov) and the
// edge-avoiding a-trous wavelet filter (k_atrous; Dammertz et al., HPG 2010, with a plane-distance
// term in place of the position term).  No reference counterpart: the reference has no denoiser.
//
// The per-pixel functions are RT_HD: the kernels below and the host check harness
// (rt_hostcheck.cpp hc_aovs / hc_denoise) run the same code.  Everything is float64, evaluated in
// the order written here with FP contraction disabled; tests/denoise_ref.py restates it in numpy.
//
// Guides of pixel p (planar, n = width * height):
//   hit_id    nearest collider of the pixel-centre pinhole ray (primary_ray with jitter
//             (0.5, 0.5, 0, 0)), -1 for a miss
//   depth     its distance t (FARAWAY for a miss)
//   position  O + D * t, the un-nudged hit point
//   normal    collider_normal<MAT_VATTR>(c, P) * orientation: interpolated vertex normals on
//             SRT_CF_VNORMAL triangles; normal maps are ignored
//   albedo    Glossy: the shader's diffuse term (p[0..2], or texel * diff_coeff); Diffuse / Emissive:
//             p[0..2] or the texel; Refractive / ThinFilm: (1, 1, 1)
// A miss and a hit on the SkyBox / Panorama collider are background: normal, albedo and position are
// zero.  The exactly zero normal is the background mark (normals of real hits have unit length).
//
// Filter level l = 0 .. levels-1, step s = 2^l, colour c -> c':
//   h = (1/16, 1/4, 3/8, 1/4, 1/16), sigma_c(l) = sigma_color * 2^-l
//   for dy in -2..2 (outer), dx in -2..2 (inner), q = p + s * (dx, dy):
//     w = h[dy+2] * h[dx+2] * exp(-(|c_p - c_q|^2 / sigma_c(l)^2 + |n_p - n_q|^2 / sigma_normal^2
//                                   + |a_p - a_q|^2 / sigma_albedo^2
//                                   + (|n_p . (x_q - x_p)| / t_p)^2 / sigma_plane^2))
//     w = 0 when q is outside the image, q is background or c_q has a non-finite component;
//     the centre tap always weighs h[2] * h[2]
//   c'_p = sum(w * c_q) / sum(w)
// A background pixel and a pixel whose own colour is not finite are copied through.
//
// Variance-guided, albedo-demodulated mode (srt_denoise_var; tests/denoise_var_ref.py restates it).  The
// frame comes as two half-frames A (mean of ka samples) and B (mean of kb samples), spp = ka + kb;
// lum(x) = (0.2126 x.r + 0.7152 x.g) + 0.0722 x.b.  SRT_DENOISE_VARIANCE and SRT_DENOISE_DEMODULATE are
// independent; with neither, the levels above run on c.
//   prepare (k_dn_prepare, one thread per pixel):
//     c = (ka * A + kb * B) / spp
//     ok = p is not background and every component of A and B is finite
//     demodulate and ok: d = max(albedo, 1e-3) per channel, uA = A / d, uB = B / d, u = c / d
//     otherwise:         uA = A, uB = B, u = c
//     v = ((ka * kb) / (spp * spp)) * (lum(uA) - lum(uB))^2 when ok, else 0      (variance of lum(u))
//   level l with VARIANCE (k_atrous<true>), u -> u', v -> v':
//     level 0: k = (1/4, 1/2, 1/4); g_p = sum(k[dy+1] * k[dx+1] * v_q) / sum(k[dy+1] * k[dx+1]) over
//       q = p + (dx, dy), dy in -1..1 (outer), dx in -1..1 (inner), q inside the image and not background
//     level l >= 1: g_p = v_p, the level's own v (an aggregate over the previous level's taps already).  Were the
//       3x3 estimate taken again at every level, the variance a clean pixel beside a noisy one picks up would
//       reach one pixel further into a noise-free region per level, and the filter would alter it
//     the colour term of w is |lum(u_p) - lum(u_q)| / (sigma_lum * sqrt(g_p) + 1e-8), the same at every level;
//     the other three terms, the tap order, the centre tap and the taps left out are those above
//     u'_p = sum(w * u_q) / sum(w),  v'_p = sum(w^2 * v_q) / sum(w)^2
//     a pixel that is copied through keeps its v
//   finish (k_dn_finish, with DEMODULATE): c' = u' * d where prepare divided, else u' itself (which is c,
//     bit for bit, on background and non-finite pixels); resolved by resolve_pixel
//
// Temporal accumulation (srt_temporal_accumulate, k_temporal; tests/temporal_ref.py restates it).  It runs before
// prepare: half-frames A, B in, half-frames out_a, out_b out, each blended with its own reprojected history (A's
// history never mixes with B's, so the two stay independent estimates and v above stays a valid noise estimate).
// Pixel p of the current frame has guides hit_id_p, x_p (position), n_p (normal), albedo, t_p (depth); the previous
// call left hist_a, hist_b (the accumulated, demodulated half-frames), hist_len (accumulated frames, a double) and
// its own hit_id / position / normal; primes mark the previous frame's camera.  hist_len == NULL: no history.
//   ok = p is not background and A, B are finite (dn_halves_ok)
//   d = dn_divisor(albedo) with SRT_TEMPORAL_DEMODULATE, else 1;  uA = A / d, uB = B / d per channel
//   not ok: out_a = A, out_b = B (bit for bit), out_hist_a = A, out_hist_b = B, out_len = 0
//   projection: e = x_p - look_from', fwd' = fwd_fd' / focal_distance' per component, zc = dot(e, fwd'),
//     xc = dot(e, right') / zc, yc = dot(e, up') / zc
//     fx = W > 1 ? ((xc + cw'/2) / cw') * (W-1) : 0,  fy = H > 1 ? ((ch'/2 - yc) / ch') * (H-1) : 0
//     (the inverse of np.linspace(-cw/2, cw/2, W) / linspace(ch/2, -ch/2, H))
//     no history unless zc > 0, -1 < fx < W and -1 < fy < H (NaN fails these tests)
//   taps: x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0; in this order (y0, x0) with
//     w = (1-ax)(1-ay), (y0, x0+1) with ax(1-ay), (y0+1, x0) with (1-ax)ay, (y0+1, x0+1) with ax*ay
//     tap q is valid when it is inside the image, w > 0, hist_len_q >= 1, hist_hit_id_q == hit_id_p,
//     |n_p - n_q|^2 <= normal_max and |dot(n_p, x_q - x_p)| / t_p <= plane_max
//     sw = sum(w) over the valid taps; history exists when sw >= 0.01
//     hA = sum(w * hist_a_q) / sw, hB likewise, L = sum(w * hist_len_q) / sw
//   with history: N = min(L + 1, max_history), alpha = 1 / N, uA' = hA + alpha * (uA - hA), uB' likewise;
//     out_len = N, out_hist_a/b = uA'/uB', out_a/b = uA' * d / uB' * d (uA' / uB' themselves without DEMODULATE)
//   without (a disocclusion included): out_a = A, out_b = B (bit for bit), out_hist_a/b = uA/uB, out_len = 1
// The current frame's hit_id / position / normal are the next call's history guides; the caller keeps them.
//
// Per-collider motion (motion != NULL; k_temporal<true>, tests/temporal_motion_ref.py restates it).  motion[n_motion][12],
// float64: row m belongs to the collider whose device index is m (the hit_id srt_render_aovs writes); entries 0..8
// are a 3x3 matrix R, row-major, entries 9..11 a vector t, and together they map a point on that collider in the
// current frame to the same surface point in the previous frame.  For an ok pixel with history present, id = hit_id_p:
//   id < 0 or id >= n_motion: no history (the "without" branch above)
//   x'_k = ((R[k][0] * x_p.x + R[k][1] * x_p.y) + R[k][2] * x_p.z) + t[k]
//   n'_k = (R[k][0] * n_p.x + R[k][1] * n_p.y) + R[k][2] * n_p.z
//   the projection takes e = x' - look_from'; a tap is valid under the conditions above with n' in place of n_p
//   and x' in place of x_p: |n' - n_q|^2 <= normal_max and |dot(n', x_q - x')| / t_p <= plane_max (t_p is the
//   current depth, unchanged); everything after the taps is unchanged
// which is the definition above on guides whose position and normal are x' and n' (depth, hit_id and albedo as they
// are).  A row holding a NaN gives a NaN zc, which fails zc > 0: that collider's pixels take the "without" branch
// (out_a = A, out_b = B bit for bit, out_len = 1) -- how a caller says "this collider changed in a way a rigid
// transform does not express".  Rows are expected to be rigid; nothing checks it and n' is not renormalised.  The
// identity row (1,0,0, 0,1,0, 0,0,1, 0,0,0) gives x' = x_p and n' = n_p bit for bit (x*1 + y*0 + z*0 + 0 on finite
// guides; the sign of a zero may differ, which no later step tells apart).
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include "rt_device.h"

namespace rt {

// ---- first-hit guides ----------------------------------------------------------------------------
struct AovPixel {
    int32_t id;
    double t;
    d3 P, N, A;
};

RT_HD AovPixel aov_pixel(const SceneView& S, const srt_camera& cam, double xc, double yr, uint32_t& err) {
    const double j[4] = {0.5, 0.5, 0.0, 0.0};  // the pixel centre through the lens centre
    d3 O, D;
    primary_ray(cam, xc, yr, j, O, D);
    AovPixel r;
    double on;
    bool ties;
    r.id = nearest_hit(S, O, D, r.t, on, ties);
    r.P = r.N = r.A = d3{0.0, 0.0, 0.0};
    if (r.id < 0) return r;
    const RT_RO srt_collider& c = S.col[r.id];
    const RT_RO srt_material& m = S.mat[c.material];
    if (m.type == SRT_SKY) return r;
    r.P = add(O, mul(D, r.t));
    r.N = mul(collider_normal<MAT_VATTR>(c, r.P), on);
    if (m.type == SRT_REFRACTIVE || m.type == SRT_THINFILM) {
        r.A = d3{1.0, 1.0, 1.0};
    } else if (m.tex >= 0) {
        double u, v;
        if (!collider_uv<MAT_VATTR>(c, r.P, u, v)) err |= ERR_UNSUPPORTED;
        r.A = tex_rgb(S, m.tex, u, v, err);
        if (m.type == SRT_GLOSSY) r.A = mul(r.A, m.p[3]);  // texture colour * diff_coeff (glossy.py:30)
    } else {
        r.A = ld3(m.p);
    }
    return r;
}

// ---- a-trous filter --------------------------------------------------------------------------------
struct AtrousTap {
    d3 c, n, a, x;  // colour, normal, albedo, position of one pixel
};

// the planes in global memory, planar [3][npix], rows of W pixels
struct AtrousPlanes {
    const double *rgb, *normal, *albedo, *position, *depth;
    int64_t npix;
    int64_t W;
    RT_HDM AtrousTap tap(int64_t qy, int64_t qx) const {
        const int64_t q = qy * W + qx;
        AtrousTap t;
        t.c = d3{rgb[q], rgb[npix + q], rgb[2 * npix + q]};
        t.n = d3{normal[q], normal[npix + q], normal[2 * npix + q]};
        t.a = d3{albedo[q], albedo[npix + q], albedo[2 * npix + q]};
        t.x = d3{position[q], position[npix + q], position[2 * npix + q]};
        return t;
    }
};

struct AtrousLevel {
    int32_t W, H, step;
    double sc2, sn2, sa2, sp2;  // sigma_c(l)^2, sigma_normal^2, sigma_albedo^2, sigma_plane^2
};

// what a level of the variance-guided mode reads and writes beside the colour (unused without VAR)
struct AtrousVar {
    const double* v;  // [npix] variance of lum(u)
    double* v_out;    // [npix] the level's v'
    double sl;        // sigma_lum
};

// pixel i of a planar [3][n] image
RT_HDM d3 dn_ld3(const double* p, int64_t n, int64_t i) { return d3{p[i], p[n + i], p[2 * n + i]}; }
RT_HD bool dn_finite(double v) { return v - v == 0.0; }
RT_HD bool dn_finite3(d3 v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z); }
RT_HD double dn_sq(d3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }
RT_HD double dn_lum(d3 c) { return (0.2126 * c.x + 0.7152 * c.y) + 0.0722 * c.z; }

// g_p of pixel (x, y): the 3x3 Gaussian of v over the taps inside the image that are not background
RT_HD double atrous_var3x3(const AtrousPlanes& G, const AtrousLevel& K, const double* v, int32_t x, int32_t y) {
    const double k[3] = {0.25, 0.5, 0.25};
    double gs = 0.0, gw = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int64_t qy = (int64_t)y + dy;
        if (qy < 0 || qy >= K.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int64_t qx = (int64_t)x + dx;
            if (qx < 0 || qx >= K.W) continue;
            const int64_t q = qy * G.W + qx;
            if (is_zero(d3{G.normal[q], G.normal[G.npix + q], G.normal[2 * G.npix + q]})) continue;
            const double kk = k[dy + 1] * k[dx + 1];
            gs += kk * v[q];
            gw += kk;
        }
    }
    return gs / gw;
}

// c'_p of pixel (x, y) (with VAR: u'_p, and v'_p in vout).  The dy loop's bounds test is the same for every
// pixel of a row (wave-uniform on the device); a tap outside the row reads the clamped column and weighs nothing.
template <bool VAR>
RT_HD d3 atrous_pixel(const AtrousPlanes& G, const AtrousLevel& K, const AtrousVar& V, int32_t x, int32_t y,
                      double& vout) {
    const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const AtrousTap p = G.tap(y, x);
    if constexpr (VAR) vout = V.v[(int64_t)y * G.W + x];
    if (is_zero(p.n) || !dn_finite3(p.c)) return p.c;
    const double tp = G.depth[(int64_t)y * G.W + x];
    double sw = 0.0;
    d3 sc = d3{0.0, 0.0, 0.0};
    double lp = 0.0, den = 1.0, sv = 0.0;
    if constexpr (VAR) {
        lp = dn_lum(p.c);
        den = V.sl * sqrt(K.step == 1 ? atrous_var3x3(G, K, V.v, x, y) : vout) + 1e-8;
    }
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = (int64_t)y + (int64_t)dy * K.step;
        if (qy < 0 || qy >= K.H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = (int64_t)x + (int64_t)dx * K.step;
            const bool inside = qx >= 0 && qx < K.W;
            const int64_t qxc = qx < 0 ? 0 : (qx >= K.W ? K.W - 1 : qx);
            const AtrousTap q = G.tap(qy, qxc);
            const double hh = h[dy + 2] * h[dx + 2];
            double w;
            if (dx == 0 && dy == 0) {
                w = hh;
            } else if (!inside || is_zero(q.n) || !dn_finite3(q.c)) {
                continue;
            } else {
                double tc;
                if constexpr (VAR)
                    tc = fabs(lp - dn_lum(q.c)) / den;
                else
                    tc = dn_sq(sub(p.c, q.c)) / K.sc2;
                const double tn = dn_sq(sub(p.n, q.n)) / K.sn2;
                const double ta = dn_sq(sub(p.a, q.a)) / K.sa2;
                const double e = fabs(dot(p.n, sub(q.x, p.x))) / tp;
                const double tpl = (e * e) / K.sp2;
                w = hh * exp(-(((tc + tn) + ta) + tpl));
            }
            sw += w;
            sc = add(sc, mul(q.c, w));
            if constexpr (VAR) sv += (w * w) * V.v[qy * G.W + qxc];
        }
    }
    if constexpr (VAR) vout = sv / (sw * sw);
    return divs(sc, sw);
}

// ---- half-frames: prepare and finish (header comment) ------------------------------------------------
struct DnHalves {
    const double *a, *b;  // [3][npix] each
    double ka, kb, spp;   // sample counts, spp = ka + kb
    int32_t demod;
};

struct DnPrepared {
    d3 u;
    double v;
};

RT_HD d3 dn_divisor(d3 a) { return d3{a.x > 1e-3 ? a.x : 1e-3, a.y > 1e-3 ? a.y : 1e-3, a.z > 1e-3 ? a.z : 1e-3}; }
RT_HD bool dn_halves_ok(d3 A, d3 B, d3 n) { return !is_zero(n) && dn_finite3(A) && dn_finite3(B); }

RT_HD DnPrepared dn_prepare_pixel(const DnHalves& F, d3 A, d3 B, d3 n, d3 alb) {
    DnPrepared r;
    r.u = divs(add(mul(A, F.ka), mul(B, F.kb)), F.spp);
    r.v = 0.0;
    if (!dn_halves_ok(A, B, n)) return r;
    d3 uA = A, uB = B;
    if (F.demod) {
        const d3 d = dn_divisor(alb);
        uA = d3{A.x / d.x, A.y / d.y, A.z / d.z};
        uB = d3{B.x / d.x, B.y / d.y, B.z / d.z};
        r.u = d3{r.u.x / d.x, r.u.y / d.y, r.u.z / d.z};
    }
    const double dl = dn_lum(uA) - dn_lum(uB);
    r.v = ((F.ka * F.kb) / (F.spp * F.spp)) * (dl * dl);
    return r;
}

// c' of a pixel whose filtered u' is `u` (SRT_DENOISE_DEMODULATE)
RT_HD d3 dn_finish_pixel(d3 u, d3 A, d3 B, d3 n, d3 alb) {
    if (!dn_halves_ok(A, B, n)) return u;
    return mul(u, dn_divisor(alb));
}

// ---- temporal accumulation (header comment) -----------------------------------------------------------
// the previous frame's camera: srt_camera's scalars, fwd = fwd_fd / focal_distance per component
struct TemporalCam {
    d3 from, right, up, fwd;
    double cw, ch;
};

RT_HD TemporalCam temporal_cam(const srt_camera& c) {
    TemporalCam t;
    t.from = ld3(c.look_from);
    t.right = ld3(c.right);
    t.up = ld3(c.up);
    t.fwd = d3{c.fwd_fd[0] / c.focal_distance, c.fwd_fd[1] / c.focal_distance, c.fwd_fd[2] / c.focal_distance};
    t.cw = c.cam_width;
    t.ch = c.cam_height;
    return t;
}

// the planes in global memory, planar [3][npix] or [npix], rows of W pixels
struct TemporalPlanes {
    const double *a, *b;  // the current half-frames
    const int32_t* hit_id;
    const double *position, *normal, *albedo, *depth;
    const double *hist_a, *hist_b, *hist_len;  // hist_len == NULL: no history
    const int32_t* hist_hit_id;
    const double *hist_position, *hist_normal;
    int64_t npix;
    int32_t W, H;
    TemporalCam cam;
    double max_history, normal_max, plane_max;
    int32_t demod;
    // [n_motion][12] rows (R row-major, t), read by temporal_pixel<true> alone: the <false> kernel never loads
    // these two arguments, so they cost it no SGPR
    int32_t n_motion;
    const double* motion;
};

struct TemporalPixel {
    d3 a, b, hist_a, hist_b;
    double len;
};

RT_HD d3 tp_div3(d3 a, d3 d) { return d3{a.x / d.x, a.y / d.y, a.z / d.z}; }

// MOTION: x_p and n_p go through the pixel's row of T.motion first (header comment)
template <bool MOTION>
RT_HD TemporalPixel temporal_pixel(const TemporalPlanes& T, int32_t x, int32_t y) {
    const int64_t n = T.npix, ip = (int64_t)y * T.W + x;
    const d3 A = dn_ld3(T.a, n, ip), B = dn_ld3(T.b, n, ip), nrm = dn_ld3(T.normal, n, ip);
    TemporalPixel r;
    r.a = r.hist_a = A;
    r.b = r.hist_b = B;
    r.len = 0.0;
    if (!dn_halves_ok(A, B, nrm)) return r;
    d3 d = d3{1.0, 1.0, 1.0};
    if (T.demod) {
        d = dn_divisor(dn_ld3(T.albedo, n, ip));
        r.hist_a = tp_div3(A, d);
        r.hist_b = tp_div3(B, d);
    }
    r.len = 1.0;
    if (!T.hist_len) return r;
    d3 xp = dn_ld3(T.position, n, ip);
    d3 np = nrm;
    int32_t id;
    if constexpr (MOTION) {
        id = T.hit_id[ip];
        if (id < 0 || id >= T.n_motion) return r;
        const double* M = T.motion + (int64_t)id * 12;
        const d3 x0 = xp;
        xp = d3{((M[0] * x0.x + M[1] * x0.y) + M[2] * x0.z) + M[9], ((M[3] * x0.x + M[4] * x0.y) + M[5] * x0.z) + M[10],
                ((M[6] * x0.x + M[7] * x0.y) + M[8] * x0.z) + M[11]};
        np = d3{(M[0] * nrm.x + M[1] * nrm.y) + M[2] * nrm.z, (M[3] * nrm.x + M[4] * nrm.y) + M[5] * nrm.z,
                (M[6] * nrm.x + M[7] * nrm.y) + M[8] * nrm.z};
    }
    const d3 e = sub(xp, T.cam.from);
    const double zc = dot(e, T.cam.fwd);
    const double xc = dot(e, T.cam.right) / zc, yc = dot(e, T.cam.up) / zc;
    const double fx = T.W > 1 ? ((xc + T.cam.cw / 2.0) / T.cam.cw) * (double)(T.W - 1) : 0.0;
    const double fy = T.H > 1 ? ((T.cam.ch / 2.0 - yc) / T.cam.ch) * (double)(T.H - 1) : 0.0;
    if (!(zc > 0.0 && fx > -1.0 && fx < (double)T.W && fy > -1.0 && fy < (double)T.H)) return r;
    const double xf = floor(fx), yf = floor(fy);
    const double ax = fx - xf, ay = fy - yf;
    const int32_t x0 = (int32_t)xf, y0 = (int32_t)yf;
    if constexpr (!MOTION) id = T.hit_id[ip];
    const double tp = T.depth[ip];
    const double wt[4] = {(1.0 - ax) * (1.0 - ay), ax * (1.0 - ay), (1.0 - ax) * ay, ax * ay};
    double sw = 0.0, L = 0.0;
    d3 hA = d3{0.0, 0.0, 0.0}, hB = d3{0.0, 0.0, 0.0};
    for (int k = 0; k < 4; ++k) {
        const int32_t qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const double w = wt[k];
        if (qx < 0 || qx >= T.W || qy < 0 || qy >= T.H || !(w > 0.0)) continue;
        const int64_t q = (int64_t)qy * T.W + qx;
        const double lq = T.hist_len[q];
        if (!(lq >= 1.0) || T.hist_hit_id[q] != id) continue;
        if (!(dn_sq(sub(np, dn_ld3(T.hist_normal, n, q))) <= T.normal_max)) continue;
        if (!(fabs(dot(np, sub(dn_ld3(T.hist_position, n, q), xp))) / tp <= T.plane_max)) continue;
        sw += w;
        hA = add(hA, mul(dn_ld3(T.hist_a, n, q), w));
        hB = add(hB, mul(dn_ld3(T.hist_b, n, q), w));
        L += w * lq;
    }
    if (!(sw >= 0.01)) return r;
    hA = divs(hA, sw);
    hB = divs(hB, sw);
    L = L / sw;
    const double N = L + 1.0 < T.max_history ? L + 1.0 : T.max_history;
    const double alpha = 1.0 / N;
    r.hist_a = add(hA, mul(sub(r.hist_a, hA), alpha));
    r.hist_b = add(hB, mul(sub(r.hist_b, hB), alpha));
    r.len = N;
    r.a = T.demod ? mul(r.hist_a, d) : r.hist_a;
    r.b = T.demod ? mul(r.hist_b, d) : r.hist_b;
    return r;
}

// out_srgb8 of one pixel: resolve_pixel, k_resolve's rule
RT_HD uint32_t denoise_resolve(d3 c) {
    uint8_t px[3];
    double a0, a1, a2;
    resolve_pixel(c.x, c.y, c.z, a0, a1, a2, px);
    return (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | 0xFF000000u;
}

#if defined(__HIPCC__)
constexpr int DN_BLOCK = 256;

struct AovOut {
    int32_t* hit_id;
    double *depth, *position, *normal, *albedo;
};

// one thread per pixel of the camera; cam.xs / cam.ys are device arrays
__global__ __launch_bounds__(DN_BLOCK) void k_aov(SceneView S, srt_camera cam, AovOut out, uint32_t* flags) {
    const int64_t n = (int64_t)cam.width * cam.height;
    uint32_t err = 0;
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * DN_BLOCK) {
        const int64_t row = i / cam.width, col = i - row * cam.width;
        const AovPixel r = aov_pixel(S, cam, cam.xs[col], cam.ys[row], err);
        if (out.hit_id) out.hit_id[i] = r.id;
        if (out.depth) out.depth[i] = r.t;
        if (out.position) { out.position[i] = r.P.x; out.position[n + i] = r.P.y; out.position[2 * n + i] = r.P.z; }
        if (out.normal) { out.normal[i] = r.N.x; out.normal[n + i] = r.N.y; out.normal[2 * n + i] = r.N.z; }
        if (out.albedo) { out.albedo[i] = r.A.x; out.albedo[n + i] = r.A.y; out.albedo[2 * n + i] = r.A.z; }
    }
    if (err) atomicOr(flags, err);
}

// One filter level.  A wave takes 64 consecutive pixels of one row (work item = row * segs + segment),
// so each of the 25 taps of each plane is one contiguous row segment; the taps read global memory and
// the caches absorb the reuse between neighbouring pixels and rows.  (A variant that staged 64 x 4 pixel
// tiles and their halo in LDS for steps 1 and 2 gave the same bits and was slower)
template <bool VAR>
__global__ __launch_bounds__(DN_BLOCK) void k_atrous(AtrousPlanes G, AtrousLevel K, double* out, AtrousVar V) {
    const int64_t segs = (K.W + 63) / 64, items = segs * K.H;
    const int lane = threadIdx.x & 63;
    constexpr int WAVES = DN_BLOCK / 64;
    for (int64_t it = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * WAVES) {
        const int64_t y = it / segs;
        const int64_t x = (it - y * segs) * 64 + lane;
        if (x >= K.W) continue;
        double v;
        const d3 c = atrous_pixel<VAR>(G, K, V, (int32_t)x, (int32_t)y, v);
        const int64_t ip = y * K.W + x;
        out[ip] = c.x;
        out[G.npix + ip] = c.y;
        out[2 * G.npix + ip] = c.z;
        if constexpr (VAR) V.v_out[ip] = v;
    }
}

// u and v of the half-frames (header comment); `v` may be NULL (no SRT_DENOISE_VARIANCE).  One thread per
// pixel, streaming: 12 planes in, 3 or 4 out
__global__ __launch_bounds__(DN_BLOCK) void k_dn_prepare(DnHalves F, const double* normal, const double* albedo, int64_t n,
                                                         double* u, double* v) {
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * DN_BLOCK) {
        const DnPrepared r = dn_prepare_pixel(F, dn_ld3(F.a, n, i), dn_ld3(F.b, n, i), dn_ld3(normal, n, i),
                                              dn_ld3(albedo, n, i));
        u[i] = r.u.x;
        u[n + i] = r.u.y;
        u[2 * n + i] = r.u.z;
        if (v) v[i] = r.v;
    }
}

// c' = u' * d in place over `rgb` and, with `u8`, the resolved image (as k_denoise_resolve)
__global__ __launch_bounds__(DN_BLOCK) void k_dn_finish(DnHalves F, const double* normal, const double* albedo, int64_t n,
                                                        double* rgb, uint8_t* u8, int rgbx) {
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * DN_BLOCK) {
        const d3 c = dn_finish_pixel(dn_ld3(rgb, n, i), dn_ld3(F.a, n, i), dn_ld3(F.b, n, i), dn_ld3(normal, n, i),
                                     dn_ld3(albedo, n, i));
        rgb[i] = c.x;
        rgb[n + i] = c.y;
        rgb[2 * n + i] = c.z;
        if (!u8) continue;
        const uint32_t px = denoise_resolve(c);
        if (rgbx) {
            reinterpret_cast<uint32_t*>(u8)[i] = px;
        } else {
            u8[3 * i] = (uint8_t)px;
            u8[3 * i + 1] = (uint8_t)(px >> 8);
            u8[3 * i + 2] = (uint8_t)(px >> 16);
        }
    }
}

struct TemporalOut {
    double *a, *b, *hist_a, *hist_b;  // [3][npix] each
    double* len;                      // [npix]
};

// Temporal accumulation of the two half-frames (header comment).  Work items as in k_atrous: a wave takes 64
// consecutive pixels of one row, so the streaming reads and the 13 planar stores are coalesced, and the four
// gathered history taps of neighbouring lanes fall in the same one or two row segments of the previous frame.
// One item per wave and no grid-stride loop (the grid is ceil(items / waves per block) blocks): with the loop the
// 18 plane pointers and the camera stay live across it and 88 SGPRs spill; without it none does
// (profiles/temporal_resource_usage.txt).  No LDS, no atomics.  out.a / out.b may be the planes T.a / T.b
// themselves (a pixel reads only its own A, B); the out.hist_* planes must not be the T.hist_* planes, which
// other pixels gather from.  MOTION: each lane also loads the 12 doubles of its collider's row of T.motion (ordinary
// vector loads of a table of a few KB, which the caches hold) and spends 18 multiply-adds on x' and n'
// (profiles/temporal_motion_resource_usage.txt).
template <bool MOTION>
__global__ __launch_bounds__(DN_BLOCK) void k_temporal(TemporalPlanes T, TemporalOut out) {
    const int64_t segs = (T.W + 63) / 64, items = segs * T.H;
    constexpr int WAVES = DN_BLOCK / 64;
    const int64_t it = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (it >= items) return;
    const int64_t y = it / segs;
    const int64_t x = (it - y * segs) * 64 + (threadIdx.x & 63);
    if (x >= T.W) return;
    const int64_t n = T.npix;
    const TemporalPixel r = temporal_pixel<MOTION>(T, (int32_t)x, (int32_t)y);
    const int64_t ip = y * T.W + x;
    out.a[ip] = r.a.x; out.a[n + ip] = r.a.y; out.a[2 * n + ip] = r.a.z;
    out.b[ip] = r.b.x; out.b[n + ip] = r.b.y; out.b[2 * n + ip] = r.b.z;
    out.hist_a[ip] = r.hist_a.x; out.hist_a[n + ip] = r.hist_a.y; out.hist_a[2 * n + ip] = r.hist_a.z;
    out.hist_b[ip] = r.hist_b.x; out.hist_b[n + ip] = r.hist_b.y; out.hist_b[2 * n + ip] = r.hist_b.z;
    out.len[ip] = r.len;
}

// out_srgb8 of the filtered frame: [n][3], or [n][4] (R, G, B, 255) with SRT_DENOISE_RGBX
__global__ __launch_bounds__(DN_BLOCK) void k_denoise_resolve(const double* rgb, int64_t n, uint8_t* u8, int rgbx) {
    for (int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * DN_BLOCK) {
        const uint32_t v = denoise_resolve(d3{rgb[i], rgb[n + i], rgb[2 * n + i]});
        if (rgbx) {
            reinterpret_cast<uint32_t*>(u8)[i] = v;
        } else {
            u8[3 * i] = (uint8_t)v;
            u8[3 * i + 1] = (uint8_t)(v >> 8);
            u8[3 * i + 2] = (uint8_t)(v >> 16);
        }
    }
}
#endif  // __HIPCC__

}  // namespace rt
#endif  // RT_DENOISE_H
