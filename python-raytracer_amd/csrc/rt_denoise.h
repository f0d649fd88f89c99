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

RT_HDM d3 dn_ld3(const double* p, int64_t n, int64_t i) { return d3{p[i], p[n + i], p[2 * n + i]}; }

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
