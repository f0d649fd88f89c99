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

RT_HD bool dn_finite(double v) { return v - v == 0.0; }
RT_HD bool dn_finite3(d3 v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z); }
RT_HD double dn_sq(d3 v) { return (v.x * v.x + v.y * v.y) + v.z * v.z; }

// c'_p of pixel (x, y).  The dy loop's bounds test is the same for every pixel of a row (wave-uniform on
// the device); a tap outside the row reads the clamped column and weighs nothing.
RT_HD d3 atrous_pixel(const AtrousPlanes& G, const AtrousLevel& K, int32_t x, int32_t y) {
    const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    const AtrousTap p = G.tap(y, x);
    if (is_zero(p.n) || !dn_finite3(p.c)) return p.c;
    const double tp = G.depth[(int64_t)y * G.W + x];
    double sw = 0.0;
    d3 sc = d3{0.0, 0.0, 0.0};
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
                const double tc = dn_sq(sub(p.c, q.c)) / K.sc2;
                const double tn = dn_sq(sub(p.n, q.n)) / K.sn2;
                const double ta = dn_sq(sub(p.a, q.a)) / K.sa2;
                const double e = fabs(dot(p.n, sub(q.x, p.x))) / tp;
                const double tpl = (e * e) / K.sp2;
                w = hh * exp(-(((tc + tn) + ta) + tpl));
            }
            sw += w;
            sc = add(sc, mul(q.c, w));
        }
    }
    return divs(sc, sw);
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
__global__ __launch_bounds__(DN_BLOCK) void k_atrous(AtrousPlanes G, AtrousLevel K, double* out) {
    const int64_t segs = (K.W + 63) / 64, items = segs * K.H;
    const int lane = threadIdx.x & 63;
    constexpr int WAVES = DN_BLOCK / 64;
    for (int64_t it = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < items; it += (int64_t)gridDim.x * WAVES) {
        const int64_t y = it / segs;
        const int64_t x = (it - y * segs) * 64 + lane;
        if (x >= K.W) continue;
        const d3 c = atrous_pixel(G, K, (int32_t)x, (int32_t)y);
        const int64_t ip = y * K.W + x;
        out[ip] = c.x;
        out[G.npix + ip] = c.y;
        out[2 * G.npix + ip] = c.z;
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
