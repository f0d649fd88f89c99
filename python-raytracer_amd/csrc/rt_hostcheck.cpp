// rt_hostcheck.cpp -- TEST HARNESS ONLY (tests/_build/libsightpy_hostcheck.so).
//
// A sequential, breadth-first CPU driver over the *same* per-ray functions the gfx950 kernels
// use (rt_device.h), compiled by g++ with -ffp-contract=off.  It lets the CPU test suite check
// the kernel math against the numpy oracle in a container without a GPU.  It is never loaded by
// the product package (sightpy/_native.py loads only libsightpy_hip.so and fails loudly without
// it); it mirrors the kernel's RNG keys and child-path hashing, so Monte-Carlo scenes give the
// same samples as the GPU path up to transcendental-function ulps.
#include <cstring>
#include <string>
#include <vector>

#include "rt_bvh.h"
#include "rt_denoise.h"
#include "rt_device.h"
#include "rt_mt.h"
#include "rt_pose.h"
#include "rt_deform.h"

using namespace rt;

namespace {

thread_local std::string g_err;

struct Scene {
    SceneView S{};
    int max_depth = 0;
    int has_diffuse = 0;
};

thread_local BvhBuild g_bvh;  // the BVH of the scene of the current call
thread_local int g_use_bvh = 1;
thread_local bool g_vattr = false;  // the scene of the current call has SRT_CF_VNORMAL / SRT_CF_VUV triangles
thread_local bool g_plight = false;  // ... has an SRT_LIGHT_POSITIONAL light
thread_local std::vector<srt_light> g_lights;  // its light table as the kernels read it (pack_lights)
// rows of the current hc_render (null: identity / hc_trace): Monte-Carlo draws are keyed by the
// global pixel, as key_pix in rt_trace_common.h
thread_local const int32_t* g_rows = nullptr;
thread_local int64_t g_width = 0;

uint32_t key_pix(uint32_t pix) {
    if (!g_rows) return pix;
    const uint32_t W = (uint32_t)g_width, lr = pix / W;
    return (uint32_t)g_rows[lr] * W + (pix - lr * W);
}

SceneView view_of(const srt_scene_desc* d) {
    SceneView S{};
    if (g_use_bvh) {
        bvh_build(d->colliders, d->n_colliders, g_bvh);
    } else {
        g_bvh = BvhBuild{};
        for (int i = 0; i < d->n_colliders; ++i) g_bvh.lin.push_back(i);
    }
    S.nlin = (int)g_bvh.lin.size();
    S.lin = g_bvh.lin.data();
    S.bvh = g_bvh.nodes.empty() ? nullptr : g_bvh.nodes.data();
    S.bvh_tri = g_bvh.tri.empty() ? nullptr : g_bvh.tri.data();
    S.bvh_nodes = (int)g_bvh.nodes.size();
    S.bvh_bound = g_bvh.bound;
    S.col = d->colliders; S.mat = d->materials; S.tex = d->textures; S.texels = d->texels;
    g_lights.assign((size_t)(d->n_lights > 0 ? d->n_lights : 0), srt_light{});  // (the kernels' layout, as the upload's)
    if (d->n_lights > 0) pack_lights(d->lights, d->n_lights, g_lights.data());
    S.lights = reinterpret_cast<const DevLight*>(g_lights.data()); S.media = d->media; S.glossy_f0 = d->glossy_f0; S.light_local = d->light_local;
    S.importance = d->importance;
    S.ncol = d->n_colliders; S.nmat = d->n_materials; S.ntex = d->n_textures; S.nlights = d->n_lights;
    S.nmedia = d->n_media; S.nimp = d->n_importance;
    S.sky_col = sky_collider(d->colliders, d->n_colliders, d->materials);
    S.nshadow = 0;
    g_vattr = false;
    for (int i = 0; i < d->n_colliders; ++i) {
        if (d->colliders[i].flags & SRT_CF_SHADOW) S.nshadow++;
        // (the feature scan of srt_upload_scene: the shaders' MAT_VATTR instantiation)
        if (d->colliders[i].type == SRT_TRIANGLE && (d->colliders[i].flags & (SRT_CF_VNORMAL | SRT_CF_VUV)))
            g_vattr = true;
    }
    g_plight = false;  // (as the scan sets MAT_PLIGHT)
    for (int i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type == SRT_LIGHT_POSITIONAL) g_plight = true;
    for (int k = 0; k < 3; ++k) S.ambient[k] = d->ambient[k];
    return S;
}

int depth_cap(const srt_scene_desc* d) {
    int diff = 0;
    for (int i = 0; i < d->n_materials; ++i)
        if (d->materials[i].type == SRT_DIFFUSE) diff = 1;
    return d->max_ray_depth + 1 + (diff ? 2 : 0);
}

struct HostEmit {
    const SceneView& S;
    const Ray& r;
    std::vector<Ray>& next;
    double* fb;
    int64_t npix;
    uint64_t seed;
    int depth;
    uint32_t round;
    int64_t* sh;

    void local(d3 c) const {
        if (is_zero(c)) return;
        fb[r.pix] += r.w.x * c.x;
        fb[npix + r.pix] += r.w.y * c.y;
        fb[2 * npix + r.pix] += r.w.z * c.z;
    }
    void shadow(int n) const { *sh += n; }
    void push(const Child& c, uint32_t path) const {
        Ray k;
        k.o = c.o; k.d = c.d; k.w = mul(r.w, c.w);
        k.pix = r.pix;
        k.meta = pack_meta(c.medium, meta_depth(r.meta) + 1, c.dfl);
        k.path = path;
        next.push_back(k);
    }
    void child(const Child& c) const { push(c, child_path(r.path, c.slot, round)); }
    void diffuse(const DiffuseGen& g, int mi) const {
        for (int k = 0; k < g.count; ++k) {
            Rng rng;
            const uint32_t cpath = child_path(r.path, 0x100u + (uint32_t)k, round);
            rng.init(seed, key_pix(r.pix), cpath, 0xD1000000u | (uint32_t)depth);
            push(diffuse_child(S, S.mat[mi], g, rng, (uint32_t)k), cpath);
        }
    }
};

double mc_uniform(const SceneView& S, uint64_t seed, int depth, const Ray& r, int cid, uint32_t round) {
    if (!(S.col[cid].flags & SRT_CF_MC)) return 0.0;
    Rng g;
    g.init(seed, key_pix(r.pix), r.path, 0x3C000000u | ((uint32_t)depth << 8) | round);
    return g.one();
}

template <uint32_t MATS>
void trace_one_feat(const SceneView& S, const Ray& r, int depth, uint64_t seed, std::vector<Ray>& next, double* fb,
                    int64_t npix, uint32_t& err, int64_t& shadow, int32_t* hit_slot) {
    double t, o;
    bool ties;
    int id = nearest_hit(S, r.o, r.d, t, o, ties);
    if (hit_slot) *hit_slot = id;
    if (id < 0) return;
    HostEmit em{S, r, next, fb, npix, seed, depth, 0u, &shadow};
    shade_hit<MATS>(S, id, S.col[id].material, r, t, o, em, err, mc_uniform(S, seed, depth, r, id, 0));
    if (ties) {
        uint32_t round = 1;
        for (int c = id + 1; c < S.ncol; ++c) {
            double oc;
            if (collider_hit(S.col[c], r.o, r.d, oc) == t) {
                HostEmit et{S, r, next, fb, npix, seed, depth, round, &shadow};
                shade_hit<MATS>(S, c, S.col[c].material, r, t, oc, et, err, mc_uniform(S, seed, depth, r, c, round));
                ++round;
            }
        }
    }
}

void trace_one(const SceneView& S, const Ray& r, int depth, uint64_t seed, std::vector<Ray>& next, double* fb,
               int64_t npix, uint32_t& err, int64_t& shadow, int32_t* hit_slot) {
    if (g_plight)  // (never with g_vattr: refused at lowering, as srt_upload_scene refuses it)
        trace_one_feat<MAT_GENERIC | MAT_BVH | MAT_PLIGHT>(S, r, depth, seed, next, fb, npix, err, shadow, hit_slot);
    else if (g_vattr)
        trace_one_feat<MAT_GENERIC | MAT_BVH | MAT_VATTR>(S, r, depth, seed, next, fb, npix, err, shadow, hit_slot);
    else
        trace_one_feat<MAT_GENERIC | MAT_BVH>(S, r, depth, seed, next, fb, npix, err, shadow, hit_slot);
}

int err_code(uint32_t e) {
    if (e & ERR_INDEX) { g_err = "index out of bounds in a texture/table lookup"; return SRT_ERR_INDEX; }
    if (e & ERR_UNSUPPORTED) { g_err = "uv requested on a Triangle"; return SRT_ERR_ARG; }
    if (e & ERR_NAME) { g_err = "name 'M' is not defined (PointLight.get_L)"; return SRT_ERR_NAME; }
    return SRT_OK;
}

}  // namespace

extern "C" {

const char* hc_last_error(void) { return g_err.c_str(); }

// 1: triangle colliders of large meshes go through the BVH (as on the GPU); 0: linear loop only
void hc_set_bvh(int on) { g_use_bvh = on; }
int hc_bvh_nodes(const srt_scene_desc* d) {
    BvhBuild b;
    bvh_build(d->colliders, d->n_colliders, b);
    return (int)b.nodes.size();
}

// Breadth-first render of `args->spp` samples (host pointers only); out_rgb = linear RGB / spp.
int hc_render(const srt_scene_desc* d, const srt_camera* cam, const srt_render_args* a, srt_stats* st) {
    SceneView S = view_of(d);
    const int64_t W = cam->width, npix = (int64_t)a->n_rows * W;
    std::vector<double> fb(3 * npix, 0.0);
    uint32_t err = 0;
    int64_t shadow = 0;
    srt_stats stats{};
    const int dcap = depth_cap(d);
    g_rows = a->rows;
    g_width = W;
    for (int s = 0; s < a->spp; ++s) {
        std::vector<Ray> cur, next;
        for (int64_t p = 0; p < npix; ++p) {
            int64_t lr = p / W, col = p % W;
            int grow = a->rows ? a->rows[lr] : (int)lr;
            double j[4];
            if (a->jitter) {
                const double* b = a->jitter + (int64_t)s * 4 * npix + p;
                j[0] = b[0]; j[1] = b[npix]; j[2] = b[2 * npix]; j[3] = b[3 * npix];
            } else {
                Rng g;
                g.init(a->seed, (uint32_t)(grow * W + col), (uint32_t)(a->sample_base + s), 0xCA3E0000u);
                g.two(j[0], j[1]);
                g.two(j[2], j[3]);
            }
            Ray r;
            primary_ray(*cam, cam->xs[col], cam->ys[grow], j, r.o, r.d);
            r.w = d3{1.0, 1.0, 1.0};
            r.pix = (uint32_t)p;
            r.meta = pack_meta(0, 0, 0);
            r.path = mix32(0x5EED0000u, (uint32_t)(a->sample_base + s));
            int32_t* hs = a->out_hit_id ? a->out_hit_id + (int64_t)s * npix + p : nullptr;
            trace_one(S, r, 0, a->seed, next, fb.data(), npix, err, shadow, hs);
        }
        stats.rays_per_depth[0] += npix;
        for (int dpt = 1; dpt <= dcap && !next.empty(); ++dpt) {
            cur.swap(next);
            next.clear();
            stats.rays_per_depth[dpt] += (int64_t)cur.size();
            for (const Ray& r : cur) trace_one(S, r, dpt, a->seed, next, fb.data(), npix, err, shadow, nullptr);
        }
        if (!next.empty()) { g_err = "rays alive after the depth cap"; return SRT_ERR_DEPTH; }
    }
    if (int rc = err_code(err)) return rc;
    for (int64_t p = 0; p < npix; ++p) {
        double r = fb[p] / a->spp, g = fb[npix + p] / a->spp, b = fb[2 * npix + p] / a->spp;
        uint8_t px[3];
        double q0, q1, q2;
        resolve_pixel(r, g, b, q0, q1, q2, px);
        if (a->out_rgb) { a->out_rgb[p] = r; a->out_rgb[npix + p] = g; a->out_rgb[2 * npix + p] = b; }
        if (a->out_srgb8) { a->out_srgb8[3 * p] = px[0]; a->out_srgb8[3 * p + 1] = px[1]; a->out_srgb8[3 * p + 2] = px[2]; }
    }
    stats.n_depths = dcap + 1;
    for (int k = 0; k <= dcap; ++k) stats.total_rays += stats.rays_per_depth[k];
    stats.shadow_rays = shadow;
    stats.passes = 1;
    if (st) *st = stats;
    return SRT_OK;
}

int hc_trace(const srt_scene_desc* d, const srt_trace_args* a, srt_stats* st) {
    SceneView S = view_of(d);
    g_rows = nullptr;
    const int64_t n = a->n;
    std::vector<double> fb(3 * n, 0.0);
    std::vector<Ray> cur, next;
    for (int64_t i = 0; i < n; ++i) {
        Ray r;
        r.o = d3{a->origin[i], a->origin[n + i], a->origin[2 * n + i]};
        r.d = d3{a->dir[i], a->dir[n + i], a->dir[2 * n + i]};
        r.w = d3{1.0, 1.0, 1.0};
        r.pix = (uint32_t)i;
        r.meta = pack_meta(a->medium ? (uint32_t)a->medium[i] : 0u, (uint32_t)a->depth, (uint32_t)a->diffuse_reflections);
        r.path = mix32(0x7A11u, (uint32_t)i);
        cur.push_back(r);
    }
    uint32_t err = 0;
    int64_t shadow = 0;
    srt_stats stats{};
    const int dlast = a->depth + depth_cap(d);
    for (int dpt = a->depth; dpt <= dlast && !cur.empty(); ++dpt) {
        stats.rays_per_depth[dpt] = (int64_t)cur.size();
        next.clear();
        for (const Ray& r : cur) trace_one(S, r, dpt, a->seed, next, fb.data(), n, err, shadow, nullptr);
        cur.swap(next);
    }
    if (!cur.empty()) { g_err = "rays alive after the depth cap"; return SRT_ERR_DEPTH; }
    if (int rc = err_code(err)) return rc;
    std::memcpy(a->out_rgb, fb.data(), 3 * n * sizeof(double));
    stats.n_depths = dlast + 1;
    for (int k = 0; k < SRT_MAX_DEPTHS; ++k) stats.total_rays += stats.rays_per_depth[k];
    stats.shadow_rays = shadow;
    if (st) *st = stats;
    return SRT_OK;
}

// the nearest hit of each of the n rays (O, D: three planes of n) in `S`; each output may be NULL
static int nearest_all(const SceneView& S, const double* O, const double* D, int64_t n, double* t, int32_t* id,
                       double* orient) {
    for (int64_t i = 0; i < n; ++i) {
        double tn, on;
        bool ties;
        int c = nearest_hit(S, d3{O[i], O[n + i], O[2 * n + i]}, d3{D[i], D[n + i], D[2 * n + i]}, tn, on, ties);
        if (t) t[i] = tn;
        if (id) id[i] = c;
        if (orient) orient[i] = on;
    }
    return SRT_OK;
}

int hc_nearest(const srt_scene_desc* d, const double* O, const double* D, int64_t n, double* t, int32_t* id,
               double* orient) {
    return nearest_all(view_of(d), O, D, n, t, id, orient);
}

int hc_intersect_collider(const srt_collider* c, const double* O, const double* D, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) {
        double o;
        out[i] = collider_hit(*c, d3{O[i], O[n + i], O[2 * n + i]}, d3{D[i], D[n + i], D[2 * n + i]}, o);
        out[n + i] = o;
    }
    return SRT_OK;
}

// k_collider_surface: Collider.get_Normal (N [3][n]) and get_uv (uv [2][n]) at points P [3][n]; the uv of
// a Triangle without SRT_CF_VUV is undefined (SRT_ERR_ARG, as srt_collider_surface)
int hc_collider_surface(const srt_collider* c, const double* P, int64_t n, double* N, double* uv) {
    if (uv && c->type == SRT_TRIANGLE && !(c->flags & SRT_CF_VUV)) {
        g_err = "Triangle uv is undefined in the reference (triangle.py:79-83)";
        return SRT_ERR_ARG;
    }
    for (int64_t i = 0; i < n; ++i) {
        const d3 p = d3{P[i], P[n + i], P[2 * n + i]};
        if (N) {
            const d3 v = collider_normal<MAT_VATTR>(*c, p);
            N[i] = v.x; N[n + i] = v.y; N[2 * n + i] = v.z;
        }
        if (uv) {
            double u = 0.0, v = 0.0;
            collider_uv<MAT_VATTR>(*c, p, u, v);
            uv[i] = u; uv[n + i] = v;
        }
    }
    return SRT_OK;
}

int hc_primary_rays(const srt_camera* cam, const double* J, double* O, double* D) {
    const int64_t n = (int64_t)cam->width * cam->height;
    for (int64_t i = 0; i < n; ++i) {
        int64_t row = i / cam->width, col = i % cam->width;
        double j[4] = {J[i], J[n + i], J[2 * n + i], J[3 * n + i]};
        d3 o, d;
        primary_ray(*cam, cam->xs[col], cam->ys[row], j, o, d);
        O[i] = o.x; O[n + i] = o.y; O[2 * n + i] = o.z;
        D[i] = d.x; D[n + i] = d.y; D[2 * n + i] = d.z;
    }
    return SRT_OK;
}

// k_aov: the first-hit guide images (rt_denoise.h aov_pixel), host pointers; any output may be NULL
int hc_aovs(const srt_scene_desc* d, const srt_camera* cam, srt_aov_out* out) {
    SceneView S = view_of(d);
    const int64_t n = (int64_t)cam->width * cam->height;
    uint32_t err = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t row = i / cam->width, col = i % cam->width;
        const AovPixel r = aov_pixel(S, *cam, cam->xs[col], cam->ys[row], err);
        if (out->hit_id) out->hit_id[i] = r.id;
        if (out->depth) out->depth[i] = r.t;
        if (out->position) { out->position[i] = r.P.x; out->position[n + i] = r.P.y; out->position[2 * n + i] = r.P.z; }
        if (out->normal) { out->normal[i] = r.N.x; out->normal[n + i] = r.N.y; out->normal[2 * n + i] = r.N.z; }
        if (out->albedo) { out->albedo[i] = r.A.x; out->albedo[n + i] = r.A.y; out->albedo[2 * n + i] = r.A.z; }
    }
    return err_code(err);
}

// srt_denoise: the levels of k_atrous one after the other over two colour buffers, then k_denoise_resolve
int hc_denoise(int32_t width, int32_t height, const srt_denoise_args* a) {
    if (width <= 0 || height <= 0 || !a->rgb || !a->normal || !a->albedo || !a->position || !a->depth ||
        a->levels < 0 || a->levels > SRT_DENOISE_MAX_LEVELS || !(a->sigma_color > 0.0) || !(a->sigma_normal > 0.0) ||
        !(a->sigma_albedo > 0.0) || !(a->sigma_plane > 0.0)) {
        g_err = "hc_denoise: bad argument";
        return SRT_ERR_ARG;
    }
    const int64_t n = (int64_t)width * height;
    AtrousPlanes G{a->rgb, a->normal, a->albedo, a->position, a->depth, n, width};
    std::vector<double> pong[2];
    for (int l = 0; l < a->levels; ++l) {
        AtrousLevel K{};
        K.W = width, K.H = height, K.step = 1 << l;
        const double sc = a->sigma_color * ldexp(1.0, -l);
        K.sc2 = sc * sc;
        K.sn2 = a->sigma_normal * a->sigma_normal;
        K.sa2 = a->sigma_albedo * a->sigma_albedo;
        K.sp2 = a->sigma_plane * a->sigma_plane;
        std::vector<double>& o = pong[l & 1];
        o.resize((size_t)(3 * n));
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) {
                double v;
                const d3 c = atrous_pixel<false>(G, K, AtrousVar{}, x, y, v);
                const int64_t ip = (int64_t)y * width + x;
                o[(size_t)ip] = c.x; o[(size_t)(n + ip)] = c.y; o[(size_t)(2 * n + ip)] = c.z;
            }
        G.rgb = o.data();
    }
    const bool rgbx = (a->flags & SRT_DENOISE_RGBX) != 0;
    if (a->out_srgb8)
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t v = denoise_resolve(d3{G.rgb[i], G.rgb[n + i], G.rgb[2 * n + i]});
            uint8_t* px = a->out_srgb8 + (rgbx ? 4 : 3) * i;
            px[0] = (uint8_t)v; px[1] = (uint8_t)(v >> 8); px[2] = (uint8_t)(v >> 16);
            if (rgbx) px[3] = 255;
        }
    if (a->out_rgb) std::memmove(a->out_rgb, G.rgb, (size_t)(3 * n) * sizeof(double));
    return SRT_OK;
}

// srt_denoise_var: k_dn_prepare, the levels of k_atrous<VAR> over two colour (and variance) buffers,
// k_dn_finish / k_denoise_resolve
int hc_denoise_var(int32_t width, int32_t height, const srt_denoise_var_args* a) {
    const bool var = (a->flags & SRT_DENOISE_VARIANCE) != 0, demod = (a->flags & SRT_DENOISE_DEMODULATE) != 0;
    if (width <= 0 || height <= 0 || !a->rgb_a || !a->rgb_b || !a->normal || !a->albedo || !a->position || !a->depth ||
        a->spp_a <= 0 || a->spp_b <= 0 || a->levels < 0 || a->levels > SRT_DENOISE_MAX_LEVELS ||
        (a->flags & ~(SRT_DENOISE_RGBX | SRT_DENOISE_VARIANCE | SRT_DENOISE_DEMODULATE)) ||
        !((var ? a->sigma_lum : a->sigma_color) > 0.0) || !(a->sigma_normal > 0.0) || !(a->sigma_albedo > 0.0) ||
        !(a->sigma_plane > 0.0) || (!a->out_rgb && !a->out_srgb8) || (a->out_variance && !var)) {
        g_err = "hc_denoise_var: bad argument";
        return SRT_ERR_ARG;
    }
    const int64_t n = (int64_t)width * height;
    DnHalves F{a->rgb_a, a->rgb_b, (double)a->spp_a, (double)a->spp_b, (double)a->spp_a + (double)a->spp_b, demod ? 1 : 0};
    const auto at = [n](const double* p, int64_t i) { return d3{p[i], p[n + i], p[2 * n + i]}; };
    std::vector<double> cb[2], vb[2];
    for (int k = 0; k < 2; ++k) {
        cb[k].resize((size_t)(3 * n));
        vb[k].resize((size_t)n);
    }
    for (int64_t i = 0; i < n; ++i) {
        const DnPrepared r = dn_prepare_pixel(F, at(F.a, i), at(F.b, i), at(a->normal, i), at(a->albedo, i));
        cb[0][(size_t)i] = r.u.x; cb[0][(size_t)(n + i)] = r.u.y; cb[0][(size_t)(2 * n + i)] = r.u.z;
        vb[0][(size_t)i] = r.v;
    }
    AtrousPlanes G{cb[0].data(), a->normal, a->albedo, a->position, a->depth, n, width};
    for (int l = 0; l < a->levels; ++l) {
        AtrousLevel K{};
        K.W = width, K.H = height, K.step = 1 << l;
        const double sc = a->sigma_color * ldexp(1.0, -l);
        K.sc2 = sc * sc;
        K.sn2 = a->sigma_normal * a->sigma_normal;
        K.sa2 = a->sigma_albedo * a->sigma_albedo;
        K.sp2 = a->sigma_plane * a->sigma_plane;
        std::vector<double>& o = cb[(l + 1) & 1];
        const AtrousVar V{vb[l & 1].data(), vb[(l + 1) & 1].data(), a->sigma_lum};
        for (int32_t y = 0; y < height; ++y)
            for (int32_t x = 0; x < width; ++x) {
                double v = 0.0;
                const d3 c = var ? atrous_pixel<true>(G, K, V, x, y, v) : atrous_pixel<false>(G, K, V, x, y, v);
                const int64_t ip = (int64_t)y * width + x;
                o[(size_t)ip] = c.x; o[(size_t)(n + ip)] = c.y; o[(size_t)(2 * n + ip)] = c.z;
                V.v_out[ip] = v;
            }
        G.rgb = o.data();
    }
    double* res = cb[a->levels & 1].data();
    if (demod)
        for (int64_t i = 0; i < n; ++i) {
            const d3 c = dn_finish_pixel(at(res, i), at(F.a, i), at(F.b, i), at(a->normal, i), at(a->albedo, i));
            res[i] = c.x; res[n + i] = c.y; res[2 * n + i] = c.z;
        }
    const bool rgbx = (a->flags & SRT_DENOISE_RGBX) != 0;
    if (a->out_srgb8)
        for (int64_t i = 0; i < n; ++i) {
            const uint32_t v = denoise_resolve(at(res, i));
            uint8_t* px = a->out_srgb8 + (rgbx ? 4 : 3) * i;
            px[0] = (uint8_t)v; px[1] = (uint8_t)(v >> 8); px[2] = (uint8_t)(v >> 16);
            if (rgbx) px[3] = 255;
        }
    if (a->out_rgb) std::memcpy(a->out_rgb, res, (size_t)(3 * n) * sizeof(double));
    if (a->out_variance) std::memcpy(a->out_variance, vb[a->levels & 1].data(), (size_t)n * sizeof(double));
    return SRT_OK;
}

// srt_temporal_accumulate: k_temporal's temporal_pixel over host arrays (the outputs may be rgb_a / rgb_b; they
// must not be the history arrays)
int hc_temporal(int32_t width, int32_t height, const srt_temporal_args* a) {
    const bool demod = (a->flags & SRT_TEMPORAL_DEMODULATE) != 0;
    if (width <= 0 || height <= 0 || a->max_history < 1 || !(a->normal_max >= 0.0) || !(a->plane_max >= 0.0) ||
        a->normal_max - a->normal_max != 0.0 || a->plane_max - a->plane_max != 0.0 ||
        (a->flags & ~SRT_TEMPORAL_DEMODULATE) || !a->rgb_a || !a->rgb_b || !a->hit_id || !a->position || !a->normal ||
        !a->depth || (demod && !a->albedo) || !a->out_a || !a->out_b || !a->out_hist_a || !a->out_hist_b || !a->out_len ||
        (a->hist_len && (!a->hist_a || !a->hist_b || !a->hist_hit_id || !a->hist_position || !a->hist_normal ||
                         !a->prev_cam || a->prev_cam->width != width || a->prev_cam->height != height ||
                         a->out_hist_a == a->hist_a || a->out_hist_b == a->hist_b || a->out_len == a->hist_len)) ||
        (a->motion && a->n_motion < 1)) {
        g_err = "hc_temporal: bad argument";
        return SRT_ERR_ARG;
    }
    const int64_t n = (int64_t)width * height;
    TemporalPlanes T{};
    T.a = a->rgb_a, T.b = a->rgb_b, T.hit_id = a->hit_id, T.position = a->position, T.normal = a->normal;
    T.albedo = a->albedo, T.depth = a->depth;
    if (a->hist_len) {
        T.hist_a = a->hist_a, T.hist_b = a->hist_b, T.hist_len = a->hist_len, T.hist_hit_id = a->hist_hit_id;
        T.hist_position = a->hist_position, T.hist_normal = a->hist_normal;
        T.cam = temporal_cam(*a->prev_cam);
    }
    T.npix = n, T.W = width, T.H = height;
    T.max_history = (double)a->max_history, T.normal_max = a->normal_max, T.plane_max = a->plane_max;
    T.demod = demod ? 1 : 0;
    const bool motion = a->motion && a->hist_len;  // a first frame ignores the table
    if (motion) T.motion = a->motion, T.n_motion = a->n_motion;
    for (int32_t y = 0; y < height; ++y)
        for (int32_t x = 0; x < width; ++x) {
            const TemporalPixel r = motion ? temporal_pixel<true>(T, x, y) : temporal_pixel<false>(T, x, y);
            const int64_t ip = (int64_t)y * width + x;
            a->out_a[ip] = r.a.x; a->out_a[n + ip] = r.a.y; a->out_a[2 * n + ip] = r.a.z;
            a->out_b[ip] = r.b.x; a->out_b[n + ip] = r.b.y; a->out_b[2 * n + ip] = r.b.z;
            a->out_hist_a[ip] = r.hist_a.x; a->out_hist_a[n + ip] = r.hist_a.y; a->out_hist_a[2 * n + ip] = r.hist_a.z;
            a->out_hist_b[ip] = r.hist_b.x; a->out_hist_b[n + ip] = r.hist_b.y; a->out_hist_b[2 * n + ip] = r.hist_b.z;
            a->out_len[ip] = r.len;
        }
    if (a->ms_kernel) *a->ms_kernel = 0.0;
    return SRT_OK;
}

// rt_device.h's Philox4x32-10 and path hash (known-answer tests of the Monte-Carlo stream)
void hc_philox(const uint32_t* ctr, uint32_t k0, uint32_t k1, uint32_t* out) {
    const u4 r = philox(u4{ctr[0], ctr[1], ctr[2], ctr[3]}, k0, k1);
    out[0] = r.a; out[1] = r.b; out[2] = r.c; out[3] = r.d;
}
uint32_t hc_mix32(uint32_t h, uint32_t v) { return mix32(h, v); }

// row-band shard map of the sharded render (rt_device.h): band height, owner rank and local row of
// global row y, with at most kmax bands per rank, dealt round-robin
int hc_shard_kmax(int64_t H, int n, int kmax, int fanout) { return shard_kmax(H, n, kmax, fanout); }
int64_t hc_shard_map(int64_t H, int n, int kmax, int32_t* owner, int64_t* local) {
    const int64_t h = shard_band_height(H, n, kmax);
    for (int64_t y = 0; y < H; ++y) {
        owner[y] = shard_of_row(y, n, h);
        local[y] = shard_local_row(y, n, h);
    }
    return h;
}

// numpy legacy rand stream by the segmented jump-ahead scheme of rt_mt.h, run serially
int hc_mt_uniforms(const uint32_t* key, int pos, int64_t n_out, int64_t n_skip, double* out, uint32_t* key_out,
                   int* pos_out) {
    if (pos < 0 || pos > rtmt::N || n_out < 0 || n_skip < 0 || n_out + n_skip == 0) return SRT_ERR_ARG;
    rtmt::uniforms_serial(key, pos, n_out, n_skip, out, key_out, pos_out);
    return SRT_OK;
}

// x^J mod phi (rt_mt.h xpow_mod), 624 words
void hc_xpow_mod(uint64_t J, uint32_t* out) {
    const std::vector<uint32_t> p = rtmt::xpow_mod(J);
    memcpy(out, p.data(), rtmt::N * 4);
}

// the window J words past `key` by the polynomial jump (rt_mt.h jump_serial with x^J)
void hc_jump_window(const uint32_t* key, uint64_t J, uint32_t* out) {
    const std::vector<uint32_t> p = rtmt::xpow_mod(J);
    rtmt::jump_serial(key, p.data(), out);
}

// ---- posed triangle meshes (rt_pose.h) ----
// the records rec[0, n) under one pose, as k_pose_triangles writes them
void hc_pose_triangles(const srt_collider* rec, int n, const double* pose, srt_collider* out) {
    for (int i = 0; i < n; ++i) pose_triangle_record(rec[i], pose, out[i]);
}

namespace {
// the boxes of the built tree `B` over the table `col` as it stands, height by height (k_bvh_refit's launches)
void refit_levels(BvhBuild& B, const srt_collider* col) {
    BvhLevels lv;
    bvh_levels(B.nodes, lv);
    for (size_t h = 0; h + 1 < lv.offset.size(); ++h)
        for (int j = lv.offset[h]; j < lv.offset[h + 1]; ++j)
            for (int k = 0; k < 4; ++k) bvh_refit_slot(B.nodes.data(), B.tri.data(), col, lv.nodes[j], k);
}

// srt_pose_colliders on the host: the table `col` as it stands is the rest shape; it is posed range by range, then
// the built tree `B` refitted and its bound set by the library's own rule (rt_pose.h); false for ranges the
// library refuses
bool pose_and_refit(int n_ranges, const int32_t* first, const int32_t* count, const double* poses,
                    std::vector<srt_collider>& col, BvhBuild& B) {
    const std::vector<srt_collider> rest = col;
    PoseLayout PL;
    if (!pose_layout_build(rest.data(), (int)rest.size(), n_ranges, first, count, PL).empty()) return false;
    for (int r = 0; r < n_ranges; ++r)
        for (int i = first[r]; i < first[r] + count[r]; ++i)
            pose_triangle_record(rest[i], poses + (size_t)r * POSE_DOUBLES, col[i]);
    if (B.nodes.empty()) return true;
    refit_levels(B, col.data());
    bool all_identity;
    B.bound = pose_layout_bound(PL, poses, B.bound, all_identity);
    return true;
}

// One mesh as srt_deform_topology registers it and srt_deform_colliders is handed it (host pointers).
struct HcDeform {
    int32_t first, count, n_verts;
    const int32_t* corner;
    const uint8_t* recompute;
    const double* center;
    const double* P;
};
// the three steps of srt_deform_colliders over rest[0, count) (the mesh's own records), in the kernels' order;
// false for a corner index outside [0, n_verts) (which the library refuses at registration)
bool deform_records(const HcDeform& h, const srt_collider* rest, srt_collider* out) {
    for (int j = 0; j < 3 * h.count; ++j)
        if (h.corner[j] < 0 || h.corner[j] >= h.n_verts) return false;
    std::vector<int32_t> offset, list;
    deform_csr(h.corner, h.count, h.n_verts, offset, list);
    std::vector<double> cross((size_t)3 * h.count, 0.0), sum((size_t)3 * h.n_verts, 0.0);
    DeformMesh M{};
    M.first = h.first, M.count = h.count, M.n_verts = h.n_verts;
    M.corner = h.corner, M.recompute = h.recompute, M.csr_offset = offset.data(), M.csr_corner = list.data();
    for (int k = 0; k < 3; ++k) M.center[k] = h.center[k];
    M.P = h.P, M.face_cross = cross.data(), M.vertex_sum = sum.data();
    for (int f = 0; f < h.count; ++f) deform_face_cross(M, f);
    for (int v = 0; v < h.n_verts; ++v) deform_vertex_sum(M, v);
    for (int f = 0; f < h.count; ++f) {
        srt_collider rec;
        deform_triangle_record(M, f, rest[f], rec);
        out[f] = rec;
    }
    return true;
}
// srt_deform_colliders on the host: the mesh's range of `col` rewritten, the built tree `B` refitted and its
// bound set by the library's own rule (rt_pose.h)
bool deform_and_refit(const HcDeform& h, std::vector<srt_collider>& col, BvhBuild& B) {
    if (h.first < 0 || h.count < 1 || (size_t)h.first + h.count > col.size()) return false;
    std::vector<srt_collider> rest(col.begin() + h.first, col.begin() + h.first + h.count);
    if (!deform_records(h, rest.data(), col.data() + h.first)) return false;
    if (B.nodes.empty()) return true;
    refit_levels(B, col.data());
    B.bound = rest_table_bound(col.data(), (int)col.size());
    return true;
}

// `d`'s table and tree `B` (as built) after an optional deformation (`h`, null: none) and then the poses of
// n_ranges ranges (0: none), as srt_pose_colliders would follow srt_deform_colliders
bool animate(const srt_scene_desc* d, const HcDeform* h, int n_ranges, const int32_t* first, const int32_t* count,
             const double* poses, std::vector<srt_collider>& col, BvhBuild& B) {
    col.assign(d->colliders, d->colliders + d->n_colliders);
    if (h && !deform_and_refit(*h, col, B)) return false;
    return n_ranges <= 0 || pose_and_refit(n_ranges, first, count, poses, col, B);
}

// hc_bvh_refit's and hc_deform_refit's outputs: the node count, or -1 for what the library refuses
int refit_out(const srt_scene_desc* d, const HcDeform* h, int n_ranges, const int32_t* first, const int32_t* count,
              const double* poses, void* nodes, int cap_nodes, int32_t* tri, int cap_tri, srt_collider* out,
              float* bound) {
    BvhBuild B;
    bvh_build(d->colliders, d->n_colliders, B);
    std::vector<srt_collider> col;
    if (!animate(d, h, n_ranges, first, count, poses, col, B)) return -1;
    if (nodes && !B.nodes.empty())
        memcpy(nodes, B.nodes.data(), sizeof(BvhNode) * (size_t)std::min<int>(cap_nodes, (int)B.nodes.size()));
    if (tri && !B.tri.empty()) memcpy(tri, B.tri.data(), 4 * (size_t)std::min<int>(cap_tri, (int)B.tri.size()));
    if (out && !col.empty()) memcpy(out, col.data(), sizeof(srt_collider) * col.size());
    if (bound) *bound = B.bound;
    return (int)B.nodes.size();
}

// hc_pose_nearest's and hc_deform_nearest's: hc_nearest on the animated scene, through the refitted BVH or
// (hc_set_bvh(0)) the linear loop over the rewritten table
int nearest_out(const srt_scene_desc* d, const HcDeform* h, int n_ranges, const int32_t* first, const int32_t* count,
                const double* poses, const double* O, const double* D, int64_t n, double* t, int32_t* id,
                double* orient) {
    SceneView S = view_of(d);
    std::vector<srt_collider> col;
    if (!animate(d, h, n_ranges, first, count, poses, col, g_bvh)) return -1;
    S.col = col.data();
    S.bvh_bound = g_bvh.bound;
    return nearest_all(S, O, D, n, t, id, orient);
}
}  // namespace

// The 4-wide nodes of `d`'s BVH after srt_pose_colliders' two steps on the host (n_ranges 0: as built).
// Returns the node count (-1 for ranges the library refuses); up to cap_nodes nodes (128 bytes each, rt_device.h
// BvhNode) go to `nodes`, up to cap_tri leaf slots (collider indices) to `tri`, the posed table (d->n_colliders
// records) to `posed`, the traversal's bound to `bound`; each may be NULL.
int hc_bvh_refit(const srt_scene_desc* d, int n_ranges, const int32_t* first, const int32_t* count,
                 const double* poses, void* nodes, int cap_nodes, int32_t* tri, int cap_tri, srt_collider* posed,
                 float* bound) {
    return refit_out(d, nullptr, n_ranges, first, count, poses, nodes, cap_nodes, tri, cap_tri, posed, bound);
}

// hc_nearest on the posed scene
int hc_pose_nearest(const srt_scene_desc* d, int n_ranges, const int32_t* first, const int32_t* count,
                    const double* poses, const double* O, const double* D, int64_t n, double* t, int32_t* id,
                    double* orient) {
    return nearest_out(d, nullptr, n_ranges, first, count, poses, O, D, n, t, id, orient);
}

// ---- deformed triangle meshes (rt_deform.h) ----
// The records rest[0, count) of a mesh under the vertex array P, as k_deform_triangles writes them (0, or -1 for
// a corner index outside [0, n_verts)).
int hc_deform_triangles(const srt_collider* rest, int count, int n_verts, const int32_t* corner,
                        const uint8_t* recompute, const double* center, const double* P, srt_collider* out) {
    return deform_records(HcDeform{0, count, n_verts, corner, recompute, center, P}, rest, out) ? 0 : -1;
}

// hc_bvh_refit for a deformed mesh: `d`'s BVH as built, the mesh [first, first + count) deformed and the tree
// refitted, then (n_ranges > 0) the ranges posed from the deformed table as srt_pose_colliders would after
// srt_deform_colliders.  Outputs as hc_bvh_refit's; -1 for a bad range or corner index.
int hc_deform_refit(const srt_scene_desc* d, int first, int count, int n_verts, const int32_t* corner,
                    const uint8_t* recompute, const double* center, const double* P, int n_ranges,
                    const int32_t* pfirst, const int32_t* pcount, const double* poses, void* nodes, int cap_nodes,
                    int32_t* tri, int cap_tri, srt_collider* out, float* bound) {
    const HcDeform h{first, count, n_verts, corner, recompute, center, P};
    return refit_out(d, &h, n_ranges, pfirst, pcount, poses, nodes, cap_nodes, tri, cap_tri, out, bound);
}

// hc_pose_nearest for a deformed (and then posed) mesh
int hc_deform_nearest(const srt_scene_desc* d, int first, int count, int n_verts, const int32_t* corner,
                      const uint8_t* recompute, const double* center, const double* P, int n_ranges,
                      const int32_t* pfirst, const int32_t* pcount, const double* poses, const double* O,
                      const double* D, int64_t n, double* t, int32_t* id, double* orient) {
    const HcDeform h{first, count, n_verts, corner, recompute, center, P};
    return nearest_out(d, &h, n_ranges, pfirst, pcount, poses, O, D, n, t, id, orient);
}

}  // extern "C"
