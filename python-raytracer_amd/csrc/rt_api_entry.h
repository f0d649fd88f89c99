// rt_api_entry.h -- entry points of one kernel each: srt_nearest, srt_intersect_collider,
// srt_collider_surface, srt_texture_lookup, srt_material_normal, srt_primary_rays; the first-hit AOVs and
// the denoiser (srt_render_aovs, srt_denoise, srt_denoise_var, srt_temporal_accumulate; kernels in rt_denoise.h);
// device memory for the caller
// (srt_device_alloc, srt_device_free, srt_memcpy); srt_mt19937_uniforms.
// At its head, what only these entry points use: run_kernel, EventList, stage_in.
// A fragment of rt_kernels.hip, included at its end and not compiled alone.  Before it: what stands above
// its include in rt_kernels.hip; it uses (the API kernels, DevList, grid_for, check_flags, finish_async, mt_launch).
namespace {

// The shared tail of the single-kernel entry points: `kernel` over `n` items on the current slot's
// stream, checked and waited for.  With `dflags` the kernel's flag word is read back and judged
// (check_flags) into *flag_rc, which the entry point returns once its outputs are copied.
template <typename K, typename... A>
int run_kernel(srt_ctx* c, int64_t n, const uint32_t* dflags, int* flag_rc, K kernel, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, c->max_blocks)), dim3(BLOCK), 0, c->f->stream, args...);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->f->stream));
    if (!dflags) return SRT_OK;
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, dflags, 4, hipMemcpyDefault));
    *flag_rc = check_flags(flags);
    return SRT_OK;
}

// HIP events of one call, destroyed with it
struct EventList {
    std::vector<hipEvent_t> e;
    ~EventList() {
        for (hipEvent_t v : e) (void)hipEventDestroy(v);
    }
    hipError_t create(int n) {
        for (int i = 0; i < n; ++i) {
            hipEvent_t v;
            if (hipError_t rc = hipEventCreate(&v); rc != hipSuccess) return rc;
            e.push_back(v);
        }
        return hipSuccess;
    }
};

// an input array of a call: device memory is used in place, host memory is copied into a buffer of `bufs`
template <typename T>
hipError_t stage_in(DevList& bufs, const T* src, int64_t count, const T** dst) {
    if (is_device_ptr(src)) {
        *dst = src;
        return hipSuccess;
    }
    T* p = nullptr;
    const hipError_t e = bufs.in(&p, src, count);
    *dst = p;
    return e;
}

}  // namespace

extern "C" {

int srt_nearest(srt_ctx* c, const double* O, const double* D, int64_t n, double* t, int32_t* id, double* orient) {
    if (!c || !O || !D) return fail(SRT_ERR_ARG, "null argument");
    if (!c->has_scene) return fail(SRT_ERR_NOSCENE, "no scene uploaded");
    if (n <= 0) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    double *dO, *dD, *dt, *dor;
    int32_t* did;
    HIP_TRY(bufs.in(&dO, O, 3 * n));
    HIP_TRY(bufs.in(&dD, D, 3 * n));
    HIP_TRY(bufs.alloc(&dt, n));
    HIP_TRY(bufs.alloc(&dor, n));
    HIP_TRY(bufs.alloc(&did, n));
    if (int rc = run_kernel(c, n, nullptr, nullptr, k_nearest, c->S, dO, dD, n, dt, did, dor)) return rc;
    if (t) HIP_TRY(bufs.copy(t, dt, n));
    if (id) HIP_TRY(bufs.copy(id, did, n));
    if (orient) HIP_TRY(bufs.copy(orient, dor, n));
    return SRT_OK;
}

int srt_intersect_collider(srt_ctx* c, const srt_collider* col, const double* O, const double* D, int64_t n,
                           double* out) {
    if (!c || !col || !O || !D || !out) return fail(SRT_ERR_ARG, "null argument");
    if (col->type < 0 || col->type > 3) return fail(SRT_ERR_ARG, "bad collider type");
    if (n <= 0) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    double *dO, *dD, *dout;
    srt_collider* dcol;
    HIP_TRY(bufs.in(&dO, O, 3 * n));
    HIP_TRY(bufs.in(&dD, D, 3 * n));
    HIP_TRY(bufs.alloc(&dout, 2 * n));
    HIP_TRY(bufs.in(&dcol, col, 1));
    if (int rc = run_kernel(c, n, nullptr, nullptr, k_intersect_one, dcol, dO, dD, n, dout)) return rc;
    HIP_TRY(bufs.copy(out, dout, 2 * n));
    return SRT_OK;
}

int srt_collider_surface(srt_ctx* c, const srt_collider* col, const double* P, int64_t n, double* N, double* uv,
                         int primitive_uv) {
    if (!c || !col || !P || (!N && !uv)) return fail(SRT_ERR_ARG, "null argument");
    if (col->type < 0 || col->type > 3) return fail(SRT_ERR_ARG, "bad collider type");
    if (uv && col->type == SRT_TRIANGLE && !(col->flags & SRT_CF_VUV))
        return fail(SRT_ERR_ARG, "Triangle uv is undefined in the reference (triangle.py:79-83)");
    if (n <= 0) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    srt_collider rec = *col;
    if (!primitive_uv) rec.flags &= ~SRT_CF_UV_CROSS;  // the collider's own 4x3 cross coordinates
    double *dP, *dN = nullptr, *duv = nullptr;
    srt_collider* dcol;
    HIP_TRY(bufs.in(&dP, P, 3 * n));
    if (N) HIP_TRY(bufs.alloc(&dN, 3 * n));
    if (uv) HIP_TRY(bufs.alloc(&duv, 2 * n));
    HIP_TRY(bufs.in(&dcol, &rec, 1));
    if (int rc = run_kernel(c, n, nullptr, nullptr, k_collider_surface, dcol, dP, n, dN, duv)) return rc;
    if (N) HIP_TRY(bufs.copy(N, dN, 3 * n));
    if (uv) HIP_TRY(bufs.copy(uv, duv, 2 * n));
    return SRT_OK;
}

int srt_texture_lookup(srt_ctx* c, const srt_texture* tex, const uint8_t* texels, int64_t texel_bytes,
                       const double* uv, int64_t n, double* rgb) {
    if (!c || !tex || !texels || !uv || !rgb) return fail(SRT_ERR_ARG, "null argument");
    if (tex->offset < 0 || tex->offset + tex->height * tex->width * tex->channels > texel_bytes)
        return fail(SRT_ERR_ARG, "texture record outside the texel array");
    if (n <= 0) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    uint8_t* dtexels;
    srt_texture* dtex;
    double *duv, *drgb;
    uint32_t* dflags;
    HIP_TRY(bufs.in(&dtexels, texels, texel_bytes));
    HIP_TRY(bufs.in(&dtex, tex, 1));
    HIP_TRY(bufs.in(&duv, uv, 2 * n));
    HIP_TRY(bufs.alloc(&drgb, 3 * n));
    HIP_TRY(bufs.alloc(&dflags, 1));
    HIP_TRY(hipMemset(dflags, 0, 4));
    SceneView S{};
    S.tex = (const RT_RO srt_texture*)dtex;
    S.texels = (const RT_RO uint8_t*)dtexels;
    S.ntex = 1;
    int flag_rc = SRT_OK;
    if (int rc = run_kernel(c, n, dflags, &flag_rc, k_texture_lookup, S, duv, n, drgb, dflags)) return rc;
    HIP_TRY(bufs.copy(rgb, drgb, 3 * n));
    return flag_rc;
}

int srt_material_normal(srt_ctx* c, const srt_collider* col, const srt_texture* normalmap, const uint8_t* texels,
                        int64_t texel_bytes, const double* P, const double* orient, int64_t n, double* N) {
    if (!c || !col || !P || !orient || !N) return fail(SRT_ERR_ARG, "null argument");
    if (col->type < 0 || col->type > 3) return fail(SRT_ERR_ARG, "bad collider type");
    if (normalmap) {
        if (!texels || normalmap->offset < 0 || normalmap->channels < 3 || normalmap->channel0 < 0 ||
            normalmap->channel0 + 3 > normalmap->channels ||
            normalmap->offset + (int64_t)normalmap->height * normalmap->width * normalmap->channels > texel_bytes)
            return fail(SRT_ERR_ARG, "normal-map record outside the texel array");
        if (col->type != SRT_PLANE && col->type != SRT_CUBOID)
            return fail(SRT_ERR_ARG, "a normal map needs the collider's inverse_basis_matrix (Plane, Cuboid)");
    }
    if (n <= 0) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    srt_material mrec{};
    mrec.type = SRT_GLOSSY;
    mrec.tex = mrec.tex_aux0 = mrec.tex_aux1 = -1;
    mrec.normalmap = normalmap ? 0 : -1;
    srt_collider* dcol;
    srt_material* dmat;
    srt_texture* dtex = nullptr;
    uint8_t* dtexels = nullptr;
    double *dP, *dor, *dN;
    uint32_t* dflags;
    HIP_TRY(bufs.in(&dcol, col, 1));
    HIP_TRY(bufs.in(&dmat, &mrec, 1));
    HIP_TRY(bufs.in(&dP, P, 3 * n));
    HIP_TRY(bufs.in(&dor, orient, n));
    HIP_TRY(bufs.alloc(&dN, 3 * n));
    HIP_TRY(bufs.alloc(&dflags, 1));
    HIP_TRY(hipMemset(dflags, 0, 4));
    SceneView S{};
    if (normalmap) {
        HIP_TRY(bufs.in(&dtex, normalmap, 1));
        HIP_TRY(bufs.in(&dtexels, texels, texel_bytes));
        S.tex = (const RT_RO srt_texture*)dtex;
        S.texels = (const RT_RO uint8_t*)dtexels;
        S.ntex = 1;
    }
    int flag_rc = SRT_OK;
    if (int rc = run_kernel(c, n, dflags, &flag_rc, k_material_normal, S, dcol, dmat, dP, dor, n, dN, dflags)) return rc;
    HIP_TRY(bufs.copy(N, dN, 3 * n));
    return flag_rc;
}

int srt_primary_rays(srt_ctx* c, const srt_camera* cam, const double* J, double* O, double* D) {
    if (!c || !cam || !J || !O || !D) return fail(SRT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    const int64_t n = (int64_t)cam->width * cam->height;
    double *dJ, *dO, *dD, *xs, *ys;
    HIP_TRY(bufs.in(&dJ, J, 4 * n));
    HIP_TRY(bufs.alloc(&dO, 3 * n));
    HIP_TRY(bufs.alloc(&dD, 3 * n));
    HIP_TRY(bufs.in(&xs, cam->xs, cam->width));
    HIP_TRY(bufs.in(&ys, cam->ys, cam->height));
    srt_camera k = *cam;
    k.xs = xs;
    k.ys = ys;
    if (int rc = run_kernel(c, n, nullptr, nullptr, k_primary_rays, k, dJ, n, dO, dD)) return rc;
    HIP_TRY(bufs.copy(O, dO, 3 * n));
    HIP_TRY(bufs.copy(D, dD, 3 * n));
    return SRT_OK;
}

// ---- denoising (rt_denoise.h) -----------------------------------------------------------------------
int srt_render_aovs(srt_ctx* c, const srt_camera* cam, srt_aov_out* out) {
    if (!c || !cam || !out) return fail(SRT_ERR_ARG, "null argument");
    if (!c->has_scene) return fail(SRT_ERR_NOSCENE, "no scene uploaded");
    if (cam->width <= 0 || cam->height <= 0 || !cam->xs || !cam->ys) return fail(SRT_ERR_ARG, "bad camera");
    if (std::find(c->col_hit_albedo.begin(), c->col_hit_albedo.end(), 1) != c->col_hit_albedo.end())
        return fail(SRT_ERR_ARG, "srt_render_aovs: the scene holds an SRT_MF_HIT_ALBEDO material (a user texture: "
                                 "its albedo is not known to the device)");
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    const int64_t n = (int64_t)cam->width * cam->height;
    AovOut d{};
    if (out->hit_id) HIP_TRY(bufs.alloc(&d.hit_id, n));
    if (out->depth) HIP_TRY(bufs.alloc(&d.depth, n));
    if (out->position) HIP_TRY(bufs.alloc(&d.position, 3 * n));
    if (out->normal) HIP_TRY(bufs.alloc(&d.normal, 3 * n));
    if (out->albedo) HIP_TRY(bufs.alloc(&d.albedo, 3 * n));
    double *xs, *ys;
    uint32_t* dflags;
    HIP_TRY(bufs.in(&xs, cam->xs, cam->width));
    HIP_TRY(bufs.in(&ys, cam->ys, cam->height));
    HIP_TRY(bufs.alloc(&dflags, 1));
    HIP_TRY(hipMemset(dflags, 0, 4));
    srt_camera k = *cam;
    k.xs = xs;
    k.ys = ys;
    SceneView S = c->S;
    S.nlut_lds = 0;  // (k_aov stages no texture tables in LDS: it reads them from the texture records)
    EventList ev;
    HIP_TRY(ev.create(2));
    hipStream_t st = c->f->stream;
    HIP_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(k_aov, dim3(grid_for(n, c->max_blocks)), dim3(DN_BLOCK), 0, st, S, k, d, dflags);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    out->ms_kernel = ms;
    uint32_t flags = 0;
    HIP_TRY(hipMemcpy(&flags, dflags, 4, hipMemcpyDefault));
    if (int rc = check_flags(flags)) return rc;
    if (out->hit_id) HIP_TRY(bufs.copy(out->hit_id, d.hit_id, n));
    if (out->depth) HIP_TRY(bufs.copy(out->depth, d.depth, n));
    if (out->position) HIP_TRY(bufs.copy(out->position, d.position, 3 * n));
    if (out->normal) HIP_TRY(bufs.copy(out->normal, d.normal, 3 * n));
    if (out->albedo) HIP_TRY(bufs.copy(out->albedo, d.albedo, 3 * n));
    return SRT_OK;
}

int srt_denoise(srt_ctx* c, int32_t width, int32_t height, const srt_denoise_args* a) {
    if (!c || !a) return fail(SRT_ERR_ARG, "null argument");
    if (width <= 0 || height <= 0) return fail(SRT_ERR_ARG, "srt_denoise: non-positive image size");
    if (!a->rgb || !a->normal || !a->albedo || !a->position || !a->depth)
        return fail(SRT_ERR_ARG, "srt_denoise: NULL colour or guide array");
    if (a->levels < 0 || a->levels > SRT_DENOISE_MAX_LEVELS) return fail(SRT_ERR_ARG, "srt_denoise: levels outside 0..8");
    if (!(a->sigma_color > 0.0) || !(a->sigma_normal > 0.0) || !(a->sigma_albedo > 0.0) || !(a->sigma_plane > 0.0))
        return fail(SRT_ERR_ARG, "srt_denoise: sigmas must be positive");
    if (a->flags & ~SRT_DENOISE_RGBX) return fail(SRT_ERR_ARG, "srt_denoise: unknown flag");
    if (!a->out_rgb && !a->out_srgb8) return fail(SRT_ERR_ARG, "srt_denoise: no output");
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    const int64_t n = (int64_t)width * height;
    AtrousPlanes G{};
    G.npix = n;
    G.W = width;
    HIP_TRY(stage_in(bufs, a->rgb, 3 * n, &G.rgb));
    HIP_TRY(stage_in(bufs, a->normal, 3 * n, &G.normal));
    HIP_TRY(stage_in(bufs, a->albedo, 3 * n, &G.albedo));
    HIP_TRY(stage_in(bufs, a->position, 3 * n, &G.position));
    HIP_TRY(stage_in(bufs, a->depth, n, &G.depth));
    double* pong[2] = {nullptr, nullptr};  // the levels' colour buffers
    for (int k = 0; k < std::min(a->levels, 2); ++k) HIP_TRY(bufs.alloc(&pong[k], 3 * n));
    const bool rgbx = (a->flags & SRT_DENOISE_RGBX) != 0;
    const int64_t u8_bytes = n * (rgbx ? 4 : 3);
    uint8_t* du8 = nullptr;
    if (a->out_srgb8) {
        if (is_device_ptr(a->out_srgb8))
            du8 = a->out_srgb8;
        else
            HIP_TRY(bufs.alloc(&du8, u8_bytes));
    }
    EventList ev;
    if (a->ms_levels) HIP_TRY(ev.create(a->levels + 2));
    hipStream_t st = c->f->stream;
    const int64_t segs = ((int64_t)width + 63) / 64;
    const int grid = grid_for(segs * height * 64, c->max_blocks);
    if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[0], st));
    for (int l = 0; l < a->levels; ++l) {
        AtrousLevel K{};
        K.W = width, K.H = height, K.step = 1 << l;
        const double sc = a->sigma_color * ldexp(1.0, -l);
        K.sc2 = sc * sc;
        K.sn2 = a->sigma_normal * a->sigma_normal;
        K.sa2 = a->sigma_albedo * a->sigma_albedo;
        K.sp2 = a->sigma_plane * a->sigma_plane;
        hipLaunchKernelGGL(k_atrous<false>, dim3(grid), dim3(DN_BLOCK), 0, st, G, K, pong[l & 1], AtrousVar{});
        HIP_TRY(hipGetLastError());
        if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[(size_t)l + 1], st));
        G.rgb = pong[l & 1];
    }
    if (du8) {
        hipLaunchKernelGGL(k_denoise_resolve, dim3(grid_for(n, c->max_blocks)), dim3(DN_BLOCK), 0, st, G.rgb, n, du8,
                           rgbx ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[(size_t)a->levels + 1], st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int l = 0; l <= a->levels && a->ms_levels; ++l) {
        // each level, then the whole chain (first launch to the end of the resolve)
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[l < a->levels ? (size_t)l : 0], ev.e[(size_t)l + 1]));
        a->ms_levels[l] = ms;
    }
    if (a->out_rgb && a->out_rgb != G.rgb) HIP_TRY(bufs.copy(a->out_rgb, G.rgb, 3 * n));
    if (a->out_srgb8 && du8 != a->out_srgb8) HIP_TRY(bufs.copy(a->out_srgb8, (const uint8_t*)du8, u8_bytes));
    return SRT_OK;
}

int srt_denoise_var(srt_ctx* c, int32_t width, int32_t height, const srt_denoise_var_args* a) {
    if (!c || !a) return fail(SRT_ERR_ARG, "null argument");
    if (width <= 0 || height <= 0) return fail(SRT_ERR_ARG, "srt_denoise_var: non-positive image size");
    if (!a->rgb_a || !a->rgb_b || !a->normal || !a->albedo || !a->position || !a->depth)
        return fail(SRT_ERR_ARG, "srt_denoise_var: NULL half-frame or guide array");
    if (a->spp_a <= 0 || a->spp_b <= 0) return fail(SRT_ERR_ARG, "srt_denoise_var: spp_a and spp_b must be positive");
    if (a->levels < 0 || a->levels > SRT_DENOISE_MAX_LEVELS) return fail(SRT_ERR_ARG, "srt_denoise_var: levels outside 0..8");
    if (a->flags & ~(SRT_DENOISE_RGBX | SRT_DENOISE_VARIANCE | SRT_DENOISE_DEMODULATE))
        return fail(SRT_ERR_ARG, "srt_denoise_var: unknown flag");
    const bool var = (a->flags & SRT_DENOISE_VARIANCE) != 0, demod = (a->flags & SRT_DENOISE_DEMODULATE) != 0;
    if (!((var ? a->sigma_lum : a->sigma_color) > 0.0) || !(a->sigma_normal > 0.0) || !(a->sigma_albedo > 0.0) ||
        !(a->sigma_plane > 0.0))
        return fail(SRT_ERR_ARG, "srt_denoise_var: the sigmas in use must be positive");
    if (!a->out_rgb && !a->out_srgb8) return fail(SRT_ERR_ARG, "srt_denoise_var: no output");
    if (a->out_variance && !var) return fail(SRT_ERR_ARG, "srt_denoise_var: out_variance needs SRT_DENOISE_VARIANCE");
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    const int64_t n = (int64_t)width * height;
    DnHalves F{};
    F.ka = a->spp_a, F.kb = a->spp_b, F.spp = (double)a->spp_a + (double)a->spp_b;
    F.demod = demod ? 1 : 0;
    AtrousPlanes G{};
    G.npix = n;
    G.W = width;
    HIP_TRY(stage_in(bufs, a->rgb_a, 3 * n, &F.a));
    HIP_TRY(stage_in(bufs, a->rgb_b, 3 * n, &F.b));
    HIP_TRY(stage_in(bufs, a->normal, 3 * n, &G.normal));
    HIP_TRY(stage_in(bufs, a->albedo, 3 * n, &G.albedo));
    HIP_TRY(stage_in(bufs, a->position, 3 * n, &G.position));
    HIP_TRY(stage_in(bufs, a->depth, n, &G.depth));
    // prepare writes cb[0] / vb[0]; level l reads buffer l & 1 and writes the other one
    double *cb[2] = {nullptr, nullptr}, *vb[2] = {nullptr, nullptr};
    for (int k = 0; k < std::min(a->levels + 1, 2); ++k) {
        HIP_TRY(bufs.alloc(&cb[k], 3 * n));
        if (var) HIP_TRY(bufs.alloc(&vb[k], n));
    }
    const bool rgbx = (a->flags & SRT_DENOISE_RGBX) != 0;
    const int64_t u8_bytes = n * (rgbx ? 4 : 3);
    uint8_t* du8 = nullptr;
    if (a->out_srgb8) {
        if (is_device_ptr(a->out_srgb8))
            du8 = a->out_srgb8;
        else
            HIP_TRY(bufs.alloc(&du8, u8_bytes));
    }
    EventList ev;
    if (a->ms_levels) HIP_TRY(ev.create(a->levels + 3));  // before and after prepare, after each level, the end
    hipStream_t st = c->f->stream;
    const int64_t segs = ((int64_t)width + 63) / 64;
    const int grid = grid_for(segs * height * 64, c->max_blocks), grid_px = grid_for(n, c->max_blocks);
    if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(k_dn_prepare, dim3(grid_px), dim3(DN_BLOCK), 0, st, F, G.normal, G.albedo, n, cb[0], vb[0]);
    HIP_TRY(hipGetLastError());
    if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[1], st));
    G.rgb = cb[0];
    for (int l = 0; l < a->levels; ++l) {
        AtrousLevel K{};
        K.W = width, K.H = height, K.step = 1 << l;
        const double sc = a->sigma_color * ldexp(1.0, -l);
        K.sc2 = sc * sc;
        K.sn2 = a->sigma_normal * a->sigma_normal;
        K.sa2 = a->sigma_albedo * a->sigma_albedo;
        K.sp2 = a->sigma_plane * a->sigma_plane;
        double* out = cb[(l + 1) & 1];
        if (var)
            hipLaunchKernelGGL(k_atrous<true>, dim3(grid), dim3(DN_BLOCK), 0, st, G, K, out,
                               AtrousVar{vb[l & 1], vb[(l + 1) & 1], a->sigma_lum});
        else
            hipLaunchKernelGGL(k_atrous<false>, dim3(grid), dim3(DN_BLOCK), 0, st, G, K, out, AtrousVar{});
        HIP_TRY(hipGetLastError());
        if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[(size_t)l + 2], st));
        G.rgb = out;
    }
    double* res = cb[a->levels & 1];  // == G.rgb
    if (demod) {
        hipLaunchKernelGGL(k_dn_finish, dim3(grid_px), dim3(DN_BLOCK), 0, st, F, G.normal, G.albedo, n, res, du8,
                           rgbx ? 1 : 0);
        HIP_TRY(hipGetLastError());
    } else if (du8) {
        hipLaunchKernelGGL(k_denoise_resolve, dim3(grid_px), dim3(DN_BLOCK), 0, st, (const double*)res, n, du8,
                           rgbx ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (a->ms_levels) HIP_TRY(hipEventRecord(ev.e[(size_t)a->levels + 2], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (a->ms_levels) {
        float ms = 0.f;
        for (int l = 0; l < a->levels; ++l) {
            HIP_TRY(hipEventElapsedTime(&ms, ev.e[(size_t)l + 1], ev.e[(size_t)l + 2]));
            a->ms_levels[l] = ms;
        }
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[(size_t)a->levels + 2]));
        a->ms_levels[a->levels] = ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        a->ms_levels[a->levels + 1] = ms;
    }
    if (a->out_rgb) HIP_TRY(bufs.copy(a->out_rgb, (const double*)res, 3 * n));
    if (a->out_variance) HIP_TRY(bufs.copy(a->out_variance, (const double*)vb[a->levels & 1], n));
    if (a->out_srgb8 && du8 != a->out_srgb8) HIP_TRY(bufs.copy(a->out_srgb8, (const uint8_t*)du8, u8_bytes));
    return SRT_OK;
}

int srt_temporal_accumulate(srt_ctx* c, int32_t width, int32_t height, const srt_temporal_args* a) {
    if (!c || !a) return fail(SRT_ERR_ARG, "null argument");
    if (width <= 0 || height <= 0) return fail(SRT_ERR_ARG, "srt_temporal_accumulate: non-positive image size");
    if (a->max_history < 1) return fail(SRT_ERR_ARG, "srt_temporal_accumulate: max_history must be at least 1");
    if (!(a->normal_max >= 0.0) || !(a->plane_max >= 0.0) || a->normal_max - a->normal_max != 0.0 ||
        a->plane_max - a->plane_max != 0.0)
        return fail(SRT_ERR_ARG, "srt_temporal_accumulate: normal_max and plane_max must be finite and not negative");
    if (a->flags & ~SRT_TEMPORAL_DEMODULATE) return fail(SRT_ERR_ARG, "srt_temporal_accumulate: unknown flag");
    const bool demod = (a->flags & SRT_TEMPORAL_DEMODULATE) != 0;
    if (!a->rgb_a || !a->rgb_b || !a->hit_id || !a->position || !a->normal || !a->depth || (demod && !a->albedo))
        return fail(SRT_ERR_ARG, "srt_temporal_accumulate: NULL half-frame or guide array");
    if (!a->out_a || !a->out_b || !a->out_hist_a || !a->out_hist_b || !a->out_len)
        return fail(SRT_ERR_ARG, "srt_temporal_accumulate: NULL output");
    if (a->hist_len) {
        if (!a->hist_a || !a->hist_b || !a->hist_hit_id || !a->hist_position || !a->hist_normal || !a->prev_cam)
            return fail(SRT_ERR_ARG, "srt_temporal_accumulate: hist_len without the other history arrays or prev_cam");
        if (a->prev_cam->width != width || a->prev_cam->height != height)
            return fail(SRT_ERR_ARG, "srt_temporal_accumulate: prev_cam is of another size");
        if (a->out_hist_a == a->hist_a || a->out_hist_b == a->hist_b || a->out_len == a->hist_len)
            return fail(SRT_ERR_ARG, "srt_temporal_accumulate: the history cannot be updated in place");
    }
    if (a->motion && a->n_motion < 1) return fail(SRT_ERR_ARG, "srt_temporal_accumulate: motion with n_motion < 1");
    HIP_TRY(hipSetDevice(c->device));
    DevList bufs;
    const int64_t n = (int64_t)width * height;
    TemporalPlanes T{};
    T.npix = n;
    T.W = width, T.H = height;
    T.max_history = (double)a->max_history, T.normal_max = a->normal_max, T.plane_max = a->plane_max;
    T.demod = demod ? 1 : 0;
    HIP_TRY(stage_in(bufs, a->rgb_a, 3 * n, &T.a));
    HIP_TRY(stage_in(bufs, a->rgb_b, 3 * n, &T.b));
    HIP_TRY(stage_in(bufs, a->hit_id, n, &T.hit_id));
    HIP_TRY(stage_in(bufs, a->position, 3 * n, &T.position));
    HIP_TRY(stage_in(bufs, a->normal, 3 * n, &T.normal));
    if (demod) HIP_TRY(stage_in(bufs, a->albedo, 3 * n, &T.albedo));
    HIP_TRY(stage_in(bufs, a->depth, n, &T.depth));
    if (a->hist_len) {
        T.cam = temporal_cam(*a->prev_cam);
        HIP_TRY(stage_in(bufs, a->hist_a, 3 * n, &T.hist_a));
        HIP_TRY(stage_in(bufs, a->hist_b, 3 * n, &T.hist_b));
        HIP_TRY(stage_in(bufs, a->hist_len, n, &T.hist_len));
        HIP_TRY(stage_in(bufs, a->hist_hit_id, n, &T.hist_hit_id));
        HIP_TRY(stage_in(bufs, a->hist_position, 3 * n, &T.hist_position));
        HIP_TRY(stage_in(bufs, a->hist_normal, 3 * n, &T.hist_normal));
    }
    const bool motion = a->motion && a->hist_len;  // a first frame ignores the table
    if (motion) {
        T.n_motion = a->n_motion;
        HIP_TRY(stage_in(bufs, a->motion, (int64_t)a->n_motion * 12, &T.motion));
    }
    // an output in device memory is written in place, a host array through a buffer of the call
    double* const host[5] = {a->out_a, a->out_b, a->out_hist_a, a->out_hist_b, a->out_len};
    const int64_t count[5] = {3 * n, 3 * n, 3 * n, 3 * n, n};
    double* dev[5];
    for (int k = 0; k < 5; ++k) {
        if (is_device_ptr(host[k]))
            dev[k] = host[k];
        else
            HIP_TRY(bufs.alloc(&dev[k], count[k]));
    }
    const TemporalOut out{dev[0], dev[1], dev[2], dev[3], dev[4]};
    EventList ev;
    HIP_TRY(ev.create(2));
    hipStream_t st = c->f->stream;
    // one 64-pixel row segment per wave, no grid-stride loop (k_temporal)
    const int64_t items = (((int64_t)width + 63) / 64) * height, blocks = (items + DN_BLOCK / 64 - 1) / (DN_BLOCK / 64);
    if (blocks > 0x7fffffff) return fail(SRT_ERR_ARG, "srt_temporal_accumulate: image too large");
    HIP_TRY(hipEventRecord(ev.e[0], st));
    if (motion)
        hipLaunchKernelGGL(k_temporal<true>, dim3((unsigned)blocks), dim3(DN_BLOCK), 0, st, T, out);
    else
        hipLaunchKernelGGL(k_temporal<false>, dim3((unsigned)blocks), dim3(DN_BLOCK), 0, st, T, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(hipStreamSynchronize(st));
    if (a->ms_kernel) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *a->ms_kernel = ms;
    }
    for (int k = 0; k < 5; ++k)
        if (dev[k] != host[k]) HIP_TRY(bufs.copy(host[k], (const double*)dev[k], count[k]));
    return SRT_OK;
}

int srt_device_alloc(srt_ctx* c, int64_t bytes, void** out) {
    if (!c || !out || bytes <= 0) return fail(SRT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(out, (size_t)bytes));
    return SRT_OK;
}

int srt_device_free(srt_ctx* c, void* p) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (p) HIP_TRY(hipFree(p));
    return SRT_OK;
}

int srt_memcpy(srt_ctx* c, void* dst, const void* src, int64_t bytes) {
    if (!c || !dst || !src || bytes < 0) return fail(SRT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDefault));
    return SRT_OK;
}

int srt_mt19937_uniforms(srt_ctx* c, const uint32_t* key, int32_t pos, int64_t n_out, int64_t n_skip, double* out,
                         uint32_t* key_out, int32_t* pos_out) {
    if (!c || !key || !key_out || !pos_out || (n_out > 0 && !out)) return fail(SRT_ERR_ARG, "null argument");
    c->pf.valid = false;  // (generates from the stream state a prefetch assumed)
    if (pos < 0 || pos > rtmt::N || n_out < 0 || n_skip < 0) return fail(SRT_ERR_ARG, "bad position or count");
    if (is_device_ptr(key) || is_device_ptr(key_out)) return fail(SRT_ERR_ARG, "key and key_out are host arrays");
    if (n_out + n_skip == 0) {
        memcpy(key_out, key, rtmt::N * 4);
        *pos_out = pos;
        return SRT_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_async(c, nullptr);  // frames in flight may use the generator's scratch
    if (rc) return rc;
    if ((rc = mt_ensure(c))) return rc;
    double* dst = out;
    const bool host_out = n_out > 0 && !is_device_ptr(out);
    if (host_out) {
        if ((rc = c->mt_out.ensure(n_out))) return rc;
        dst = c->mt_out;
    }
    hipStream_t st = c->f->stream;
    HIP_TRY(hipMemcpyAsync(mt_key0(c), key, rtmt::N * 4, hipMemcpyHostToDevice, st));
    int final_pos = 0;
    if ((rc = mt_win_ensure(c, *c->f, (int64_t)rtmt::SEGS * rtmt::N))) return rc;
    if ((rc = mt_launch(c, st, c->f->mt_win, mt_key0(c), pos, n_out, n_skip, dst, &final_pos))) return rc;
    if (host_out) HIP_TRY(hipMemcpyAsync(out, dst, (size_t)n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(key_out, mt_dump(c), rtmt::N * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *pos_out = final_pos;
    return SRT_OK;
}

}  // extern "C"
