// rt_api_trace.h -- tracing and shading the caller's rays on the per-depth path: trace_impl (seed the queue,
// one launch per depth, the retries, the children of one shading level) and check_level_args; then the
// entry points srt_trace, srt_shade, srt_shade_level, srt_shade_level_inputs.
// A fragment of rt_kernels.hip, included at its end and not compiled alone.  Before it: what stands above
// its include in rt_kernels.hip; it uses (k_seed_queue, k_shade_forced*, k_fx_combine, k_gather_children,
// pick_variant, DevList, grid_for, base_params, ensure_queues, trace_grid, check_flags, finish_async).
namespace {
// get_raycolor (srt_trace) or Material.get_color at given hits (srt_shade: fid/ft/fo non-null)
// kids (srt_shade_level): shade the first depth only and hand its children back instead of tracing them
// in (srt_shade_level_inputs): the per-hit shading inputs of a scene that needs them
int trace_impl(srt_ctx* c, const srt_trace_args* a, const int32_t* fid, const double* ft, const double* fo,
               srt_stats* st, srt_children* kids = nullptr, const srt_hit_inputs* in = nullptr,
               const char* who = "srt_trace") {
    auto t_start = std::chrono::steady_clock::now();
    if (!c || !a || !a->origin || !a->dir || !a->out_rgb) return fail(SRT_ERR_ARG, "null argument");
    c->pf.valid = false;  // (slot 0's buffers are reused here)
    if (!c->has_scene) return fail(SRT_ERR_NOSCENE, "no scene uploaded");
    if (c->needs_inputs && !in) return refuse_inputs_scene(who);
    if (a->depth < 0 || a->depth > 200 || a->diffuse_reflections < 0) return fail(SRT_ERR_ARG, "bad depth");
    if (a->n <= 0) return SRT_OK;
    if (a->n >= ((int64_t)1 << 31)) return fail(SRT_ERR_ARG, "batch too large");
    HIP_TRY(hipSetDevice(c->device));
    int rc0 = finish_async(c, nullptr);
    if (rc0) return rc0;
    c->f->dirty = true;  // counts/flags/shadow are left as this call's memsets and kernels leave them
    const int64_t n = a->n;
    int rc = SRT_OK;
    DevList bufs;  // (freed on every return)
    const hipStream_t st0 = c->f->stream;
    double *O = nullptr, *D = nullptr;
    int32_t* med = nullptr;
    HIP_TRY(bufs.in(&O, a->origin, 3 * n, st0));
    HIP_TRY(bufs.in(&D, a->dir, 3 * n, st0));
    if (a->medium) HIP_TRY(bufs.in(&med, a->medium, n, st0));
    // the user's per-hit values, copied in with the other per-call buffers
    double *dalb = nullptr, *dldist = nullptr, *dlirr = nullptr;
    if (in && in->albedo) HIP_TRY(bufs.in(&dalb, in->albedo, 3 * n, st0));
    if (in && in->n_lights > 0) {
        HIP_TRY(bufs.in(&dldist, in->light_dist, (int64_t)in->n_lights * n, st0));
        HIP_TRY(bufs.in(&dlirr, in->light_irr, (int64_t)in->n_lights * 3 * n, st0));
    }
    int32_t* dfid = nullptr;
    double *dft = nullptr, *dfo = nullptr;
    if (fid) {
        HIP_TRY(bufs.in(&dfid, fid, n, st0));
        HIP_TRY(bufs.in(&dft, ft, n, st0));
        HIP_TRY(bufs.in(&dfo, fo, n, st0));
    }
    if ((rc = c->f->fb.ensure(3 * n))) return rc;
    if ((rc = c->f->fbx.ensure(fx_words(n)))) return rc;
    if ((rc = ensure_queues(*c->f, n * c->fanout))) return rc;
    // depths a->depth .. a->depth + cap (the batch's depth is a scalar in the reference)
    const int d0 = a->depth;
    const int dlast = kids ? d0 : std::min(SRT_MAX_DEPTHS - 2, d0 + depth_cap(c));
    srt_stats S{};
    std::vector<uint32_t> counts(SRT_MAX_DEPTHS * NSHARD);
    bool fx = c->deterministic;  // fixed-point colour sums (fb_add)
    for (int attempt = 0;; ++attempt) {
        if (attempt > 8) { rc = fail(SRT_ERR_MEMORY, "ray queues keep overflowing"); break; }
        HIP_TRY(hipMemsetAsync(c->f->fb, 0, (size_t)3 * n * 8, c->f->stream));
        HIP_TRY(hipMemsetAsync(c->f->fbx, 0, (size_t)fx_words(n) * 8, c->f->stream));
        HIP_TRY(hipMemsetAsync(c->f->counts, 0, (size_t)SRT_MAX_DEPTHS * NSHARD * 4, c->f->stream));
        HIP_TRY(hipMemsetAsync(c->f->flags, 0, 8, c->f->stream));
        HIP_TRY(hipMemsetAsync(c->f->shadow, 0, 8 * NSHARD, c->f->stream));
        uint32_t seed_counts[NSHARD];
        for (int s = 0; s < NSHARD; ++s) seed_counts[s] = (uint32_t)((n - s + NSHARD - 1) / NSHARD);
        HIP_TRY(hipMemcpyAsync(c->f->counts + (int64_t)d0 * NSHARD, seed_counts, sizeof(seed_counts),
                               hipMemcpyHostToDevice, c->f->stream));
        hipLaunchKernelGGL(k_seed_queue, dim3(grid_for(n, c->max_blocks)), dim3(BLOCK), 0, c->f->stream, c->f->q[d0 & 1],
                           c->f->seg, O, D, med, n, (uint32_t)d0, (uint32_t)a->diffuse_reflections, (uint32_t)c->S.nmedia);
        HIP_TRY(hipGetLastError());
        TraceParams P = base_params(c, *c->f, a->seed);
        P.fb = c->f->fb;
        P.fbx = fx ? c->f->fbx : nullptr;
        P.npix = n;
        const Variant& V = pick_variant(c->mats, c->seq_on ? c->seq : 0);
        for (int d = d0; d <= dlast; ++d) {
            P.depth = d;
            P.qin = c->f->q[d & 1];
            P.qout = c->f->q[(d + 1) & 1];
            P.cnt_in = c->f->counts + (int64_t)d * NSHARD;
            P.cnt_out = c->f->counts + (int64_t)(d + 1) * NSHARD;
            if (fid && d == d0) {
                P.force_id = dfid;
                P.force_t = dft;
                P.force_o = dfo;
                const bool bvh = (c->mats & MAT_BVH) != 0, va = (c->mats & MAT_VATTR) != 0;
                if (in) {
                    const HitPtrs H{dalb, dldist, dlirr};
                    hipLaunchKernelGGL(va ? (bvh ? k_shade_forced_inputs<MATS_BVH_VATTR | MAT_HITIN>
                                                 : k_shade_forced_inputs<MAT_GENERIC | MAT_VATTR | MAT_HITIN>)
                                          : (bvh ? k_shade_forced_inputs<MAT_GENERIC | MAT_BVH | MAT_HITIN>
                                                 : k_shade_forced_inputs<MAT_GENERIC | MAT_HITIN>),
                                       dim3(trace_grid(c)), dim3(BLOCK), lut_bytes(c), c->f->stream, P, H);
                } else if (c->mats & MAT_PLIGHT) {  // (never with MAT_VATTR: check_scene_desc)
                    hipLaunchKernelGGL(bvh ? k_shade_forced<MATS_BVH_PLIGHT> : k_shade_forced<MATS_GENERIC_PLIGHT>,
                                       dim3(trace_grid(c)), dim3(BLOCK), lut_bytes(c), c->f->stream, P);
                } else {
                    hipLaunchKernelGGL(va ? (bvh ? k_shade_forced<MATS_BVH_VATTR> : k_shade_forced<MAT_GENERIC | MAT_VATTR>)
                                          : (bvh ? k_shade_forced<MAT_GENERIC | MAT_BVH> : k_shade_forced<MAT_GENERIC>),
                                       dim3(trace_grid(c)), dim3(BLOCK), lut_bytes(c), c->f->stream, P);
                }
                P.force_id = nullptr;
                P.force_t = P.force_o = nullptr;
            } else {
                hipLaunchKernelGGL(V.trace, dim3(trace_grid(c)), dim3(BLOCK), lut_bytes(c), c->f->stream, P);
            }
            HIP_TRY(hipGetLastError());
        }
        uint32_t flags[2];
        unsigned long long shadow = 0;
        HIP_TRY(hipMemcpyAsync(counts.data(), c->f->counts, counts.size() * 4, hipMemcpyDeviceToHost, c->f->stream));
        HIP_TRY(hipMemcpyAsync(flags, c->f->flags, sizeof(flags), hipMemcpyDeviceToHost, c->f->stream));
        HIP_TRY(hipMemcpyAsync(&shadow, c->f->shadow, 8, hipMemcpyDeviceToHost, c->f->stream));
        HIP_TRY(hipStreamSynchronize(c->f->stream));
        if ((rc = check_flags(flags[0]))) break;
        if (flags[1]) {
            S.retries++;
            if (flags[1] & RETRY_FIXED_RANGE) fx = false;  // again with f64 atomics
            if ((flags[1] & RETRY_OVERFLOW) && (rc = ensure_queues(*c->f, 2 * c->f->seg * NSHARD))) break;
            continue;
        }
        if (!kids && depth_total(counts.data() + (int64_t)(dlast + 1) * NSHARD, c->f->seg) != 0) {
            rc = fail(SRT_ERR_DEPTH, "rays alive after the depth cap");
            break;
        }
        for (int d = d0; d <= dlast; ++d) S.rays_per_depth[d] = depth_total(counts.data() + (int64_t)d * NSHARD, c->f->seg);
        S.n_depths = dlast + 1;
        for (int d = 0; d < SRT_MAX_DEPTHS; ++d) S.total_rays += S.rays_per_depth[d];
        S.shadow_rays = (int64_t)shadow;
        if (fx) {
            hipLaunchKernelGGL(k_fx_combine, dim3(grid_for(n, c->max_blocks)), dim3(BLOCK), 0, c->f->stream, c->f->fb,
                               (const unsigned long long*)c->f->fbx, n, c->f->flags);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(flags, c->f->flags, sizeof(flags), hipMemcpyDeviceToHost, c->f->stream));
            HIP_TRY(hipStreamSynchronize(c->f->stream));
            if (flags[1] & RETRY_FIXED_RANGE) {
                S.retries++;
                fx = false;  // again with f64 atomics
                continue;
            }
        }
        HIP_TRY(bufs.copy(a->out_rgb, c->f->fb.p, 3 * n, st0));
        HIP_TRY(hipStreamSynchronize(c->f->stream));
        if (kids) {
            // the first depth's children, packed shard by shard (the order the queue appends gave them)
            const uint32_t* kc = counts.data() + (int64_t)(d0 + 1) * NSHARD;
            std::vector<int64_t> prefix(NSHARD);
            int64_t total = 0;
            for (int s = 0; s < NSHARD; ++s) {
                prefix[s] = total;
                total += std::min<int64_t>(kc[s], c->f->seg);
            }
            kids->n = total;
            if (total > kids->cap) {
                rc = fail(SRT_ERR_MEMORY, "children exceed srt_children.cap (n holds the count)");
                break;
            }
            if (total > 0) {
                double *kO, *kD, *kW;
                int32_t *kp, *km, *kd, *kf;
                int64_t* kpre;
                HIP_TRY(bufs.alloc(&kO, 3 * total));
                HIP_TRY(bufs.alloc(&kD, 3 * total));
                HIP_TRY(bufs.alloc(&kW, 3 * total));
                HIP_TRY(bufs.alloc(&kp, total));
                HIP_TRY(bufs.alloc(&km, total));
                HIP_TRY(bufs.alloc(&kd, total));
                HIP_TRY(bufs.alloc(&kf, total));
                HIP_TRY(bufs.alloc(&kpre, NSHARD));
                HIP_TRY(hipMemcpyAsync(kpre, prefix.data(), NSHARD * 8, hipMemcpyHostToDevice, c->f->stream));
                hipLaunchKernelGGL(k_gather_children, dim3(NSHARD), dim3(BLOCK), 0, c->f->stream, c->f->q[(d0 + 1) & 1],
                                   c->f->seg, c->f->counts + (int64_t)(d0 + 1) * NSHARD, kpre, total, kO, kD, kW, kp, km,
                                   kd, kf);
                HIP_TRY(hipGetLastError());
                for (int k = 0; k < 3; ++k) {
                    HIP_TRY(bufs.copy(kids->origin + k * kids->cap, kO + k * total, total, st0));
                    HIP_TRY(bufs.copy(kids->dir + k * kids->cap, kD + k * total, total, st0));
                    HIP_TRY(bufs.copy(kids->weight + k * kids->cap, kW + k * total, total, st0));
                }
                HIP_TRY(bufs.copy(kids->parent, kp, total, st0));
                HIP_TRY(bufs.copy(kids->medium, km, total, st0));
                HIP_TRY(bufs.copy(kids->depth, kd, total, st0));
                HIP_TRY(bufs.copy(kids->diffuse_reflections, kf, total, st0));
                HIP_TRY(hipStreamSynchronize(c->f->stream));
            }
        }
        break;
    }
    if (rc) return rc;
    S.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    if (st) *st = S;
    return SRT_OK;
}

// the hit and children arrays of the shade-level entry points (the children's count starts at zero)
int check_level_args(const int32_t* collider, const double* t, const double* orient, srt_children* kids) {
    if (!collider || !t || !orient || !kids) return fail(SRT_ERR_ARG, "null hit / children arrays");
    kids->n = 0;
    if (kids->cap < 0 || (kids->cap > 0 && (!kids->origin || !kids->dir || !kids->weight || !kids->parent ||
                                            !kids->medium || !kids->depth || !kids->diffuse_reflections)))
        return fail(SRT_ERR_ARG, "srt_children arrays");
    return SRT_OK;
}
}  // namespace

extern "C" {

int srt_trace(srt_ctx* c, const srt_trace_args* a, srt_stats* st) {
    return trace_impl(c, a, nullptr, nullptr, nullptr, st);
}

int srt_shade(srt_ctx* c, const srt_trace_args* a, const int32_t* collider, const double* t, const double* orient,
              srt_stats* st) {
    if (!collider || !t || !orient) return fail(SRT_ERR_ARG, "null hit arrays");
    return trace_impl(c, a, collider, t, orient, st, nullptr, nullptr, "srt_shade");
}

int srt_shade_level(srt_ctx* c, const srt_trace_args* a, const int32_t* collider, const double* t, const double* orient,
                    srt_children* kids, srt_stats* st) {
    if (int rc = check_level_args(collider, t, orient, kids)) return rc;
    return trace_impl(c, a, collider, t, orient, st, kids, nullptr, "srt_shade_level");
}

int srt_shade_level_inputs(srt_ctx* c, const srt_trace_args* a, const int32_t* collider, const double* t,
                           const double* orient, const srt_hit_inputs* in, srt_children* kids, srt_stats* st) {
    if (!in || (!in->albedo && in->n_lights == 0)) {
        // nothing per hit: srt_shade_level (which refuses a scene that needs inputs; a flagged
        // material or a user light then names the missing array below)
        if (!c || !c->has_scene || !c->needs_inputs) return srt_shade_level(c, a, collider, t, orient, kids, st);
    }
    if (!c || !a) return fail(SRT_ERR_ARG, "null argument");
    if (int rc = check_level_args(collider, t, orient, kids)) return rc;
    if (!c->has_scene) return fail(SRT_ERR_NOSCENE, "no scene uploaded");
    const srt_hit_inputs none{nullptr, 0, nullptr, nullptr};
    if (!in) in = &none;
    char msg[256];
    if (in->n_lights != c->n_user_lights) {
        snprintf(msg, sizeof(msg), "srt_hit_inputs.n_lights is %d, the scene holds %d SRT_LIGHT_USER lights",
                 (int)in->n_lights, c->n_user_lights);
        return fail(SRT_ERR_ARG, msg);
    }
    if (in->n_lights > 0 && (!in->light_dist || !in->light_irr))
        return fail(SRT_ERR_ARG, "srt_hit_inputs.light_dist / light_irr are NULL while n_lights > 0");
    if (!in->albedo && a->n > 0 && a->n < ((int64_t)1 << 31)) {
        // (the hit's collider decides whether a colour is read: checked here, the kernel reads unguarded)
        std::vector<int32_t> ids((size_t)a->n);
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipMemcpy(ids.data(), collider, (size_t)a->n * 4, hipMemcpyDefault));
        for (int64_t i = 0; i < a->n; ++i) {
            const int32_t id = ids[(size_t)i];
            if (id >= 0 && id < (int32_t)c->col_hit_albedo.size() && c->col_hit_albedo[(size_t)id]) {
                snprintf(msg, sizeof(msg), "srt_hit_inputs.albedo is NULL, but ray %lld hits collider %d whose "
                         "material has SRT_MF_HIT_ALBEDO", (long long)i, (int)id);
                return fail(SRT_ERR_ARG, msg);
            }
        }
    }
    return trace_impl(c, a, collider, t, orient, st, kids, in, "srt_shade_level_inputs");
}

}  // extern "C"
