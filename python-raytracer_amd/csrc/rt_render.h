// srt_render and srt_render_prefetch (host code; included by rt_kernels.hip after the kernels and the
// context's helpers): what a frame needs of its slot, then one call as a RenderCall, whose methods are
// the phases render_impl runs in order.
namespace {

// What a frame needs of its slot, in elements (0: not used by this frame).  Every size is written once,
// in RenderCall::needs; slot_holds and grow_slot read it.
#define SLOT_BUFFERS(X) X(fb) X(fbg) X(fbx) X(rgb) X(u8) X(jit) X(hit) X(full_u8) X(g_u8) X(g_rgb) X(full_rgb)
struct FrameNeeds {
#define X(b) int64_t b = 0;
    SLOT_BUFFERS(X)
#undef X
    bool g_u8_zeroed = false;  // g_u8 holds the rehearsal's stand-in tiles: defined bytes
    int64_t mt_win = 0;
    int64_t queue_rays = 0, ring_rays = 0;  // rays per depth (per-depth kernels), rays per ring (k_frame)
    int64_t events = 0, host_words = 0;
};

// whether the slot holds everything the frame needs (grow_slot would change nothing)
bool slot_holds(const srt_ctx* c, const FrameSlot& f, const FrameNeeds& N) {
#define X(b) N.b <= f.b.cap &&
    return SLOT_BUFFERS(X) N.mt_win <= f.mt_win.cap &&
#undef X
           (!N.queue_rays || queue_seg_for(N.queue_rays) <= f.seg) &&
           (!N.ring_rays || (ring_cap_for(N.ring_rays) <= f.ring_cap && ring_slots(c) <= f.nslot)) &&
           N.events <= (int64_t)f.ev.size() && N.host_words <= f.host_words;
}

// grow the slot to what the frame needs (no frame is in flight on it)
int grow_slot(srt_ctx* c, FrameSlot& f, const FrameNeeds& N) {
    int r = SRT_OK;
    const int64_t had_g_u8 = f.g_u8.cap;
#define X(b) if (!r && N.b > 0) r = f.b.ensure(N.b);
    SLOT_BUFFERS(X)
#undef X
    if (!r && N.g_u8_zeroed && f.g_u8.cap != had_g_u8 && hipMemset(f.g_u8, 0, (size_t)f.g_u8.cap) != hipSuccess)
        r = fail(SRT_ERR_HIP, "hipMemset failed");
    if (!r && N.mt_win > 0) r = mt_win_ensure(c, f, N.mt_win);
    if (!r && N.queue_rays) r = ensure_queues(f, N.queue_rays);
    if (!r && N.ring_rays) r = ensure_ring(c, f, N.ring_rays);
    if (!r && (int64_t)f.ev.size() < N.events) {
        for (hipEvent_t e : f.ev) (void)hipEventDestroy(e);
        f.ev.assign(N.events, nullptr);
        for (auto& e : f.ev)
            if (hipEventCreate(&e) != hipSuccess) r = fail(SRT_ERR_HIP, "hipEventCreate failed");
    }
    if (!r && f.host_words < N.host_words) {
        if (f.host) (void)hipHostFree(f.host);
        f.host = nullptr;
        f.host_words = 0;
        if (hipHostMalloc((void**)&f.host, (size_t)N.host_words * 4, hipHostMallocDefault) != hipSuccess) {
            r = fail(SRT_ERR_MEMORY, "pinned host allocation failed");
        } else {
            f.host_words = N.host_words;
            memset(f.host, 0, (size_t)f.host_words * 4);  // depths beyond used_words stay zero
        }
    }
    return r;
}

// whether a frame of plan `a` may be queued behind frames of plan `b` in flight
bool same_shape(const FramePlan& a, const FramePlan& b) {
    return a.npass == b.npass && a.dcap == b.dcap && a.frame == b.frame && a.chain_from == b.chain_from &&
           a.fuse == b.fuse && a.W == b.W && a.H == b.H && a.groups == b.groups && a.sharded == b.sharded &&
           a.gather_rgb == b.gather_rgb && a.use_mt == b.use_mt;
}

// where a frame's numpy stream stands between its passes
struct StreamCursor {
    hipStream_t mst = nullptr;      // the stream the generation runs on
    const uint32_t* key = nullptr;  // (device) the key window the next pass starts from
    int pos = 0;
};

struct RenderCall {
    srt_ctx* const c;
    const srt_camera* const cam;
    const srt_render_args* const a;
    bool async = false, sharded = false, use_mt = false, gather_rgb = false, rgb_rows = false, rgbx = false;
    bool jit_dev = false, hit_dev = false, rgb_dev = false, u8_dev = false;  // the caller's buffer is device memory
    std::vector<int32_t> rows_h;
    const int32_t* rows = nullptr;  // rows of this call
    int n_rows = 0;
    int64_t band = 1;  // row-band height of a sharded frame
    int64_t W = 0, Hf = 0, npix = 0;
    FramePlan F;
    const Variant* V = nullptr;
    int64_t ntiles = 0, maxpix = 0, used_words = 0;
    int reh_n = 0;  // rank 0's assembly rehearsed: ranks of the rehearsed job
    int64_t reh_band = 1, reh_maxpix = 0;
    int mt_pm = 3, mts = 0;  // plane mask; where the generation runs (2: the MT stream, 0: the frame's)
    const srt_ctx::MtBandTab* mt_bt[2] = {nullptr, nullptr};
    int64_t mt_win_need = 0, jit_doubles = 0;
    double* res_rgb = nullptr;  // resolve targets
    uint8_t* res_u8 = nullptr;

    int check_args(bool prefetch) {
        if (!prefetch && !c->has_scene) return fail(SRT_ERR_NOSCENE, "no scene uploaded");
        if (c->has_scene && c->needs_inputs) return refuse_inputs_scene(prefetch ? "srt_render_prefetch" : "srt_render");
        if (a->flags & ~(SRT_RENDER_ASYNC | SRT_RENDER_SHARDED | SRT_RENDER_GATHER_RGB | SRT_RENDER_RGB_ROWS |
                         SRT_RENDER_RGB_LOCAL | SRT_RENDER_RGBX))
            return fail(SRT_ERR_ARG, "unknown render flag");
        if ((a->flags & SRT_RENDER_RGBX) && (a->flags & SRT_RENDER_SHARDED))
            return fail(SRT_ERR_ARG, "SRT_RENDER_RGBX: not with SRT_RENDER_SHARDED");
        if ((a->flags & SRT_RENDER_RGB_LOCAL) && (a->out_rgb || (a->flags & (SRT_RENDER_GATHER_RGB | SRT_RENDER_RGB_ROWS))))
            return fail(SRT_ERR_ARG, "SRT_RENDER_RGB_LOCAL needs out_rgb NULL and no SRT_RENDER_GATHER_RGB / RGB_ROWS");
        if ((a->flags & SRT_RENDER_RGB_ROWS) &&
            (!(a->flags & SRT_RENDER_SHARDED) || (a->flags & SRT_RENDER_GATHER_RGB) || !a->out_rgb))
            return fail(SRT_ERR_ARG, "SRT_RENDER_RGB_ROWS needs SRT_RENDER_SHARDED, out_rgb and no SRT_RENDER_GATHER_RGB");
        async = (a->flags & SRT_RENDER_ASYNC) != 0;
        sharded = (a->flags & SRT_RENDER_SHARDED) != 0;
        if (a->spp <= 0 || cam->width <= 0 || cam->height <= 0 || (!sharded && a->n_rows <= 0) || !cam->xs || !cam->ys)
            return fail(SRT_ERR_ARG, "spp, width, height, n_rows must be positive and xs/ys set");
        if (a->jitter && a->mt) return fail(SRT_ERR_ARG, "jitter and mt are exclusive");
        use_mt = a->mt != nullptr;
        if (use_mt && (a->mt->pos < 0 || a->mt->pos > rtmt::N)) return fail(SRT_ERR_ARG, "bad numpy RNG position");
        return SRT_OK;
    }

    // what srt_render_prefetch covers: a synchronous whole frame drawing numpy's stream (Scene.render)
    bool whole_sync_mt_frame() const { return !async && !sharded && use_mt && !a->rows && a->n_rows == cam->height; }

    // the rows of this call, the frame's size and where the caller's buffers live
    int select_rows() {
        n_rows = a->n_rows;
        if (sharded) {
            if (c->nranks > MAX_RANKS) return fail(SRT_ERR_ARG, "too many ranks");
            if (cam->height < c->nranks) return fail(SRT_ERR_ARG, "a sharded frame needs at least one row per rank");
            if (a->out_hit_id) return fail(SRT_ERR_ARG, "hit ids of a sharded frame are not gathered");
            band = shard_band_height(cam->height, c->nranks, shard_kmax(cam->height, c->nranks, c->shard_bands, c->fanout));
            rows_h = band_rows(cam->height, c->nranks, c->rank, band);
            n_rows = (int)rows_h.size();
            if (n_rows == 0) return fail(SRT_ERR_ARG, "a sharded frame left this rank without rows");
            rows = rows_h.data();
        } else if (a->rows) {
            if (is_device_ptr(a->rows)) return fail(SRT_ERR_ARG, "rows must be host memory");
            for (int k = 0; k < a->n_rows; ++k)
                if (a->rows[k] < 0 || a->rows[k] >= cam->height) return fail(SRT_ERR_ARG, "row index out of range");
            rows = a->rows;
        } else {
            if (a->n_rows > cam->height) return fail(SRT_ERR_ARG, "n_rows > height");
            rows_h.resize(a->n_rows);
            for (int k = 0; k < a->n_rows; ++k) rows_h[k] = k;
            rows = rows_h.data();
        }
        HIP_TRY(hipSetDevice(c->device));
        W = cam->width, Hf = cam->height;
        npix = (int64_t)n_rows * W;
        if (W * Hf >= ((int64_t)1 << 31)) return fail(SRT_ERR_ARG, "image too large");
        const int jk = ptr_kind(a->jitter), hk = ptr_kind(a->out_hit_id);
        const int rk = ptr_kind(a->out_rgb), uk = ptr_kind(a->out_srgb8);
        jit_dev = jk == 1, hit_dev = hk == 1, rgb_dev = rk == 1, u8_dev = uk == 1;
        if (async && (jk >= 2 || hk >= 2 || rk == 3 || uk == 3))
            return fail(SRT_ERR_ARG, "an asynchronous render takes device (or NULL) jitter and hit ids, and device or "
                                     "pinned host (srt_host_alloc) outputs");
        // outputs written by this rank: a shard's tiles stay on the device (the gather reads them); rank 0
        // of a sharded frame writes the whole frame to the caller's buffers after the gather
        gather_rgb = sharded && (a->flags & SRT_RENDER_GATHER_RGB) != 0;
        rgb_rows = sharded && (a->flags & SRT_RENDER_RGB_ROWS) != 0;
        if (rgb_rows && rk != 2)
            return fail(SRT_ERR_ARG, "SRT_RENDER_RGB_ROWS: out_rgb must be pinned or registered host memory");
        return SRT_OK;
    }

    // The frame's passes and kernels from its shape, the scene and the options (no HIP calls)
    void plan_frame() {
        // samples per pass: both queues must hold spp_pass * npix * fanout rays
        const int64_t per_sample = npix * c->fanout;
        const int64_t budget_rays = c->queue_budget / (2 * RAY_BYTES);
        int batch = a->batch_spp > 0 ? a->batch_spp
                                     : (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, budget_rays / per_sample));
        batch = std::min(batch, a->spp);
        while (batch > 1 && (int64_t)batch * npix * c->fanout >= ((int64_t)1 << 32) - 1) batch /= 2;
        // the numpy stream of a pass (its samples of the whole frame) is generated into the jitter buffer
        if (use_mt) while (batch > 1 && (int64_t)batch * 4 * W * Hf * 8 > ((int64_t)8 << 30)) batch /= 2;
        F.npix = npix;
        F.W = W;
        F.H = Hf;
        F.sharded = sharded;
        F.gather_rgb = gather_rgb;
        F.use_mt = use_mt;
        F.spp = a->spp;
        F.batch = batch;
        F.npass = (a->spp + batch - 1) / batch;
        F.dcap = depth_cap(c);
        F.nev = F.dcap + 2;  // events per pass: before k_primary, after each depth
        F.cnt_words = (int64_t)SRT_MAX_DEPTHS * NSHARD;
        F.pass_words = F.cnt_words + 2;
        F.frame = c->use_frame < 0 ? c->fanout > 1 : c->use_frame != 0;
        V = &pick_variant(c->mats, c->seq_on ? c->seq : 0);
        ntiles = frame_tiles(frame_tile_for(V->mats), W, npix / W);
        if (F.frame) {
            // a frame kernel block traces one 64-pixel tile through the pass's samples: a small frame (a
            // shard of a multi-GPU frame) has too few tiles to fill the GPU, so its samples are split
            // into groups, one block per (tile, group), until there are ~4 blocks per resident wave
            // slot (c->max_blocks = 4 OCC per CU)
            const int64_t want = 4 * (int64_t)c->max_blocks;
            const int64_t g = (want + ntiles - 1) / ntiles;
            F.groups = (int)std::max<int64_t>(1, std::min<int64_t>(g, batch));
        }
        // fused paths (single-child scenes): by default when the frame's threads (sample groups
        // included, pix_groups) fill two rounds of the resident threads
        F.fuse = !F.frame && c->fanout == 1 && c->chain_ok && V->fused &&
                 (c->fuse_primary > 0 ||
                  (c->fuse_primary < 0 && npix * pix_groups(c, npix, batch, true) >= fused_items(c)));
        if (!F.fuse && !F.frame && c->fanout == 1 && c->chain_ok && c->hint_key[0] == npix && c->hint_key[1] == a->spp &&
            c->hint_key[2] == batch) {
            for (int d = 1; d <= F.dcap; ++d)
                if (c->hint[d] < c->chain_rays) { F.chain_from = d; break; }
        }
        maxpix = sharded ? shard_max_rows(Hf, c->nranks, band) * W : 0;  // the gather's tile
        // only the depths this frame can reach are handed back and cleared per pass
        used_words = std::min<int64_t>(F.cnt_words, (int64_t)(F.dcap + 2) * NSHARD);
        // rank 0's assembly rehearsed (srt_ctx::rehearse_assemble): these rows are rank 0's of an n-rank job
        if (c->rehearse_assemble > 1 && !sharded && a->rows && a->out_srgb8 && !u8_dev && !(a->flags & SRT_RENDER_RGBX)) {
            const int n = c->rehearse_assemble;
            reh_band = shard_band_height(Hf, n, shard_kmax(Hf, n, c->shard_bands, c->fanout));
            const std::vector<int32_t> r0 = band_rows(Hf, n, 0, reh_band);
            if ((int)r0.size() == n_rows && std::equal(r0.begin(), r0.end(), rows)) {
                reh_n = n;
                reh_maxpix = shard_max_rows(Hf, n, reh_band) * W;
            }
        }
    }

    // How the frame's numpy stream is generated: band tables, window table and jitter buffer sizes
    int plan_stream() {
        const int batch = F.batch;
        int rc;
        // numpy stream of a shard (rows not the whole frame): band mode, only the rows' runs generated
        // (rt_mt_kernel.h MtArgs::bands); tables for the full passes and the last pass
        mt_pm = cam->lens_radius != 0.0 ? 15 : 3;  // a pinhole camera reads planes 0 and 1 only
        mts = use_mt ? (n_rows >= Hf ? 2 : 0) : 0;
        mt_win_need = (int64_t)rtmt::SEGS * rtmt::N;
        // (the band tables and end polynomials are kept per frame shape; a context that has seen many
        // shapes drops them between frames, when no frame in flight reads them)
        if (c->async_pending == 0 && (c->mt_bandtabs.size() >= 16 || c->mt_end_polys.size() >= 64)) {
            HIP_TRY(hipDeviceSynchronize());
            c->mt_bandtabs.clear();
            c->mt_end_polys.clear();
        }
        // a whole frame with nothing in flight (synchronous, or the first of a pipeline): short segments in
        // band mode (srt_ctx::mt_short); later pipelined frames generate behind their predecessors in
        // band-mode segments of mt_pipe_split doubles (0: the tabulated 2^19-word segments)
        const int64_t whole_split = n_rows < Hf ? 0
                                  : c->async_pending == 0 ? c->mt_short
                                                                               : c->mt_pipe_split;
        if (use_mt && c->mt_bands_on && (n_rows < Hf || whole_split > 0)) {
            const int last_ns = a->spp - (F.npass - 1) * batch;
            const int64_t split = n_rows < Hf ? (int64_t)1 << 18 : whole_split;
            for (int k = 0; k < 2; ++k) {
                if ((rc = mt_band_table(c, W, Hf, k == 0 ? batch : last_ns, mt_pm, rows, n_rows, split, &mt_bt[k])))
                    return rc;
                if (mt_bt[k]) mt_win_need = std::max(mt_win_need, (int64_t)(mt_bt[k]->nseg + 1) * rtmt::N);
            }
            if (!mt_bt[0] || !mt_bt[1]) mt_bt[0] = mt_bt[1] = nullptr;
        }
        // band mode stores a shard's jitter in its own layout [s][plane][its rows][W] (1/N of the frame's)
        // when every pass generates in band mode (a pass whose generation ends inside the key window
        // takes the tabulated segments and the frame's layout)
        auto pass_words = [&](int ns, bool last) { return 2 * ((int64_t)ns * 4 * W * Hf + (last ? 4 * W * Hf : 0)); };
        const bool jit_compact = mt_bt[0] && rtmt::end_jump(pass_words(a->spp - (F.npass - 1) * batch, true)) > 0 &&
                                 (F.npass == 1 || rtmt::end_jump(pass_words(batch, false)) > 0);
        jit_doubles = use_mt ? (int64_t)batch * 4 * (jit_compact ? npix : W * Hf)
                             : (a->jitter && !jit_dev ? (int64_t)batch * 4 * npix : 0);
        return SRT_OK;
    }

    FrameNeeds needs() const {
        const bool root = sharded && c->rank == 0;  // receives every rank's tiles and assembles the frame
        FrameNeeds N;
        N.fb = N.rgb = N.u8 = 3 * npix;
        N.fbg = F.groups > 1 ? (int64_t)F.groups * 3 * npix : 0;
        N.fbx = fx_words(npix);
        N.jit = jit_doubles;
        N.mt_win = use_mt ? mt_win_need : 0;
        N.hit = a->out_hit_id && !hit_dev ? (int64_t)F.batch * npix : 0;
        N.full_u8 = (a->flags & SRT_RENDER_RGBX) ? 4 * npix : (reh_n || root) ? 3 * W * Hf : 0;
        N.g_u8 = reh_n ? reh_n * reh_maxpix * 3 : root ? c->nranks * maxpix * 3 : 0;
        N.g_u8_zeroed = reh_n > 0;
        N.g_rgb = root && gather_rgb ? c->nranks * maxpix * 3 : 0;
        N.full_rgb = root && gather_rgb ? 3 * W * Hf : 0;
        if (F.frame)  // (a split ring: each half that size)
            N.ring_rays = (int64_t)FRAME_BLOCK * (c->fanout + 2) * 2 * (frame_split_for(V->mats) ? 2 : 1);
        else
            N.queue_rays = (int64_t)F.batch * npix * c->fanout;
        N.events = F.npass * F.nev;
        // per-pass counters and flags come back through pinned memory once, at the end of the
        // frame: the passes, the resolve and the output copies are queued without a host round trip.
        // After the passes' words: the shadow-ray count (2 words), k_resolve's fixed-point range flag (1)
        N.host_words = F.npass * F.pass_words + 3;
        return N;
    }

    // Camera tables (shared by the slots): room for them, then uploaded only when they change (a
    // render loop re-sends the same ones)
    bool camera_tables_hold() const { return W <= c->xs.cap && Hf <= c->ys.cap && n_rows <= c->rows.cap; }
    int upload_camera(hipStream_t st) {
        int rc;
        const void* old[3] = {c->xs, c->ys, c->rows};
        if ((rc = c->xs.ensure(W))) return rc;
        if ((rc = c->ys.ensure(Hf))) return rc;
        if ((rc = c->rows.ensure(n_rows))) return rc;
        const void* now[3] = {c->xs, c->ys, c->rows};
        for (int k = 0; k < 3; ++k)
            if (old[k] != now[k]) c->cam_host[k].clear();
        if ((rc = upload_if_changed(c, st, c->xs, c->cam_host[0], cam->xs, (size_t)W * 8))) return rc;
        if ((rc = upload_if_changed(c, st, c->ys, c->cam_host[1], cam->ys, (size_t)Hf * 8))) return rc;
        return upload_if_changed(c, st, c->rows, c->cam_host[2], rows, (size_t)n_rows * 4);
    }

    // resolve targets: outputs in device memory are written in place by the resolve; host outputs
    // are resolved into the slot buffers and copied by DMA on the frame's stream (57 GB/s measured
    // for the ex1 1080p RGB, against 28 GB/s for a resolve kernel storing straight into pinned
    // memory over PCIe); a shard resolves into its slot tiles (gathered afterwards)
    void set_resolve_targets(const FrameSlot& f) {
        const bool rgb_local = (a->flags & SRT_RENDER_RGB_LOCAL) != 0;
        res_rgb = rgb_local ? f.rgb
                : sharded ? ((gather_rgb || rgb_rows) ? f.rgb : nullptr)
                          : a->out_rgb ? (rgb_dev ? a->out_rgb : f.rgb) : nullptr;
        rgbx = (a->flags & SRT_RENDER_RGBX) && a->out_srgb8;
        res_u8 = (sharded || rgbx) ? f.u8 : a->out_srgb8 ? (u8_dev ? a->out_srgb8 : f.u8) : nullptr;
    }

    // The stream the frame's numpy-stream generation runs on and the state it starts from.  `pf`:
    // pass 0's generation was queued by srt_render_prefetch (nothing to wait for or copy)
    int begin_stream(FrameSlot& f, const srt_ctx::MtPrefetch* pf, StreamCursor& sc) const {
        // the stream the numpy-stream generation runs on: the MT stream for a single-pass frame
        // (it waits until the slot's previous frame has read its jitter), else the frame's stream
        sc.mst = f.stream;
        if (!use_mt) return SRT_OK;
        // (auto: whole frames on the high-priority stream, shards on the frame's stream: a stream
        // shared by the frames serialises their generations, and a shard's band segments -- one
        // serial generator block each -- are long: a rank of 2's 130k-double bands take ~0.4 ms)
        if (F.npass == 1 && mts) {
            if (!c->mt_stream) {
                // a high-priority queue (mt_stream 2): the generation's blocks are dispatched ahead
                // of the trace kernels' as CUs free up
                int lo = 0, hi = 0;
                if (mts == 2 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
                    HIP_TRY(hipStreamCreateWithPriority(&c->mt_stream, hipStreamNonBlocking, hi));
                else
                    HIP_TRY(hipStreamCreateWithFlags(&c->mt_stream, hipStreamNonBlocking));
            }
            sc.mst = c->mt_stream;
            if (f.jit_busy && !pf) HIP_TRY(hipStreamWaitEvent(sc.mst, f.jit_free, 0));
        }
        // this frame's stream starts where the previous frame's ended (device dump window) or at
        // the caller's state
        if (c->mt_done && !pf) HIP_TRY(hipStreamWaitEvent(sc.mst, c->mt_done, 0));
        // the numpy stream continues on the device from the previous asynchronous frame (same `mt`)
        if (async && c->async_pending > 0 && c->mt_chain == a->mt) {
            sc.key = mt_dump(c);
            sc.pos = c->mt_pos;
        } else {
            if (!pf) HIP_TRY(hipMemcpyAsync(mt_key0(c), a->mt->key, rtmt::N * 4, hipMemcpyHostToDevice, sc.mst));
            sc.key = mt_key0(c);
            sc.pos = a->mt->pos;
        }
        return SRT_OK;
    }

    // Queue the generation of pass p's samples of the whole frame's stream (then the sizing draw after
    // the last pass; a shard reads its rows by global pixel) into the slot's jitter buffer, unless
    // srt_render_prefetch queued it (`pf`, pass 0).  *band: the jitter is in the shard's own layout;
    // *gen_on: the stream the generators run on
    int queue_pass_stream(FrameSlot& f, int p, StreamCursor& sc, const srt_ctx::MtPrefetch* pf, bool* band,
                          hipStream_t* gen_on) const {
        const int ns = std::min(F.batch, F.spp - p * F.batch);
        const bool last = p + 1 == F.npass;
        int rc;
        const int64_t n_out = (int64_t)ns * 4 * W * Hf;
        const int64_t n_skip = last ? 4 * W * Hf : 0;
        if (p > 0) sc.key = mt_dump(c);  // the previous pass's final window
        // a pipelined one-pass frame: its final window (the next frame's key) by one jump, so
        // the next frame's generation starts once this one's jump kernel has run
        const int64_t n_words = 2 * (n_out + n_skip);
        const srt_ctx::MtBandTab* bt = mt_bt[last ? 1 : 0];
        *band = bt && rtmt::end_jump(n_words) > 0;
        const bool end = *band || (async && F.npass == 1 && n_words <= (int64_t)rtmt::SEGS * rtmt::L &&
                                   rtmt::end_jump(n_words) > 0);
        const uint32_t* end_poly = nullptr;
        if (end && (rc = mt_end_poly_for(c, n_words, &end_poly))) return rc;
        // (a pinhole camera reads only the pixel-jitter planes 0 and 1 of each sample)
        *gen_on = sc.mst;
        if (pf && p == 0) {  // queued by srt_render_prefetch
            sc.pos = pf->final_pos;
            *gen_on = pf->gen_on;
            c->pf_used++;
            return SRT_OK;
        }
        if (*band) {
            if ((rc = mt_launch_bands(c, sc.mst, f.mt_win, sc.key, sc.pos, n_words, *bt, f.jit, &sc.pos, end_poly,
                                      last ? c->mt_done : nullptr, sc.mst, f.mt_jumped, gen_on)))
                return rc;
        } else if ((rc = mt_launch(c, sc.mst, f.mt_win, sc.key, sc.pos, n_out, n_skip, f.jit, &sc.pos, W * Hf, mt_pm,
                                   end_poly, end ? (int64_t)rtmt::end_jump(n_words) : 0, end ? c->mt_done : nullptr,
                                   sc.mst, f.mt_jumped, gen_on))) {
            return rc;
        }
        // otherwise the next frame's stream may start as soon as this one's is generated
        if (last && !end) HIP_TRY(hipEventRecord(c->mt_done, sc.mst));
        return SRT_OK;
    }

    // what identifies a prefetched generation besides the stream state (srt_ctx::MtPrefetch::shape)
    void prefetch_shape(const FrameSlot& f, int64_t shape[8]) const {
        const int64_t s[8] = {W, Hf, a->spp, F.batch, mt_pm, (int64_t)(&f - c->slots), mts,
                              (int64_t)c->mt_bands_on * 2 + (c->mt_short > 0)};
        memcpy(shape, s, sizeof s);
    }

    // srt_render_prefetch after the planning and buffer setup it shares with srt_render: pass 0's
    // generation of a one-pass frame is queued and described in srt_ctx::pf
    int queue_prefetch(FrameSlot& f) const {
        if (F.npass != 1 || !mts) return SRT_OK;  // (the generation would run on the frame's stream)
        StreamCursor sc;
        bool band;
        hipStream_t gen_on;
        int rc;
        if ((rc = begin_stream(f, nullptr, sc))) return rc;
        if ((rc = queue_pass_stream(f, 0, sc, nullptr, &band, &gen_on))) return rc;
        // queued: the frame's stream waits for it when srt_render comes (a wait queued
        // here would also hold up the scene upload's synchronisation of that stream)
        srt_ctx::MtPrefetch& q = c->pf;
        memcpy(q.key, a->mt->key, sizeof q.key);
        q.pos = a->mt->pos;
        prefetch_shape(f, q.shape);
        q.bt[0] = mt_bt[0];
        q.bt[1] = mt_bt[1];
        q.final_pos = sc.pos;
        q.gen_on = gen_on;
        q.valid = true;
        c->pf_queued++;
        return SRT_OK;
    }

    // this frame's first-pass generation already queued by srt_render_prefetch (same stream state,
    // same frame shape, nothing generated since): not launched again (the first iteration only)
    bool prefetched(const FrameSlot& f, const srt_ctx::MtPrefetch& pf) const {
        if (!pf.valid || !whole_sync_mt_frame() || F.npass != 1 || !mts) return false;
        int64_t shape[8];
        prefetch_shape(f, shape);
        return !memcmp(pf.shape, shape, sizeof shape) && pf.bt[0] == mt_bt[0] && pf.bt[1] == mt_bt[1] &&
               pf.pos == a->mt->pos && !memcmp(pf.key, a->mt->key, sizeof pf.key);
    }

    // A k_frame pass: the whole pass in one launch, one wave per 64-pixel tile
    int launch_frame_pass(FrameSlot& f, TraceParams& P, int ns, hipEvent_t* ev) const {
        P.ring = f.ring;
        P.ring_lock = f.ring_lock;
        P.ring_cap = f.ring_cap;
        P.nslot = f.nslot;
        P.cnt_out = f.counts;
        P.groups = std::min(F.groups, ns);
        P.ntiles = (int)ntiles;
        P.fbg = f.fbg;
        P.fuse_resolve = (F.npass == 1 && F.groups == 1);
        HIP_TRY(hipEventRecord(ev[0], f.stream));
        hipLaunchKernelGGL(V->frame, dim3((unsigned)(ntiles * P.groups)), dim3(FRAME_BLOCK), lut_bytes(c), f.stream, P);
        HIP_TRY(hipGetLastError());
        if (P.groups > 1) {
            hipLaunchKernelGGL(k_fb_groups, dim3(grid_for(3 * npix, c->max_blocks)), dim3(BLOCK), 0, f.stream, f.fb,
                               (const double*)f.fbg, P.groups, npix, (int)P.fb_first);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev[1], f.stream));
        HIP_TRY(hipEventRecord(ev[F.dcap + 1], f.stream));
        return SRT_OK;
    }

    // A pass of the per-depth kernels: depth 0 (raygen fused with the trace step; every depth of a
    // fused frame), then one launch per deeper depth.  `own_mt`: the jitter was generated on the MT stream
    int launch_wavefront_pass(FrameSlot& f, TraceParams& P, int64_t nrays, hipEvent_t* ev, bool own_mt) const {
        P.depth = 0;
        P.n_primary = nrays;
        P.qout = f.q[1];
        P.cnt_out = f.counts + NSHARD;
        HIP_TRY(hipEventRecord(ev[0], f.stream));
        // a single-pass fused frame resolves its pixels in k_primary (no framebuffer)
        P.fuse_resolve = F.fuse && F.npass == 1;
        // grid: frames in flight overlap one frame's tail with the next, and fewer, longer blocks
        // (grid-stride, max_blocks: four rounds of the resident blocks) leave the numpy-stream
        // generators of the frames behind more room; a synchronous frame has nothing to overlap,
        // so it takes one block per 256 threads and the hardware fills the tail as blocks finish
        // (same box, ex1 1080p: the synchronous launch 0.950 -> 0.908 ms; pipelined frames with the
        // full grid 0.902 -> 0.986 ms, profiles/r05_primary_grid_ab.txt)
        // the lean kernel of pipelined whole frames (its generators beside it): two blocks per CU,
        // each grid-striding over ~30 wave iterations of a 1080p frame; the frames in flight fill
        // the rest of the CU (ex1 1080p: 0.878 ms per frame at 3072 blocks, 0.838 at 512; a rank of
        // 8's shard, 2025 blocks at most, was slower with it: profiles/r05_lean_grid_ab.txt).  A
        // pipeline's first frame, with nothing in flight to fill the CUs around its blocks, keeps
        // the full four rounds (max_blocks).
        // (option sync_lean: synchronous frames take the lean kernel too -- bench.py times the pipelined
        // frames' kernel alone that way for its roofline)
        const bool lean = F.fuse && (async || c->sync_lean) && V->lean;
        if (lean) c->lean_launches++;
        const int pgrid = !async ? INT_MAX
                                 : (!lean || c->async_pending == 0               ? c->max_blocks
                                    : n_rows == Hf && c->lean_blocks > 0              ? c->lean_blocks
                                    : n_rows < Hf && c->lean_blocks_shard > 0         ? c->lean_blocks_shard
                                                                                        : c->max_blocks);
        hipLaunchKernelGGL(F.fuse ? (lean ? (c->lane_stats && V->lean_stats ? V->lean_stats : V->lean) : V->fused) : V->primary,
                           dim3(grid_for(((npix * P.pix_groups + 63) / 64) * 64, pgrid)), dim3(BLOCK),
                           lut_bytes(c), f.stream, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[1], f.stream));
        if (F.fuse)  // every depth traced: the deeper depths' events mark the same point
            for (int d = 1; d <= F.dcap; ++d) HIP_TRY(hipEventRecord(ev[1 + d], f.stream));
        if (own_mt) {  // the next generation into this slot may start
            HIP_TRY(hipEventRecord(f.jit_free, f.stream));
            f.jit_busy = true;
        }
        P.fb_first = 0;
        for (int d = 1; d <= F.dcap && !F.fuse; ++d) {
            if (F.chain_from > 0 && d > F.chain_from) break;  // traced by the chain kernel
            P.depth = d;
            P.qin = f.q[d & 1];
            P.qout = f.q[(d + 1) & 1];
            P.cnt_in = f.counts + (int64_t)d * NSHARD;
            P.cnt_out = f.counts + (int64_t)(d + 1) * NSHARD;
            P.chain = (d == F.chain_from);
            hipLaunchKernelGGL(P.chain ? V->chain : V->trace, dim3(trace_grid(c)), dim3(BLOCK), lut_bytes(c), f.stream, P);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[1 + d], f.stream));
        }
        return SRT_OK;
    }

    // Queue pass p: its jitter (generated, copied or the caller's), its kernels, its counters' hand-over
    int queue_pass(FrameSlot& f, int p, StreamCursor& sc, const srt_ctx::MtPrefetch* pf) const {
        const int s0 = p * F.batch;
        const int ns = std::min(F.batch, a->spp - s0);
        const int64_t nrays = (int64_t)ns * npix;
        int rc;
        TraceParams P = base_params(c, f, a->seed);
        P.fb = f.fb;
        P.fbx = (c->deterministic && c->fx_ok) ? f.fbx : nullptr;
        P.fb_first = (p == 0);  // the first pass's depth-0 kernel stores the framebuffer (no memset)
        // sample groups per pixel (k_primary): one (all of the pass's samples in one thread, summed
        // in registers) unless the frame has too few pixels to fill the GPU -- one GPU's shard of a
        // multi-GPU frame -- then 2, 4, .. groups on lanes of the pixel's wave (their fixed-point
        // sums are exact in any grouping: the image does not depend on it).  Enough means one
        // round of the resident threads for the per-depth kernels (a 1/8 shard of ex1 1080p, 261k
        // pixels: 6 samples per thread 118 us, 1 sample 133 us) and two for the fused paths, whose
        // threads trace whole paths (long tails: a 1/8 shard on one group per pixel 0.35 ms, 1.3
        // rounds, against 0.29 ms on the per-depth kernels)
        P.pix_groups = pix_groups(c, npix, ns, F.fuse);
        P.npix = npix;
        P.cam = *cam;
        P.cam.xs = c->xs;
        P.cam.ys = c->ys;
        P.rows = c->rows;
        P.sample_base = a->sample_base + s0;
        P.spp = ns;
        P.jit_plane = npix;
        P.dcap = F.dcap;
        P.out_rgb = res_rgb;
        P.out_u8 = res_u8;
        P.spp_total = a->spp;
        if (use_mt) {
            bool band;
            hipStream_t gen_on;
            if ((rc = queue_pass_stream(f, p, sc, pf, &band, &gen_on))) return rc;
            if (gen_on != f.stream) {
                HIP_TRY(hipEventRecord(f.jit_ready, gen_on));
                HIP_TRY(hipStreamWaitEvent(f.stream, f.jit_ready, 0));
            }
            P.jitter = f.jit;
            P.jit_plane = band ? npix : W * Hf;
            P.jit_global = band ? 0 : 1;
        } else if (a->jitter) {
            const double* src = a->jitter + (int64_t)s0 * 4 * npix;
            if (jit_dev) {
                P.jitter = src;
            } else {
                HIP_TRY(hipMemcpyAsync(f.jit, src, (size_t)nrays * 4 * 8, hipMemcpyHostToDevice, f.stream));
                P.jitter = f.jit;
            }
        }
        if (a->out_hit_id) P.hit_out = hit_dev ? a->out_hit_id + (int64_t)s0 * npix : f.hit;
        hipEvent_t* ev = f.ev.data() + (int64_t)p * F.nev;
        const bool own_mt = sc.mst != f.stream;
        if ((rc = F.frame ? launch_frame_pass(f, P, ns, ev) : launch_wavefront_pass(f, P, nrays, ev, own_mt))) return rc;
        if (F.frame && own_mt) {  // the next generation into this slot may start
            HIP_TRY(hipEventRecord(f.jit_free, f.stream));
            f.jit_busy = true;
        }
        uint32_t* hp = f.host + p * F.pass_words;
        // counters of this pass -> pinned host words [0, used_words) (the unused depths are zero
        // on the host), flags OR-ed into the two words at [cnt_words, cnt_words + 2); the last
        // pass's are handed over by k_resolve
        if (p + 1 < F.npass) {
            hipLaunchKernelGGL(k_pass_end, dim3(1), dim3(BLOCK), 0, f.stream, f.counts, used_words, f.flags, hp,
                               hp + F.cnt_words);
            HIP_TRY(hipGetLastError());
        }
        if (a->out_hit_id && !hit_dev)
            HIP_TRY(hipMemcpyAsync(a->out_hit_id + (int64_t)s0 * npix, f.hit, (size_t)nrays * 4, hipMemcpyDeviceToHost,
                                   f.stream));
        return SRT_OK;
    }

    // After the passes: the resolve, then the frame's outputs on their way (a shard's rows of the
    // linear RGB and its gather's description; the rehearsed assembly, RGBX pixels, host copies)
    int queue_outputs(FrameSlot& f) const {
        uint32_t* hshadow = f.host + F.npass * F.pass_words;
        // (a single-pass frame kernel or fused frame has resolved its pixels: k_resolve only hands over
        // the counters and the shadow count)
        const bool fused = F.npass == 1 && ((F.frame && F.groups == 1) || F.fuse);
        uint32_t* hlast = f.host + (F.npass - 1) * F.pass_words;
        hipLaunchKernelGGL(k_resolve, dim3(fused ? 1 : grid_for(npix, c->max_blocks)), dim3(BLOCK), 0, f.stream, f.fb,
                           (F.frame || !c->deterministic || !c->fx_ok) ? nullptr
                                                                       : (const unsigned long long*)f.fbx,
                           fused ? (int64_t)0 : npix, f.shadow, hshadow, (double)a->spp, res_rgb, res_u8, f.counts,
                           used_words, f.flags, hlast, hlast + F.cnt_words);
        HIP_TRY(hipGetLastError());
        f.dirty = false;  // the kernels above leave counts/flags/shadow zeroed
        // this rank's rows of the linear RGB into the shared host frame: per plane, the rank's band j
        // at frame band j n + rank, one pitched copy of the full bands, then a short last band
        if (rgb_rows) {
            const int64_t band_px = band * W;
            const int64_t nb = npix / band_px, tail = npix - nb * band_px;
            for (int pl = 0; pl < 3; ++pl) {
                double* dst = a->out_rgb + (int64_t)pl * W * Hf;
                const double* src = f.rgb + (int64_t)pl * npix;
                if (nb > 0)
                    HIP_TRY(hipMemcpy2DAsync(dst + (int64_t)c->rank * band_px, (size_t)(c->nranks * band_px * 8), src,
                                             (size_t)(band_px * 8), (size_t)(band_px * 8), (size_t)nb,
                                             hipMemcpyDeviceToHost, f.stream));
                if (tail > 0) {
                    // (the rank's band nb, in period nb)
                    const int64_t bt = nb * c->nranks + c->rank;
                    HIP_TRY(hipMemcpyAsync(dst + bt * band_px, src + nb * band_px, (size_t)(tail * 8),
                                           hipMemcpyDeviceToHost, f.stream));
                }
            }
        }
        // the shard's tiles to rank 0 (RCCL over xGMI), assembled into the frame there
        FrameSlot::Gather& G = f.gather;
        G = FrameSlot::Gather{};
        if (sharded) {
            G.on = true;
            G.W = W;
            G.H = Hf;
            G.npix = npix;
            G.maxpix = maxpix;
            G.band = band;
            G.want_u8 = true;
            G.want_rgb = gather_rgb;
            if (c->rank == 0) {
                G.dst_u8 = (a->out_srgb8 && u8_dev) ? a->out_srgb8 : f.full_u8;
                G.dst_rgb = (a->out_rgb && rgb_dev) ? a->out_rgb : f.full_rgb;
                G.host_u8 = (a->out_srgb8 && !u8_dev) ? a->out_srgb8 : nullptr;
                G.host_rgb = (a->out_rgb && !rgb_dev && gather_rgb) ? a->out_rgb : nullptr;
            }
            return SRT_OK;  // (the gather hands the frame to the caller)
        }
        const uint8_t* u8_src = f.u8;
        int64_t u8_bytes = 3 * npix;
        if (reh_n) {
            GatherTiles T{};
            for (int q = 0; q < reh_n; ++q) {
                T.u8[q] = q == 0 ? f.u8 : f.g_u8 + (int64_t)q * reh_maxpix * 3;
                T.npix[q] = shard_rank_rows(Hf, reh_n, q, reh_band) * W;
            }
            hipLaunchKernelGGL(k_assemble, dim3(grid_for(W * Hf, c->max_blocks)), dim3(BLOCK), 0, f.stream, T, reh_n,
                               reh_band, W, Hf, f.full_u8, (double*)nullptr);
            HIP_TRY(hipGetLastError());
            u8_src = f.full_u8;
            u8_bytes = 3 * W * Hf;
        }
        if (rgbx) {
            uint32_t* dst4 = reinterpret_cast<uint32_t*>(u8_dev ? a->out_srgb8 : f.full_u8);
            hipLaunchKernelGGL(k_rgbx, dim3(grid_for(npix, c->max_blocks)), dim3(BLOCK), 0, f.stream, f.u8, dst4,
                               npix);
            HIP_TRY(hipGetLastError());
            u8_src = f.full_u8;
            u8_bytes = 4 * npix;
        }
        // host outputs (pinned, for an asynchronous frame) are copied on the frame's stream
        if (a->out_srgb8 && !u8_dev)
            HIP_TRY(hipMemcpyAsync(a->out_srgb8, u8_src, (size_t)u8_bytes, hipMemcpyDeviceToHost, f.stream));
        if (a->out_rgb && !rgb_dev)
            HIP_TRY(hipMemcpyAsync(a->out_rgb, f.rgb, (size_t)3 * npix * 8, hipMemcpyDeviceToHost, f.stream));
        return SRT_OK;
    }

    // Queue the whole frame on its slot's stream: the passes, the resolve, the outputs.  `pf`: pass
    // 0's stream generation as srt_render_prefetch queued it, or null
    int queue_frame(FrameSlot& f, const srt_ctx::MtPrefetch* pf) const {
        int rc;
        if (f.pending == 0) clear_host_flags(f, F);  // k_pass_end ORs into them
        if (f.dirty) {
            HIP_TRY(hipMemsetAsync(f.shadow, 0, 8 * NSHARD, f.stream));
            HIP_TRY(hipMemsetAsync(f.counts, 0, (size_t)F.cnt_words * 4, f.stream));
            HIP_TRY(hipMemsetAsync(f.flags, 0, 8, f.stream));
        }
        f.dirty = true;
        StreamCursor sc;
        if ((rc = begin_stream(f, pf, sc))) return rc;
        for (int p = 0; p < F.npass; ++p)
            if ((rc = queue_pass(f, p, sc, pf))) return rc;
        if (use_mt) c->mt_pos = sc.pos;
        return queue_outputs(f);
    }
};

// srt_render, or with `prefetch` srt_render_prefetch: the same planning and buffer setup, then only
// the first pass's numpy-stream generation is queued (queue_prefetch) and the call returns
int render_impl(srt_ctx* c, const srt_camera* cam, const srt_render_args* a, srt_stats* st, bool prefetch) {
    auto t_start = std::chrono::steady_clock::now();
    if (!c || !cam || !a) return fail(SRT_ERR_ARG, "null argument");
    const srt_ctx::MtPrefetch pf_in = c->pf;  // (a prefetch is used by the next render only)
    c->pf.valid = false;
    RenderCall r{c, cam, a};
    int rc;
    if ((rc = r.check_args(prefetch))) return rc;
    // a prefetch of any other frame does nothing (nor of a frame of several passes: queue_prefetch)
    if (prefetch && !r.whole_sync_mt_frame()) return SRT_OK;
    if ((rc = r.select_rows())) return rc;
    r.plan_frame();
    // the slot of this frame: slot 0 for a synchronous frame (after the frames in flight),
    // alternating slots for asynchronous ones
    FrameSlot& f = r.async ? c->slots[c->next_slot] : c->slots[0];
    if (r.async && (rc = ensure_slot(f))) return rc;
    c->f = &f;
    if (!r.async && (rc = wait_frames(c, nullptr))) return rc;
    if ((rc = r.plan_stream())) return rc;
    const FrameNeeds N = r.needs();
    // frames in flight use the buffers below: a frame that would reallocate anything first waits
    // for them (and reports their errors)
    if (r.async && c->async_pending > 0) {
        const FramePlan& pp = f.pending ? f.plan : c->slots[c->last_slot].plan;
        const bool fits = same_shape(r.F, pp) && r.camera_tables_hold() && !(r.use_mt && c->mt_dirty) && slot_holds(c, f, N);
        if (!fits && (rc = wait_frames(c, nullptr))) return rc;
    }
    if ((rc = r.upload_camera(f.stream))) return rc;
    if (r.use_mt && (rc = mt_ensure(c))) return rc;
    // per-slot buffers of this frame shape (for an asynchronous frame also those of the other slots
    // while they are idle, so that the pipeline's first frame on them allocates nothing)
    if ((rc = grow_slot(c, f, N))) return rc;
    if (r.async || c->pipeline) {
        for (int k = 0; k < c->nslots; ++k) {
            FrameSlot& other = c->slots[k];
            if (&other != &f && other.pending == 0) {
                if ((rc = ensure_slot(other))) return rc;
                if ((rc = grow_slot(c, other, N))) return rc;
            }
        }
    }
    if (r.use_mt && !c->mt_done) HIP_TRY(hipEventCreateWithFlags(&c->mt_done, hipEventDisableTiming));
    // generator width: four waves (one per SIMD) beside the lean fused kernel of the frames in flight
    c->gen_nt = c->mt_gen_nt_opt ? c->mt_gen_nt_opt
                                 : ((r.async && r.F.fuse && r.V->lean != nullptr) ? 256 : rtmt_dev::MT_GEN_THREADS);
    r.set_resolve_targets(f);
    if (prefetch) return r.queue_prefetch(f);
    const srt_ctx::MtPrefetch* pf = r.prefetched(f, pf_in) ? &pf_in : nullptr;
    srt_stats S{};
    for (;;) {
        if ((rc = r.queue_frame(f, pf))) return rc;
        if (r.async) {
            // (a synchronous frame gathers after its retries: every rank gathers each frame once)
            if (r.sharded && !c->defer_gather && (rc = gather_frame(c))) return rc;
            // stats and errors come with srt_render_finish; the next asynchronous frame goes to the next slot
            if (r.use_mt) c->mt_chain = a->mt;
            c->async_pending++;
            f.pending++;
            f.plan = r.F;
            c->last_slot = (int)(&f - c->slots);
            c->next_slot = (c->last_slot + 1) % c->nslots;
            return SRT_OK;
        }
        f.dirty = true;
        HIP_TRY(hipStreamSynchronize(f.stream));
        f.dirty = false;
        const int64_t retries = S.retries;
        uint32_t bits = 0;
        rc = collect_frame(c, f, r.F, S, &bits);
        if (rc == SRT_RETRY) {
            // render the frame again: without chain mode after a tie gave a chained ray a second
            // child (the same tie would recur), with bigger queues after an overflow
            S.retries = retries + 1;
            if (S.retries > 8) return fail(SRT_ERR_MEMORY, "ray queues keep overflowing");
            if (bits & RETRY_CHAIN_TIE) {
                r.F.chain_from = 0;
                r.F.fuse = false;
            }
            if ((bits & RETRY_OVERFLOW) &&
                (rc = r.F.frame ? ensure_ring(c, f, 2 * f.ring_cap) : ensure_queues(f, 2 * f.seg * NSHARD)))
                return rc;
            pf = nullptr;  // (the retry generates its stream again from the caller's state)
            continue;
        }
        S.retries = retries;
        if (rc) return rc;
        break;
    }
    if (r.sharded && !c->defer_gather) {
        if ((rc = gather_frame(c))) return rc;
        HIP_TRY(hipStreamSynchronize(f.stream));
    }
    if (r.use_mt) {  // numpy's state after this frame's draws
        HIP_TRY(hipMemcpy(a->mt->key, mt_dump(c), rtmt::N * 4, hipMemcpyDeviceToHost));
        a->mt->pos = c->mt_pos;
    }
    if (st) {
        S.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        *st = S;
    }
    return SRT_OK;
}

}  // namespace
