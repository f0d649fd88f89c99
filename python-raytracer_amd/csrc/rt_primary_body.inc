// rt_primary_body.inc -- the body of k_primary and k_primary_lean (rt_trace_kernels.h), included in both
// kernels' definitions so that each reads its arguments in place from the kernel argument segment
// (a __device__ function taking them by reference made the fused kernels' loads of them vector loads:
// 23 -> 27 spilled VGPRs).  In scope: MATS, OCC, FUSE, LEAN and the kernel argument P0.
// LEAN (k_primary_lean): the pixel's camera coordinates and the sample's jitter are read at each
// sample's start instead of being held across the path (and prefetched a sample ahead): fewer
// registers live across the traced path, for the kernel built to 160 VGPRs.  LANE_STATS (the
// k_primary_lean instantiation srt_debug_lane_stats selects): count the depth loop's lanes.
    const TraceParams& P = P0;  // (read in place from the kernel arguments)
    stage_luts(P);
    const uint32_t shard = blockIdx.x % NSHARD;
    uint32_t err = 0;
    uint32_t shadow = 0;
    const bool fx = P.fbx != nullptr;
    const int ppw = 64 / P.pix_groups;  // pixels per wave
    const int lane = threadIdx.x & 63;
    const int grp = lane / ppw;
    const int spg = (P.spp + P.pix_groups - 1) / P.pix_groups;
    const int s_begin = min(P.spp, grp * spg), s_end = min(P.spp, s_begin + spg);
    // the fused paths' wave takes a tile of 8 x ppw / 8 pixels (8 x 4 at two sample groups) instead of
    // ppw consecutive pixels of a row: a square-ish tile straddles fewer object edges, so fewer of its
    // waves run a deeper depth for a few lanes and fewer shade several colliders in turn.  ex1 1080p,
    // same box: 336,422 -> ~331,000 wave iterations per frame (profiles/r06_lane_utilisation.txt),
    // pipelined frame 0.776 -> 0.760 ms, k_primary_lean 0.898 -> 0.852 ms (profiles/r06_wave_tile_ab.txt).
    // Not for the BVH kernel (its register pressure: 121 -> 149 spilled VGPRs, no faster).  (The host
    // keeps these launches at <= 8 sample groups, so ppw >= 8: pix_groups.)
    constexpr bool TILE = FUSE && !(MATS & MAT_BVH);
    const uint32_t Wc = (uint32_t)P.cam.width, nrows = (uint32_t)(P.npix / P.cam.width);
    const uint32_t th = (uint32_t)ppw >> 3, tiles_x = (Wc + 7u) >> 3;
    const int64_t nwaves = TILE ? (int64_t)tiles_x * ((nrows + th - 1u) / th) : (P.npix + ppw - 1) / ppw;
    const Quot qw((double)P.cam.width), qh((double)P.cam.height);
    // (the wave index is wave-uniform: readfirstlane keeps it and what derives from it in SGPRs)
    for (int64_t wv = (int64_t)blockIdx.x * (BLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
         wv < nwaves; wv += (int64_t)gridDim.x * (BLOCK / 64)) {
        const int64_t p0 = wv * ppw;
        uint32_t p, lr, col;  // the lane's pixel of the pass, its local row and column
        bool pact;
        if (TILE) {
            const uint32_t ty = (uint32_t)wv / tiles_x, tx = (uint32_t)wv - ty * tiles_x;
            uint32_t li = threadIdx.x;
            asm volatile("" : "+v"(li));  // (recomputed per wave iteration, not held across it)
            li &= (uint32_t)(ppw - 1);
            const uint32_t r = ty * th + (li >> 3), cx = tx * 8u + (li & 7u);
            pact = r < nrows && cx < Wc;
            lr = pact ? r : 0u;
            col = pact ? cx : 0u;
            p = lr * Wc + col;
        } else {
            p = (uint32_t)(p0 + (lane & (ppw - 1)));
            pact = p < (uint64_t)P.npix;
            lr = pact ? p / (uint32_t)P.cam.width : 0u;
            col = pact ? p - lr * (uint32_t)P.cam.width : 0u;
        }
        const bool active = pact && s_begin < s_end;
        const int grow = pact ? P.rows[lr] : 0;
        const double xc = pact ? P.cam.xs[col] : 0.0, yr = pact ? P.cam.ys[grow] : 0.0;  // (LEAN: per sample)
        const uint32_t gpix = (uint32_t)grow * (uint32_t)P.cam.width + col;
        const int s_stop = active ? s_end : s_begin;  // (no samples for a lane past the frame's end)
        PixAcc acc;
        // software pipeline (not LEAN): the next sample's pixel jitter is loaded while this sample is
        // traced (the lens-disk pair of a thin-lens camera is loaded when used: two fewer doubles live
        // across the trace for the pinhole cameras of every example)
        double jn[2] = {0.0, 0.0};
        if (!LEAN && active) primary_jitter(P, s_begin, p, gpix, jn);
        for (int s = s_begin; s < s_stop; ++s) {
            Ray r;
            r.o = r.d = d3{0.0, 0.0, 0.0};
            r.w = d3{1.0, 1.0, 1.0};
            r.meta = pack_meta(0, 0, 0);
            r.pix = p;
            r.path = mix32(0x5EED0000u, (uint32_t)(P.sample_base + s));
            RT_T0(tr0);
            double j[4] = {jn[0], jn[1], 0.0, 0.0};
            if constexpr (LEAN) {
                primary_jitter(P, s, p, gpix, j);
                // (opaque indices: the loads stay in the loop instead of being hoisted out of it)
                uint32_t colr = col, growr = (uint32_t)grow;
                asm volatile("" : "+v"(colr), "+v"(growr));
                const double xl = P.cam.xs[colr], yl = P.cam.ys[growr];
                const Quot qwl((double)P.cam.width), qhl((double)P.cam.height);  // (a few VALU per sample)
                if (P.cam.lens_radius != 0.0) lens_jitter(P, s, p, gpix, j);
                primary_ray(P.cam, qwl, qhl, xl, yl, j, r.o, r.d);
            } else {
                if (P.cam.lens_radius != 0.0) lens_jitter(P, s, p, gpix, j);
                if (s + 1 < s_stop) primary_jitter(P, s + 1, p, gpix, jn);
                primary_ray(P.cam, qw, qh, xc, yr, j, r.o, r.d);
            }
            RT_ACC(0, tr0);
            int32_t* hs = P.hit_out ? P.hit_out + (int64_t)s * P.npix + p : nullptr;
            RT_T0(tt0);
            if (!FUSE) {
                trace_one<MATS>(P, r, true, err, hs, GpuEmit{P, r, shard, 0u, &shadow, &acc});
            } else {
                // the sample's whole path in this thread (single-child scenes): no queue, every
                // depth's colour into `acc`; the lanes of an iteration share a depth, counted per
                // wave into the shard's counter of that depth as the queue appends would have been
                // (the child is written over r: shading reads nothing of the ray after it)
                // (one loop over the depths, depth 0 included: one inlined copy of the shaders)
                bool live = true;
                if (LANE_STATS) lane_count(P.lane_stats, __ballot(true));  // (srt_debug_lane_stats: depth 0)
                for (int d = 0;; ++d) {
                    bool has = false;
                    trace_one<MATS>(P, r, live, err, d == 0 ? hs : nullptr, FusedEmit{P, r, 0u, &shadow, &acc, &r, &has});
                    live = live && has;
                    const uint64_t m = __ballot(live);
                    if (m == 0) break;
                    if (live && lanes_below(m) == 0 && d + 1 < SRT_MAX_DEPTHS) {  // the lowest live lane
                        atomicAdd(P.cnt_out + (int64_t)d * NSHARD + shard, (uint32_t)__builtin_popcountll(m));
                        if (LANE_STATS) lane_count(P.lane_stats + 2 * (d + 1), m);
                    }
                    if (d + 1 > P.dcap) break;  // counted (the host reports rays beyond the cap), not traced
                }
            }
            RT_ACC(3, tt0);
        }
        // the pixel's sample groups (lanes of this wave) summed; lane of group 0 stores the pixel
        PixAcc& acc_r = acc;
        acc_r.reduce_lanes(fx, ppw);
        const bool owner = pact && grp == 0;
        if (FUSE && P.fuse_resolve) {
            // the frame's only pass: the pixel is complete (scene.py:118-140, k_resolve's rule)
            uint8_t px[3] = {0, 0, 0};
            if (owner) {
                if (fx && acc_r.suspect()) atomicOr(&P.flags[1], RETRY_FIXED_RANGE);
                const double spp = (double)P.spp_total;
                const double rr = acc_r.value(fx, 0) / spp, gg = acc_r.value(fx, 1) / spp, bb = acc_r.value(fx, 2) / spp;
                double a0, a1, a2;
                resolve_pixel(rr, gg, bb, a0, a1, a2, px);
                if (P.out_rgb) {
                    P.out_rgb[p] = rr;
                    P.out_rgb[P.npix + p] = gg;
                    P.out_rgb[2 * P.npix + p] = bb;
                }
            }
            if (P.out_u8) {
                if (TILE) {
                    const uint32_t ty = (uint32_t)wv / tiles_x, tx = (uint32_t)wv - ty * tiles_x;
                    store_u8_tile(P.out_u8, px, lane, 8, (int)th, (int64_t)(ty * th), (int64_t)(tx * 8u), (int64_t)Wc,
                                  (int64_t)nrows);
                } else
                    store_u8_chunk(P.out_u8 + 3 * p0, px, lane, (int)min<int64_t>(ppw, P.npix - p0));
            }
        } else if (owner && fx) {
            // the frame's fixed-point sums (k_trace adds the deeper depths of the per-depth path);
            // no other thread of this launch touches the pixel
            float* mg = fx_mag(P.fbx, P.npix) + p;
            if (P.fb_first) {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.fbx[k * P.npix + p] = acc_r.w[k];
                *mg = acc_r.mag;
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.fbx[k * P.npix + p] += acc_r.w[k];
                *mg += acc_r.mag;
            }
        } else if (owner) {
            if (P.fb_first) {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.fb[k * P.npix + p] = acc_r.value(false, k);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) P.fb[k * P.npix + p] += acc_r.value(false, k);
            }
        }
    }
    if (err) atomicOr(&P.flags[0], err);
    if (shadow) atomicAdd(P.shadow, (unsigned long long)shadow);
