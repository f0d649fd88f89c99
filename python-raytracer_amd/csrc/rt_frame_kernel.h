// rt_frame_kernel.h -- the frame kernel, the third trace path: FRAME_BLOCK, the wave's LDS block FrameLds
// with lds_get / lds_put, the per-variant choices frame_tile_for / frame_split_for / frame_lifo_for,
// frame_tile_index, frame_tiles (host), the ring emitters FrameEmit and FrameEmitFx, and k_frame.
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: rt_trace_common.h and
// rt_trace_kernels.h (trace_one, stage_luts, store_u8_chunk, store_u8_tile).
namespace {

// ---- the frame kernel ----------------------------------------------------------------------
// One wave (a 64-thread block) owns a tile of 64 consecutive pixels and traces their whole ray
// trees: it generates the tile's primary rays sample by sample, appends every child to a private
// ring in HBM and drains the ring in FIFO order, taking a full 64-ray chunk whenever one is
// pending and new primaries otherwise.  Colours go to per-pixel accumulators in LDS; at the end
// the wave writes (or resolves) its 64 pixels.  No atomics between waves, no per-depth launches:
// the depth tails of different tiles overlap on the GPU instead of serialising kernel after
// kernel, and all samples of a pixel are queued together, which keeps lanes ~95 % busy
// (simulated on the ex1 1080p path-length distribution: 94.6 % with pure chunks).
constexpr int FRAME_BLOCK = 64;

struct FrameLds {
    double acc[3][FRAME_BLOCK];  // per-pixel colour sums of the tile
    uint32_t depth_cnt[SRT_MAX_DEPTHS];
    uint32_t head, tail;         // ring positions (wave-uniform; kept in LDS so that updates made
                                 // under divergent control flow are seen by every lane)
    uint32_t head1, tail1;       // (FRAME_SPLIT) the second ring's: rays travelling inside a medium
    uint32_t slot;
    uint32_t overflow;
};

// The ring positions are shared by the wave's lanes through LDS.  Plain loads/stores would let the
// compiler forward a lane's own earlier value past another lane's update (a data race under the
// single-thread model), so every access is an atomic at workgroup scope and the reserving lane's
// result is broadcast with a cross-lane read.
__device__ __forceinline__ uint32_t lds_get(uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_put(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// k_frame's tile: 8 x 8 pixels of the pass or 64 consecutive ones of a row; the tile's first pixel is
// tile0, and the LDS accumulator of pixel tile0 + d is the lane that owns it.  A square tile's rays
// stay coherent deeper (fewer chunks mix colliders): same box, ex3 1080p d8 frame 2.755 -> 2.605 ms,
// cornell 800x800 512 spp 4006 -> 3939 ms, but the thin-film example4 4K 13.95 -> 14.09 ms, so the
// thin-film variants keep rows (profiles/r06_frame_tile_ab.txt).
constexpr bool frame_tile_for(uint32_t mats) { return (mats & mat_bit(SRT_THINFILM)) == 0; }
// k_frame's ring split in two halves for the refractive variants without thin films or Diffuse: rays
// travelling inside a medium (which next hit the body they are in) in one, the rest in the other, so
// that a chunk of the first shades one collider in one pass of the material waterfall: ex3 1080p d8
// frame 2.647 -> 2.552 ms, k_frame 2.86 -> 2.65 ms; the thin-film example4 4K 13.53 -> 14.04 ms, and
// cornell's Diffuse fan-out overflows half a ring (profiles/r06_frame_split_ab.txt)
constexpr bool frame_split_for(uint32_t mats) {
    return (mats & mat_bit(SRT_REFRACTIVE)) != 0 && (mats & (mat_bit(SRT_THINFILM) | mat_bit(SRT_DIFFUSE))) == 0;
}
// k_frame's rings drained newest first (a stack: the chunk taken is the last 64 rays pushed, usually
// the children of the chunk just traced, still in L2) for the thin-film variants (ex4 4K frame 13.83 ->
// 13.58 ms) and the split-ring ones (ex3 1080p d8, same box: frame 2.55-2.58 -> 2.45-2.47 ms,
// device-resident 2.41-2.43 -> 2.14-2.18 ms, profiles/r06_frame_split_lifo_ab.txt; before the split,
// one FIFO-or-stack ring gave ex3 no change); oldest first for the rest (cornell's Diffuse fan-out
// outgrows a stack's ring: 4.02 -> 5.24 s; profiles/r06_rejected_frame_lifo.txt)
constexpr bool frame_lifo_for(uint32_t mats) {
    return (mats & mat_bit(SRT_THINFILM)) != 0 || frame_split_for(mats);
}
__device__ __forceinline__ uint32_t frame_tile_index(bool tiled, uint32_t d, uint32_t W) {
    if (!tiled) return d;
    const uint32_t ly = d / W;
    return ly * 8u + (d - ly * W);
}
inline int64_t frame_tiles(bool tiled, int64_t W, int64_t nrows) {
    return tiled ? ((W + 7) / 8) * ((nrows + 7) / 8) : (W * nrows + FRAME_BLOCK - 1) / FRAME_BLOCK;
}

struct FrameEmit {
    const TraceParams& P;
    const Ray& r;
    uint32_t round;
    uint32_t* shadow_acc;
    FrameLds* L;
    uint32_t tile0;
    int64_t ring_base;
    bool tiled;  // (k_frame's FRAME_TILE)
    bool split;  // (k_frame's FRAME_SPLIT) rays inside a medium (child medium != 0) go to ring 1

    __device__ void local(d3 c) const {
        if (is_zero(c)) return;
        const uint32_t k = frame_tile_index(tiled, r.pix - tile0, (uint32_t)P.cam.width);
        __hip_atomic_fetch_add(&L->acc[0][k], r.w.x * c.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&L->acc[1][k], r.w.y * c.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&L->acc[2][k], r.w.z * c.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ void shadow(int n) const { *shadow_acc += (uint32_t)n; }
    // `cnt` consecutive ring positions for every active lane (wave-local: LDS counter, no atomics)
    __device__ uint32_t reserve(uint32_t cnt) const {
        uint32_t total = 0, below = 0;
        for (int b = 0; b < 8; ++b) {
            uint64_t m = __ballot((cnt >> b) & 1u);
            total += (uint32_t)__builtin_popcountll(m) << b;
            below += lanes_below(m) << b;
        }
        const uint64_t act = __ballot(1);
        const int leader = __builtin_ctzll(act);
        uint32_t base = 0;
        if (lanes_below(act) == 0)
            base = __hip_atomic_fetch_add(&L->tail, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        base = (uint32_t)__shfl((int)base, leader);
        return base + below;
    }
    // ring q (split: half the slot each) at its position pos
    __device__ void store(uint32_t pos, const Child& c, uint32_t path, int q = 0) const {
        const uint32_t depth = meta_depth(r.meta) + 1;
        const uint32_t cap = split ? (uint32_t)P.ring_cap >> 1 : (uint32_t)P.ring_cap;
        if (pos - lds_get(q ? &L->head1 : &L->head) >= cap) {  // ring full: the frame is re-rendered with bigger rings
            lds_put(&L->overflow, 1u);
            return;
        }
        queue_store(P.ring, ring_base + (int64_t)(q ? cap : 0u) + (int64_t)(pos & (cap - 1u)), c.o, c.d, mul(r.w, c.w),
                    r.pix, pack_meta(c.medium, depth, c.dfl), path);
    }
    __device__ void child(const Child& c) const {
        if (!split) {
            store(reserve(1u), c, child_path(r.path, c.slot, round));
            return;
        }
        // a ray inside a medium (a refractive body: it next hits that body from inside) to ring 1, the
        // rest to ring 0, so that chunks of ring 1 shade one collider in one waterfall pass
        const bool in = c.medium != 0u;
        const uint64_t m1 = __ballot(in), m0 = __ballot(!in), act = __ballot(1);
        const int leader = __builtin_ctzll(act);
        uint32_t b0 = 0, b1 = 0;
        if (lanes_below(act) == 0) {
            if (m0) b0 = __hip_atomic_fetch_add(&L->tail, (uint32_t)__builtin_popcountll(m0), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
            if (m1) b1 = __hip_atomic_fetch_add(&L->tail1, (uint32_t)__builtin_popcountll(m1), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        b0 = (uint32_t)__shfl((int)b0, leader);
        b1 = (uint32_t)__shfl((int)b1, leader);
        store(in ? b1 + lanes_below(m1) : b0 + lanes_below(m0), c, child_path(r.path, c.slot, round), in ? 1 : 0);
    }
    // the fan-out child-major in the ring (as GpuEmit::diffuse): the k-th children of the lanes are
    // consecutive, every store a coalesced run.  Lane-major positions scattered each store over 64
    // cache lines and doubled the ring's HBM writes (cornell k_frame: 309 GB written per pass for
    // 143 GB of rays, PMC WRITE_SIZE)
    __device__ void diffuse(const DiffuseGen& g, int mi) const {
        const uint32_t cnt = (uint32_t)g.count;
        const uint32_t base = reserve(cnt) - wave_below(cnt);
        const auto& m = P.S.mat[mi];
        uint32_t off = 0;
        for (uint32_t k = 0;; ++k) {
            const uint64_t mk = __ballot(cnt > k);
            if (!mk) break;
            if (cnt > k) {
                Rng rng;
                const uint32_t cpath = child_path(r.path, 0x100u + k, round);
                rng.init(P.seed, key_pix(P, r.pix), cpath, 0xD1000000u | meta_depth(r.meta));
                store(base + off + lanes_below(mk), diffuse_child(P.S, m, g, rng, k), cpath);
            }
            off += (uint32_t)__builtin_popcountll(mk);
        }
    }
};

// FrameEmit for the k_frame variants that sum in fixed point when the frame does (P.fbx set; the
// MAT_VATTR variants): the tile's sums are integers in acc's words
struct FrameEmitFx : FrameEmit {
    __device__ void local(d3 c) const {
        if (!P.fbx) return FrameEmit::local(c);
        if (is_zero(c)) return;
        const uint32_t k = frame_tile_index(tiled, r.pix - tile0, (uint32_t)P.cam.width);
        // fb_add's terms: each rounded to a multiple of 2^-FX_BITS and added as an integer, so the
        // tile's totals do not depend on the ring's order and equal the per-depth kernels' bit for
        // bit.  A term of magnitude >= 2^17 (or NaN) is left out, and a partial sum of magnitude >= 2^61
        // scaled (2^17 in colour units) is distrusted: every term is below 2^61 scaled, so no sum wraps
        // without landing there first.  Either renders the frame again in f64 (as does a total the
        // resolve of the other paths would distrust, fx_suspect: k_frame's end).
        const d3 t = mul(r.w, c);
        bool ok = ((fabs(t.x) + fabs(t.y)) + fabs(t.z)) < FX_MAX;
        if (ok) {
            const double tv[3] = {t.x, t.y, t.z};
            for (int ch = 0; ch < 3; ++ch) {
                const unsigned long long add = (unsigned long long)__double2ll_rn(tv[ch] * FX_SCALE);
                const unsigned long long old = __hip_atomic_fetch_add(
                    reinterpret_cast<unsigned long long*>(&L->acc[ch][k]), add, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_WORKGROUP);
                const long long sum = (long long)(old + add);
                ok &= sum < (1ll << 61) && sum >= -(1ll << 61);
            }
        }
        if (!ok) atomicOr(&P.flags[1], RETRY_FIXED_RANGE);
    }
};

template <uint32_t MATS, int OCC = 2>
__global__ __launch_bounds__(FRAME_BLOCK, OCC) void k_frame(TraceParams P0) {
    constexpr bool FRAME_TILE = frame_tile_for(MATS), FRAME_LIFO = frame_lifo_for(MATS);
    constexpr bool FRAME_SPLIT = frame_split_for(MATS);
    // The variants for per-vertex attributes sum a tile's colours as the per-depth kernels do, in fixed
    // point (FrameEmitFx::local), when the frame does (P.fbx set): their frames are then the per-depth
    // kernels' bit for bit.  The other variants keep their float64 sums in the ring's order.
    constexpr bool FRAME_FX_VARIANT = (MATS & MAT_VATTR) != 0;
    const TraceParams& P = P0;
    const bool frame_fx = FRAME_FX_VARIANT && P0.fbx != nullptr;
    {
        const int nl = P.S.nlut_lds;
        for (int i = threadIdx.x; i < nl * 256; i += FRAME_BLOCK) rt_lds_dyn[i] = P.S.tex[i >> 8].lut[i & 255];
    }
    __shared__ FrameLds L;
    RT_T0(tf0);
    const uint32_t lane = threadIdx.x;
    for (int k = 0; k < 3; ++k) L.acc[k][lane] = 0.0;
    for (int d = lane; d < SRT_MAX_DEPTHS; d += FRAME_BLOCK) L.depth_cnt[d] = 0u;
    if (lane == 0) {
        // a free ring: slots are tried from blockIdx on; there are twice as many as resident waves
        uint32_t s = blockIdx.x % (uint32_t)P.nslot;
        while (atomicCAS(&P.ring_lock[s], 0u, 1u) != 0u) s = (s + 1u) % (uint32_t)P.nslot;
        L.slot = s;
        L.head = 0u;
        L.tail = 0u;
        L.head1 = 0u;
        L.tail1 = 0u;
        L.overflow = 0u;
    }
    __syncthreads();
    RT_ACC(18, tf0);
    const uint32_t tile = blockIdx.x % (uint32_t)P.ntiles, grp = blockIdx.x / (uint32_t)P.ntiles;
    const uint32_t Wc = (uint32_t)P.cam.width, nrows = (uint32_t)(P.npix / P.cam.width);
    const uint32_t tiles_x = (Wc + 7u) >> 3, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const uint32_t tile0 = FRAME_TILE ? (ty * 8u) * Wc + tx * 8u : tile * FRAME_BLOCK;
    const int spg = (P.spp + P.groups - 1) / P.groups;
    const int s_end = min(P.spp, (int)(grp + 1) * spg);
    const int64_t ring_base = (int64_t)L.slot * P.ring_cap;
    const uint32_t shard = blockIdx.x % NSHARD;
    uint32_t err = 0;
    uint32_t shadow = 0;
    // this lane's pixel of the tile
    uint32_t p, lr, col;
    bool pact;
    if (FRAME_TILE) {
        const uint32_t r = ty * 8u + (lane >> 3), cx = tx * 8u + (lane & 7u);
        pact = r < nrows && cx < Wc;
        lr = pact ? r : 0u;
        col = pact ? cx : 0u;
        p = pact ? lr * Wc + col : tile0;
    } else {
        p = tile0 + lane;
        pact = p < (uint32_t)P.npix;
        lr = pact ? p / (uint32_t)P.cam.width : 0u;
        col = pact ? p - lr * (uint32_t)P.cam.width : 0u;
    }
    const int grow = pact ? P.rows[lr] : 0;
    const double xc = pact ? P.cam.xs[col] : 0.0, yr = pact ? P.cam.ys[grow] : 0.0;
    const uint32_t gpix = (uint32_t)grow * (uint32_t)P.cam.width + col;
    const Quot qw((double)P.cam.width), qh((double)P.cam.height);
    int s_next = (int)grp * spg;
    const uint32_t rcap = FRAME_SPLIT ? (uint32_t)P.ring_cap >> 1 : (uint32_t)P.ring_cap;  // rays per ring
    for (;;) {
        const uint32_t head0 = lds_get(&L.head), tail0 = lds_get(&L.tail);
        const uint32_t head1 = FRAME_SPLIT ? lds_get(&L.head1) : 0u, tail1 = FRAME_SPLIT ? lds_get(&L.tail1) : 0u;
        const uint32_t pend0 = tail0 - head0, pend1 = tail1 - head1;
        if (pend0 == 0u && pend1 == 0u && s_next >= s_end) break;
        // a ring overflowed: the frame is re-rendered with bigger rings, and the positions past the
        // overflow hold no rays of this launch
        if (lds_get(&L.overflow)) break;
        // the ring a chunk comes from: the fuller of two full chunks (ring 1 on a tie), else the one
        // holding a full chunk, else (primaries done) ring 1 then ring 0
        const int q = pend1 >= (uint32_t)FRAME_BLOCK ? (pend1 >= pend0 ? 1 : 0)
                                                     : (pend0 < (uint32_t)FRAME_BLOCK && pend1 > 0u ? 1 : 0);
        const uint32_t head = q ? head1 : head0, tail = q ? tail1 : tail0, pending = q ? pend1 : pend0;
        Ray r;
        bool active;
        uint32_t depth = 0;
        int32_t* hs = nullptr;
        if (pending >= (uint32_t)FRAME_BLOCK || s_next >= s_end) {
            // a chunk of the ring: its oldest rays, or (FRAME_LIFO) its newest, whose children are then
            // pushed over them (their stores follow every lane's loads: the loaded rays are read first)
            const uint32_t take = min(pending, (uint32_t)FRAME_BLOCK);
            active = lane < take;
            RT_T0(tl0);
            const uint32_t first = FRAME_LIFO ? tail - take : head;
            if (active) {
                r = queue_load(P.ring, ring_base + (int64_t)(q ? rcap : 0u) + (int64_t)((first + lane) & (rcap - 1u)));
                depth = meta_depth(r.meta);
            } else {
                r.o = r.d = r.w = d3{0.0, 0.0, 0.0};
                r.pix = tile0; r.meta = 0; r.path = 0;
            }
            if (lane == 0) {
                if (FRAME_LIFO)
                    lds_put(q ? &L.tail1 : &L.tail, first);
                else
                    lds_put(q ? &L.head1 : &L.head, head + take);
            }
            RT_ACC(16, tl0);
        } else {
            // primary rays of sample s_next for the tile's pixels (camera.py:51-85)
            const int s = s_next++;
            active = pact;
            r.o = r.d = d3{0.0, 0.0, 0.0};
            r.w = d3{1.0, 1.0, 1.0};
            r.meta = pack_meta(0, 0, 0);
            r.pix = pact ? p : tile0;
            r.path = mix32(0x5EED0000u, (uint32_t)(P.sample_base + s));
            RT_T0(tg0);
            if (active) {
                double j[4] = {0.0, 0.0, 0.0, 0.0};
                primary_uniforms(P, s, p, gpix, j);
                primary_ray(P.cam, qw, qh, xc, yr, j, r.o, r.d);
            }
            RT_ACC(15, tg0);
            if (P.hit_out && active) hs = P.hit_out + (int64_t)s * P.npix + p;
        }
        // rays entering each depth; a ray beyond the depth cap is counted (the host reports it as an
        // error) and dropped, so every ring drains
        if (active) {
            __hip_atomic_fetch_add(&L.depth_cnt[min(depth, (uint32_t)SRT_MAX_DEPTHS - 1u)], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
            if ((int)depth > P.dcap) active = false;
        }
        RT_T0(tt2);
        if constexpr (FRAME_FX_VARIANT)
            trace_one<MATS>(P, r, active, err, hs,
                            FrameEmitFx{{P, r, 0u, &shadow, &L, tile0, ring_base, FRAME_TILE, FRAME_SPLIT}});
        else
            trace_one<MATS>(P, r, active, err, hs, FrameEmit{P, r, 0u, &shadow, &L, tile0, ring_base, FRAME_TILE, FRAME_SPLIT});
        RT_ACC(17, tt2);
    }
    RT_T0(te0);
    // tile pixels out (fixed-point sums: sum 2^-FX_BITS, fx_value's conversion)
    if (frame_fx) {
        __syncthreads();
        bool bad = false;
        for (int k = 0; k < 3; ++k) {
            const unsigned long long w = *reinterpret_cast<unsigned long long*>(&L.acc[k][lane]);
            bad |= (w >> 61) != 0;
            L.acc[k][lane] = (double)(long long)w * FX_UNIT;
        }
        if (bad) atomicOr(&P.flags[1], RETRY_FIXED_RANGE);
    }
    if (P.fuse_resolve) {
        uint8_t px[3] = {0, 0, 0};
        if (pact) {
            const double spp = (double)P.spp_total;
            double rr = L.acc[0][lane] / spp, gg = L.acc[1][lane] / spp, bb = L.acc[2][lane] / spp;
            double a0, a1, a2;
            resolve_pixel(rr, gg, bb, a0, a1, a2, px);
            if (P.out_rgb) { P.out_rgb[p] = rr; P.out_rgb[P.npix + p] = gg; P.out_rgb[2 * P.npix + p] = bb; }
        }
        if (P.out_u8) {
            if (FRAME_TILE) {
                store_u8_tile(P.out_u8, px, lane, 8, 8, (int64_t)(ty * 8u), (int64_t)(tx * 8u), (int64_t)Wc, (int64_t)nrows);
            } else {
                const int64_t p0 = p - lane;
                store_u8_chunk(P.out_u8 + 3 * p0, px, lane, (int)min<int64_t>(64, P.npix - p0));
            }
        }
    } else if (pact && P.groups > 1) {
        double* part = P.fbg + (int64_t)grp * 3 * P.npix;
        part[p] = L.acc[0][lane]; part[P.npix + p] = L.acc[1][lane]; part[2 * P.npix + p] = L.acc[2][lane];
    } else if (pact) {
        const double ar = L.acc[0][lane], ag = L.acc[1][lane], ab = L.acc[2][lane];
        if (P.fb_first) {
            P.fb[p] = ar; P.fb[P.npix + p] = ag; P.fb[2 * P.npix + p] = ab;
        } else {
            P.fb[p] += ar; P.fb[P.npix + p] += ag; P.fb[2 * P.npix + p] += ab;
        }
    }
    __syncthreads();
    for (int d = lane; d <= P.dcap + 1 && d < SRT_MAX_DEPTHS; d += FRAME_BLOCK)
        if (L.depth_cnt[d]) atomicAdd(P.cnt_out + (int64_t)d * NSHARD + shard, L.depth_cnt[d]);
    if (err) atomicOr(&P.flags[0], err);
    if (lane == 0 && lds_get(&L.overflow)) atomicOr(&P.flags[1], RETRY_OVERFLOW);
    // the wave's shadow-ray count into its shard's counter
    for (int off = 32; off > 0; off >>= 1) shadow += __shfl_xor(shadow, off);
    if (lane == 0) {
        if (shadow) atomicAdd(P.shadow + shard, (unsigned long long)shadow);
        __threadfence();
        atomicExch(&P.ring_lock[L.slot], 0u);
    }
    RT_ACC(19, te0);
}

}  // namespace
