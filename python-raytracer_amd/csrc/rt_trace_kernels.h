// rt_trace_kernels.h -- the trace step and the kernels of the per-depth and the fused paths: trace_one (the
// nearest hit, then the shading waterfall over the colliders hit in the wave), the single-child emitters
// ChainEmit and FusedEmit, lane_count, stage_luts, the uint8 stores store_u8_chunk / store_u8_tile,
// k_primary and k_primary_lean (the body of both is rt_primary_body.inc), k_trace, and the shading of the
// caller's hits for srt_shade* (shade_forced_body, k_shade_forced, k_shade_forced_inputs).
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: rt_trace_common.h
// (TraceParams, HitPtrs, the queue, fb_add, PixAcc, GpuEmit, the primary uniforms) and what precedes that.
namespace {

// One trace step for one ray (all lanes of the wave call it; `active` masks the tail).
// MATS: material types compiled into this instantiation (the host picks one covering the scene).
// Em: the emitter (GpuEmit: wavefront queues; FrameEmit: the frame kernel's per-wave ring); `em0`
// is round 0's, tied colliders get copies with rounds 1, 2, ...
template <uint32_t MATS, class Em, bool FORCED = false>
__device__ __forceinline__ void trace_one(const TraceParams& P, Ray& r, bool active, uint32_t& err, int32_t* hit_slot,
                                          const Em& em0, const HitPtrs* hp = nullptr) {
    const SceneView& S = P.S;
    double t = FARAWAY, o = FARAWAY;
    bool ties = false;
    int id = -1;
    RT_T0(tn0);
    if (FORCED) {  // the caller's hit (Material.get_color): that collider only, no tie loop
        if (active) {
            id = P.force_id[r.pix];
            t = P.force_t[r.pix];
            o = P.force_o[r.pix];
            if (id < -1 || id >= (int32_t)S.ncol) {  // not a collider of the scene (IndexError)
                err |= ERR_INDEX;
                id = -1;
            }
        }
    } else if (active) {
        id = nearest_hit<MATS>(S, r.o, r.d, t, o, ties);
    }
    if constexpr (em_in_place<Em>::value) {
        // the emitter writes the child over `r` (the fused path): no tie loop, which would read the
        // ray after shading; a tie renders the frame again without the fused path
        if (ties) atomicOr(&P.flags[1], RETRY_CHAIN_TIE);
        ties = false;
    }
    RT_ACC(1, tn0);
    if (hit_slot && active) *hit_slot = id;
#ifdef RT_ABL_NOSHADE  // diagnostic build only: raygen + nearest hit, no shading
    if (id == 12345) em0.local(d3{t, o, 0.0});
    return;
#endif
    // waterfall over the colliders hit in this wave: inside each pass the collider index, and so
    // its material and every table entry they reference, is wave-uniform (scalar loads into SGPRs,
    // uniform branches); a wave usually sees one to three distinct colliders
    // Exact ties (ray.py:131-146: every collider at the nearest distance is shaded and the colours
    // added) go through the same waterfall: after shading its collider a tied lane moves on to the
    // next collider (in index order) hit at the same distance, with the next emission round.  One
    // copy of the shaders per kernel (a separate tie loop held a second one: the kernels waited on
    // ~10 % of their wave cycles in SQ_WAIT_INST_ANY; round 6: issue stalls, the i-cache misses 0.004 %).
    RT_T0(tw0);
    // srt_shade_level_inputs: the per-hit inputs of this ray
    [[maybe_unused]] HitIn hin{};
    const HitIn* hi = nullptr;
    if constexpr (FORCED && (MATS & MAT_HITIN) != 0) {
        hin = HitIn{hp->albedo, hp->ldist, hp->lirr, P.npix, (int64_t)r.pix};
        hi = &hin;
    }
    // a SkyBox / Panorama hit without a tie: its texel words fetched now, its colour added after the
    // waterfall of the other colliders (the load latency overlaps their shading; fixed-point sums do
    // not depend on the order of the terms)
    bool sky_pre = false;
    uint32_t sky_w0 = 0u, sky_w1 = 0u;
    if constexpr (!FORCED && (MATS & mat_bit(SRT_SKY)) != 0) {
        sky_pre = S.sky_col >= 0 && id == S.sky_col && !ties;
        if (sky_pre) sky_fetch(S, r, t, sky_w0, sky_w1, err);
    }
    int cur = sky_pre ? -1 : id;  // collider this lane shades next (-1: done)
    double co = o;    // its orientation
    uint32_t rnd = 0;  // emission round: 0 the nearest collider, k the k-th tied one
    uint64_t pending = __ballot(cur >= 0);
    while (pending) {
        RT_ACC(12, tw0);  // counts waterfall passes (k = 12 calls)
        const int lead = __builtin_ctzll(pending);
        const int cu = __builtin_amdgcn_readfirstlane(__shfl(cur, lead));
        const bool mine = (cur == cu);
        if (mine) {
            // re-derive the uniform index inside the branch: here cur == cu on every active lane, and
            // the compiler would otherwise substitute the per-lane id back into every table
            // address (vector loads into VGPRs instead of scalar loads)
            const int cs = __builtin_amdgcn_readfirstlane(cur);
            const auto& c = S.col[cs];
            const int m = c.material;
            Em em = em0;
            if (rnd) em.round = rnd;
            switch (S.mat[m].type) {
                case SRT_GLOSSY:
                    if (MATS & mat_bit(SRT_GLOSSY)) shade_glossy<MATS>(S, c, m, r, t, co, em, err, hi);
                    break;
                case SRT_REFRACTIVE:
                    if (MATS & mat_bit(SRT_REFRACTIVE))
                        shade_refractive<MATS>(S, c, m, r, t, co, em, err, mc_uniform(P, r, cs, rnd));
                    break;
                case SRT_THINFILM:
                    if (MATS & mat_bit(SRT_THINFILM)) shade_thinfilm<MATS>(S, c, m, r, t, co, em, err);
                    break;
                case SRT_DIFFUSE:
                    if (MATS & mat_bit(SRT_DIFFUSE)) shade_diffuse<MATS>(S, c, m, r, t, co, em, err, hi);
                    break;
                case SRT_EMISSIVE:
                    if (MATS & mat_bit(SRT_EMISSIVE)) shade_emissive<MATS>(S, c, m, r, t, em, err, hi);
                    break;
                default:
                    if (MATS & mat_bit(SRT_SKY)) shade_sky(S, c, m, r, t, em, err);
                    break;
            }
        }
        if (!FORCED && __ballot(mine && ties)) {
            // the lanes just shaded find their next tied collider: a wave-uniform collider loop
            // (scalar table loads) from cu + 1
            int nxt = -1;
            double no = FARAWAY;
            for (int c = cu + 1; c < S.ncol; ++c) {
                double oc;
                if (mine && ties && nxt < 0 && collider_hit<MATS>(S.col[c], r.o, r.d, oc) == t) {
                    nxt = c;
                    no = oc;
                }
            }
            if (mine) {
                cur = nxt;
                co = no;
                ++rnd;
            }
        } else if (mine) {
            cur = -1;
        }
        pending = __ballot(cur >= 0);
    }
    if (sky_pre) em0.local(sky_color(S, r, sky_w0, sky_w1));
    RT_ACC(2, tw0);
}

// Chain mode emitter (scenes whose rays have at most one child): the child replaces the ray in the
// thread instead of going to the next depth's queue.  A second child (two colliders tied at the
// same distance) has no place: it raises the retry flag and the host renders the frame again
// without chain mode.
struct ChainEmit {
    const TraceParams& P;
    const Ray& r;
    uint32_t round;
    uint32_t* shadow_acc;
    Ray* next;
    bool* has;

    __device__ void local(d3 c) const { fb_add(P.fb, P.fbx, P.flags, P.npix, r.pix, r.w, c); }
    __device__ void shadow(int n) const { *shadow_acc += (uint32_t)n; }
    __device__ void put(const Child& c, uint32_t path) const {
        if (*has) {
            atomicOr(&P.flags[1], RETRY_CHAIN_TIE);
            return;
        }
        *has = true;
        next->o = c.o;
        next->d = c.d;
        next->w = mul(r.w, c.w);
        next->pix = r.pix;
        next->meta = pack_meta(c.medium, meta_depth(r.meta) + 1, c.dfl);
        next->path = path;
    }
    __device__ void child(const Child& c) const { put(c, child_path(r.path, c.slot, round)); }
    __device__ void diffuse(const DiffuseGen& g, int mi) const {
        const auto& m = P.S.mat[mi];
        for (int k = 0; k < g.count; ++k) {
            Rng rng;
            const uint32_t cpath = child_path(r.path, 0x100u + (uint32_t)k, round);
            rng.init(P.seed, key_pix(P, r.pix), cpath, 0xD1000000u | meta_depth(r.meta));
            put(diffuse_child(P.S, m, g, rng, (uint32_t)k), cpath);
        }
    }
};

// Fused-path emitter (k_primary<.., FUSE>: single-child scenes traced pixel by pixel, every depth
// in the pixel's own thread): the one child replaces the ray.  A second child (an exact tie) raises
// RETRY_CHAIN_TIE as in chain mode.  Every depth's colour goes into the thread's PixAcc: the same
// fixed-point terms the per-depth kernels add (their k_primary keeps depth 0 in a PixAcc, k_trace
// adds the deeper terms with fb_add), so the fused and the per-depth paths give the same image bit
// for bit; in f64 mode the terms are summed in the thread in trace order.
struct FusedEmit {
    static constexpr bool kInPlace = true;  // `next` is the traced ray itself (see trace_one)
    const TraceParams& P;
    const Ray& r;
    uint32_t round;
    uint32_t* shadow_acc;
    PixAcc* acc;
    Ray* next;
    bool* has;

    __device__ void local(d3 c) const {
        if (!is_zero(c)) acc->add(P.fbx != nullptr, mul(r.w, c));
    }
    __device__ void shadow(int n) const { *shadow_acc += (uint32_t)n; }
    __device__ void child(const Child& c) const {
        ChainEmit{P, r, round, shadow_acc, next, has}.child(c);
    }
    __device__ void diffuse(const DiffuseGen& g, int mi) const {
        ChainEmit{P, r, round, shadow_acc, next, has}.diffuse(g, mi);
    }
};

// srt_debug_lane_stats: one wave iteration of a depth with the live lanes m, counted by the lowest
// live lane ([0] iterations, [1] live lanes)
__device__ __forceinline__ void lane_count(unsigned long long* st, uint64_t m) {
    if (lanes_below(m) == 0) {
        atomicAdd(st, 1ull);
        atomicAdd(st + 1, (unsigned long long)__builtin_popcountll(m));
    }
}

// Copy the first `nlut` texture lookup tables into LDS (dynamic shared memory) and point the
// scene view at them: texel -> value becomes an LDS read instead of a dependent global load.
__device__ __forceinline__ void stage_luts(const TraceParams& P) {
    const int n = P.S.nlut_lds;
    for (int i = threadIdx.x; i < n * 256; i += BLOCK) rt_lds_dyn[i] = P.S.tex[i >> 8].lut[i & 255];
    __syncthreads();
}

// The uint8 RGB of n consecutive pixels (lane l < n holds pixel p0 + l; dst = out + 3 p0) as 3n/4
// dword stores instead of 3n byte stores (n a multiple of 4, dst 4-byte aligned); otherwise byte
// stores.  Every lane of the wave must call it (cross-lane reads).
__device__ __forceinline__ void store_u8_chunk(uint8_t* dst, const uint8_t px[3], int lane, int n) {
    const uint32_t v = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    if ((n & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        const int nd = (3 * n) / 4;
        const int w = lane < nd ? lane : nd - 1;
        const int q0 = (4 * w) / 3, r0 = (4 * w) % 3;  // dword w = bytes 4w..4w+3: pixels q0, q0 + 1
        const uint32_t x0 = __shfl(v, q0), x1 = __shfl(v, q0 + 1);
        if (lane < nd) reinterpret_cast<uint32_t*>(dst)[lane] = (x0 >> (8 * r0)) | (x1 << (8 * (3 - r0)));
    } else if (lane < n) {
        dst[3 * lane] = px[0];
        dst[3 * lane + 1] = px[1];
        dst[3 * lane + 2] = px[2];
    }
}

// The uint8 RGB of a tw x th pixel tile (lane l < tw th holds local pixel (row0 + l / tw, col0 + l % tw))
// of a frame of W columns and nrows rows: per tile row of tw = 8 (4) pixels, 6 (3) dword stores when
// the row is whole and dword-aligned, else byte stores.  Every lane of the wave must call it.
__device__ __forceinline__ void store_u8_tile(uint8_t* out, const uint8_t px[3], int lane, int tw, int th,
                                              int64_t row0, int64_t col0, int64_t W, int64_t nrows) {
    const uint32_t v = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
    const int nd = (3 * tw) / 4;  // dwords per tile row
    const int ry = lane / nd, w = lane % nd;
    const int q0 = (4 * w) / 3, r0 = (4 * w) % 3;
    const uint32_t x0 = __shfl(v, ry * tw + q0), x1 = __shfl(v, ry * tw + q0 + 1);
    const int64_t row = row0 + ry;
    uint8_t* dst = out + 3 * (row * W + col0);
    const bool whole = col0 + tw <= W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
    if (ry < th && row < nrows && whole) reinterpret_cast<uint32_t*>(dst)[w] = (x0 >> (8 * r0)) | (x1 << (8 * (3 - r0)));
    // rows that are cut by the frame's edge or unaligned: byte stores by the pixel's own lane
    const int py = lane / tw, pxl = lane % tw;
    const int64_t prow = row0 + py, pcol = col0 + pxl;
    uint8_t* pd = out + 3 * (prow * W + col0);
    const bool pwhole = col0 + tw <= W && (reinterpret_cast<uintptr_t>(pd) & 3) == 0;
    if (lane < tw * th && prow < nrows && pcol < W && !pwhole) {
        pd[3 * pxl] = px[0];
        pd[3 * pxl + 1] = px[1];
        pd[3 * pxl + 2] = px[2];
    }
}

// Depth 0: primary-ray generation (camera.py:51-85) fused with the trace step.  A wave takes
// ppw = 64 / G consecutive pixels of the pass: lane l traces pixel l % ppw through the samples of
// its sample group l / ppw (G = P.pix_groups, a power of two; G > 1 gives a small frame -- one GPU's
// shard of a multi-GPU frame -- enough threads to fill the GPU).  A pixel's colour is summed in the
// thread (PixAcc), its groups combined by lane shuffles, and its lane of group 0 stores the pixel:
// no framebuffer atomics, no memset.  FUSE (single-child scenes): every depth of the sample's path
// is traced in the thread too (no ray queues), and a single-pass frame resolves the pixel here
// (P.fuse_resolve: average, sRGB, uint8; no framebuffer at all).  Otherwise the children are appended
// to the depth-1 queue for k_trace.
template <uint32_t MATS, int OCC = 2, bool FUSE = false>
__global__ __launch_bounds__(BLOCK, OCC) void k_primary(TraceParams P0) {
    constexpr bool LEAN = false, LANE_STATS = false;
#include "rt_primary_body.inc"
}

// The lean form of the fused paths of single-child scenes without a BVH, for pipelined frames (the
// headline's kernel; a synchronous frame has no generation beside it and takes k_primary<.., true>):
// built to 160 VGPRs instead of the 168 of 3 waves/SIMD (amdgpu_num_vgpr counts half the unified
// VGPR+AGPR file on gfx950), so three trace waves leave 32 registers per SIMD -- room for one
// four-wave generator workgroup of the next frames' numpy stream (mt_gen_nt: 256 threads, one wave per
// SIMD) beside them instead of it waiting for a trace wave to end -- and reading the camera coordinates
// and jitter per sample (LEAN), which holds its spills to the 168-VGPR build's.  Same box, ex1 1080p d5
// 6 spp pipelined frames 0.901 -> 0.876 ms; the kernel alone (device-resident frames) 0.752 -> 0.762
// (profiles/r05_lean_primary_ab.txt).
// LANE_STATS: the instantiation srt_debug_lane_stats selects (the counting cost 2 spilled VGPRs as a
// run-time branch in the default kernels).
template <uint32_t MATS, int OCC, bool LANE_STATS = false>
__global__ __launch_bounds__(BLOCK, OCC) __attribute__((amdgpu_num_vgpr(80))) void k_primary_lean(TraceParams P0) {
    constexpr bool FUSE = true, LEAN = true;
#include "rt_primary_body.inc"
}

// Depth d >= 1: blocks b, b + NSHARD, ... drain input shard b % NSHARD and append to output shard
// b % NSHARD.
template <uint32_t MATS, int OCC = 2, bool CHAIN = false>
__global__ __launch_bounds__(BLOCK, OCC) void k_trace(TraceParams P0) {
    const TraceParams& P = P0;
    const uint32_t shard = blockIdx.x % NSHARD;
    const int64_t n = min((int64_t)P.cnt_in[shard], P.seg);
    const int64_t blk = blockIdx.x / NSHARD, nblk = gridDim.x / NSHARD;
    if (blk * BLOCK >= n) return;  // nothing in this block's part of the shard (block-uniform)
    stage_luts(P);
    uint32_t err = 0;
    uint32_t shadow = 0;
    const int64_t off = (int64_t)shard * P.seg;
    for (int64_t base = blk * BLOCK; base < n; base += nblk * BLOCK) {
        const int64_t i = base + threadIdx.x;
        const bool active = i < n;
        Ray r;
        RT_T0(tq0);
        if (active) {
            r = queue_load(P.qin, off + i);
        } else {
            r.o = r.d = r.w = d3{0.0, 0.0, 0.0};
            r.pix = 0; r.meta = 0; r.path = 0;
        }
        RT_ACC(13, tq0);
        RT_T0(tt1);
        if (!CHAIN) {
            trace_one<MATS>(P, r, active, err, nullptr, GpuEmit{P, r, shard, 0u, &shadow, nullptr});
        } else {
            // the rest of each ray's path in this thread: lanes advance one depth per iteration, so
            // the live lanes of an iteration share a depth (counted per wave into the shard's
            // counter of that depth, as the queue appends would have)
            bool live = active;
            int d = P.depth;
            for (;;) {
                Ray nx = r;
                bool has = false;
                trace_one<MATS>(P, r, live, err, nullptr, ChainEmit{P, r, 0u, &shadow, &nx, &has});
                live = live && has;
                r = nx;
                ++d;
                const uint64_t m = __ballot(live);
                if (m == 0) break;
                if (live && lanes_below(m) == 0 && d < SRT_MAX_DEPTHS)  // the lowest live lane
                    atomicAdd(P.cnt_out + (int64_t)(d - P.depth - 1) * NSHARD + shard, (uint32_t)__builtin_popcountll(m));
                if (d > P.dcap) break;  // counted (the host reports rays beyond the cap), not traced
            }
        }
        RT_ACC(14, tt1);
    }
    if (err) atomicOr(&P.flags[0], err);
    if (shadow) atomicAdd(P.shadow, (unsigned long long)shadow);
}

// srt_shade's first depth: each queued ray shaded at the caller's hit (Material.get_color,
// material.py:42-44), its children appended for the ordinary k_trace depths
template <uint32_t MATS>
__device__ __forceinline__ void shade_forced_body(const TraceParams& P, const HitPtrs* hp) {
    const uint32_t shard = blockIdx.x % NSHARD;
    const int64_t n = min((int64_t)P.cnt_in[shard], P.seg);
    const int64_t blk = blockIdx.x / NSHARD, nblk = gridDim.x / NSHARD;
    if (blk * BLOCK >= n) return;
    stage_luts(P);
    uint32_t err = 0;
    uint32_t shadow = 0;
    const int64_t off = (int64_t)shard * P.seg;
    for (int64_t base = blk * BLOCK; base < n; base += nblk * BLOCK) {
        const int64_t i = base + threadIdx.x;
        const bool active = i < n;
        Ray r;
        if (active) {
            r = queue_load(P.qin, off + i);
        } else {
            r.o = r.d = r.w = d3{0.0, 0.0, 0.0};
            r.pix = 0; r.meta = 0; r.path = 0;
        }
        trace_one<MATS, GpuEmit, true>(P, r, active, err, nullptr, GpuEmit{P, r, shard, 0u, &shadow, nullptr}, hp);
    }
    if (err) atomicOr(&P.flags[0], err);
    if (shadow) atomicAdd(P.shadow, (unsigned long long)shadow);
}
template <uint32_t MATS>
__global__ __launch_bounds__(BLOCK) void k_shade_forced(TraceParams P0) {
    shade_forced_body<MATS>(P0, nullptr);
}
// srt_shade_level_inputs' first depth: k_shade_forced with the per-hit shading inputs (MAT_HITIN)
template <uint32_t MATS>
__global__ __launch_bounds__(BLOCK) void k_shade_forced_inputs(TraceParams P0, HitPtrs H) {
    static_assert((MATS & MAT_HITIN) != 0, "the per-hit inputs are read under MAT_HITIN");
    shade_forced_body<MATS>(P0, &H);
}

}  // namespace
