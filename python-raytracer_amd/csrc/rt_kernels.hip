// rt_kernels.hip -- gfx950 ray tracer behind the C ABI of include/sightpy_rt.h: the one translation
// unit of libsightpy_hip.so.  Its first and last parts, and the host side of srt_render, are fragments of
// this unit, included in place (source map, in order):
//   rt_trace_common.h  fail / HIP_TRY, Queue, TraceParams, key_pix, the fixed-point sums, PixAcc, GpuEmit
//   (this file)        the kernels, the variants, DevBuf / DevList, the context, the MT host side, scene upload
//   rt_render.h        render_impl, before srt_render and its siblings; then srt_trace and srt_shade* here
//   rt_api_entry.h     the single-kernel entry points, AOVs and denoise, device memory, srt_mt19937_uniforms
//   rt_api_group.h     communicators, srt_render_group*, allreduce, barrier
//   rt_api_misc.h      host memory, the srt_debug_* hooks, srt_synchronize
//
// The reference (sightpy) recursively evaluates numpy batches: intersect every collider, reduce the
// nearest hit, compact the rays per collider, shade, recurse (ray.py:122-148).  A colour composes
// linearly along the ray tree (colour = local + F * child), so every ray carries the product of the
// weights above it (its throughput) and its contribution is summed into the per-pixel framebuffer,
// in order-independent fixed-point sums by default (f64 atomics otherwise).  A frame takes one of
// three kernel paths (RenderCall::plan_frame in rt_render.h chooses; all three share trace_one):
//
//   per-depth    k_primary generates the primary rays (camera.py:51-85) and traces depth 0; one k_trace
//                launch per deeper depth reads ray queue d in HBM (structure of arrays, sharded append
//                counters) and appends the children to queue d + 1.  In chain mode the k_trace of a
//                thinly populated depth follows each ray's single-child chain to its end.  srt_trace and
//                the shade levels seed the queues from the caller's rays and run this path.
//   fused, lean  single-child scenes: k_primary<.., FUSE> traces a pixel's whole path in its thread, no
//                queue; k_primary_lean is the same body under a register cap for pipelined frames,
//                which leaves room for the next frame's numpy-stream generators beside it.
//   k_frame      scenes whose rays branch (refractive, thin-film, diffuse fan-out): one wave per
//                64-pixel tile traces the whole pass, its children in a per-wave ring in HBM; a
//                single-pass frame resolves its pixels in the kernel.
//
// Scene tables are read through wave-uniform indices (scalar loads) in the collider loop; shading runs
// as a waterfall over the materials present in a wave.  k_resolve (spp average + sRGB + intensity clip
// + uint8, scene.py:118-140) ends a frame that did not resolve itself.  Device memory is owned by
// DevBuf (one allocation with a capacity) and DevList (allocations released together).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_denoise.h"
#include "rt_mt.h"
#include "rt_mt_kernel.h"

using namespace rt;
using namespace rtmt_dev;

#include "rt_trace_common.h"

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

// Kernel variants by the material types they contain; the host picks the first covering the scene.
constexpr uint32_t MATS_GLOSSY_SKY = mat_bit(SRT_GLOSSY) | mat_bit(SRT_SKY);
constexpr uint32_t MATS_DIELECTRIC = MATS_GLOSSY_SKY | mat_bit(SRT_REFRACTIVE) | mat_bit(SRT_EMISSIVE);
constexpr uint32_t MATS_FILM = mat_bit(SRT_THINFILM) | mat_bit(SRT_SKY) | mat_bit(SRT_GLOSSY);
constexpr uint32_t MATS_MC = mat_bit(SRT_DIFFUSE) | mat_bit(SRT_EMISSIVE) | mat_bit(SRT_REFRACTIVE);
struct Variant {
    uint32_t mats;
    void (*primary)(TraceParams);
    void (*trace)(TraceParams);
    void (*frame)(TraceParams);
    void (*chain)(TraceParams);
    void (*fused)(TraceParams) = nullptr;  // k_primary<.., FUSE>: whole single-child paths per pixel
    // k_primary_lean (160 VGPRs): the fused paths of pipelined frames, whose numpy-stream generators
    // then run beside them (mt_gen_launch); synchronous frames take `fused`
    void (*lean)(TraceParams) = nullptr;
    void (*lean_stats)(TraceParams) = nullptr;  // k_primary_lean<.., LANE_STATS> (srt_debug_lane_stats)
};
// The trace kernels are built for RT_OCC = 3 waves/SIMD.  Same-box A/B against 2 waves/SIMD
// (profiles/r03_occ_ab.txt): device-resident ex1 1080p 1.22 -> 1.10 ms, ex3 k_frame 3.36 -> 3.06 ms,
// ex4 4K 14.5 -> 13.2 ms, cornell 4.87 -> 4.05 s, mesh 12.2 -> 10.2 ms.
#ifndef RT_OCC
#define RT_OCC 3
#endif
constexpr int OCC = RT_OCC;  // waves/SIMD the trace kernels are built for (register cap 512 / OCC)
#ifndef RT_FUSE_OCC
#define RT_FUSE_OCC 3  // waves/SIMD of the fused k_primary (168 VGPRs; its spills: DESIGN.md §3)
#endif
#ifndef RT_BVH_LDS_STACK
#define RT_BVH_LDS_STACK 1  // the BVH variants' traversal stacks start in LDS (rt_device.h BvhStack)
#endif
constexpr uint32_t LDS_STK = RT_BVH_LDS_STACK ? MAT_LDS_STACK : 0u, LDS_STK_FRAME = RT_BVH_LDS_STACK ? MAT_LDS_STACK | MAT_LDS_NARROW : 0u;
#ifndef RT_MESH_FUSE_OCC
#define RT_MESH_FUSE_OCC RT_FUSE_OCC  // the glossy BVH variant's fused k_primary
#endif
constexpr uint32_t MATS_MESH = MATS_GLOSSY_SKY | MAT_TRI | MAT_BVH;  // a glossy TriangleMesh in the ex1 setting
constexpr uint32_t MATS_MESH_VATTR = MATS_MESH | MAT_VATTR;                // ... smooth-shaded / textured
constexpr uint32_t MATS_BVH_VATTR = MAT_GENERIC | MAT_BVH | MAT_VATTR;
constexpr uint32_t MATS_GLOSSY_PLIGHT = MATS_GLOSSY_SKY | MAT_PLIGHT;  // positional lights (MAT_PLIGHT)
constexpr uint32_t MATS_GENERIC_PLIGHT = MAT_GENERIC | MAT_PLIGHT;
constexpr uint32_t MATS_BVH_PLIGHT = MAT_GENERIC | MAT_BVH | MAT_PLIGHT;
const Variant VARIANTS[] = {
    {MATS_GLOSSY_SKY, k_primary<MATS_GLOSSY_SKY, OCC>, k_trace<MATS_GLOSSY_SKY, OCC>, k_frame<MATS_GLOSSY_SKY, OCC>, k_trace<MATS_GLOSSY_SKY, OCC, true>,
     k_primary<MATS_GLOSSY_SKY, RT_FUSE_OCC, true>, k_primary_lean<MATS_GLOSSY_SKY, RT_FUSE_OCC>,
     k_primary_lean<MATS_GLOSSY_SKY, RT_FUSE_OCC, true>},
#ifndef RT_EXP_MIN  // (register-usage experiments, tools/resource_usage.py: the headline variants only, a quicker compile)
    {MATS_DIELECTRIC, k_primary<MATS_DIELECTRIC, OCC>, k_trace<MATS_DIELECTRIC, OCC>, k_frame<MATS_DIELECTRIC, OCC>, k_trace<MATS_DIELECTRIC, OCC, true>},
    {MATS_FILM, k_primary<MATS_FILM, OCC>, k_trace<MATS_FILM, OCC>, k_frame<MATS_FILM, OCC>, k_trace<MATS_FILM, OCC, true>},
    {MATS_MC, k_primary<MATS_MC, OCC>, k_trace<MATS_MC, OCC>, k_frame<MATS_MC, OCC>, k_trace<MATS_MC, OCC, true>},
    // a glossy TriangleMesh in the ex1 setting (the mesh bench): the BVH traversal, no other features
    {MATS_MESH, k_primary<MATS_MESH | LDS_STK, OCC>, k_trace<MATS_MESH | LDS_STK, OCC>, k_frame<MATS_MESH | LDS_STK_FRAME, OCC>,
     k_trace<MATS_MESH | LDS_STK, OCC, true>, k_primary<MATS_MESH | LDS_STK, RT_MESH_FUSE_OCC, true>},
    {MAT_GENERIC, k_primary<MAT_GENERIC, OCC>, k_trace<MAT_GENERIC, OCC>, k_frame<MAT_GENERIC, OCC>,
     k_trace<MAT_GENERIC, OCC, true>},
    // scenes with a triangle BVH (TriangleMesh)
    {MAT_GENERIC | MAT_BVH, k_primary<MAT_GENERIC | MAT_BVH | LDS_STK, OCC>, k_trace<MAT_GENERIC | MAT_BVH | LDS_STK, OCC>,
     k_frame<MAT_GENERIC | MAT_BVH | LDS_STK_FRAME, OCC>, k_trace<MAT_GENERIC | MAT_BVH | LDS_STK, OCC, true>},
    // Triangles with per-vertex normals / texture coordinates (MAT_VATTR, set by no scene without them, so
    // these stay behind every variant above): the glossy mesh, the linear triangle loop, the BVH
    {MATS_MESH_VATTR, k_primary<MATS_MESH_VATTR | LDS_STK, OCC>, k_trace<MATS_MESH_VATTR | LDS_STK, OCC>,
     k_frame<MATS_MESH_VATTR | LDS_STK_FRAME, OCC>, k_trace<MATS_MESH_VATTR | LDS_STK, OCC, true>,
     k_primary<MATS_MESH_VATTR | LDS_STK, RT_MESH_FUSE_OCC, true>},
    {MAT_GENERIC | MAT_VATTR, k_primary<MAT_GENERIC | MAT_VATTR, OCC>, k_trace<MAT_GENERIC | MAT_VATTR, OCC>,
     k_frame<MAT_GENERIC | MAT_VATTR, OCC>, k_trace<MAT_GENERIC | MAT_VATTR, OCC, true>},
    {MATS_BVH_VATTR, k_primary<MATS_BVH_VATTR | LDS_STK, OCC>, k_trace<MATS_BVH_VATTR | LDS_STK, OCC>,
     k_frame<MATS_BVH_VATTR | LDS_STK_FRAME, OCC>, k_trace<MATS_BVH_VATTR | LDS_STK, OCC, true>},
    // Scenes with a PositionalLight / SpotLight (MAT_PLIGHT, set by no scene without one, so these stay
    // behind every variant above): Glossy surfaces under the sky box with the fused paths (a lit room
    // on a large frame), then the generic rows with and without the BVH.  No collider-sequence variant
    // carries the bit: such a scene intersects its colliders in the loop.  Nor does a MAT_VATTR one: a
    // scene with both is refused at upload (check_scene_desc; the two rows cost more build time than
    // their share of the kernels).
    {MATS_GLOSSY_PLIGHT, k_primary<MATS_GLOSSY_PLIGHT, OCC>, k_trace<MATS_GLOSSY_PLIGHT, OCC>,
     k_frame<MATS_GLOSSY_PLIGHT, OCC>, k_trace<MATS_GLOSSY_PLIGHT, OCC, true>,
     k_primary<MATS_GLOSSY_PLIGHT, RT_FUSE_OCC, true>},
    {MATS_GENERIC_PLIGHT, k_primary<MATS_GENERIC_PLIGHT, OCC>, k_trace<MATS_GENERIC_PLIGHT, OCC>,
     k_frame<MATS_GENERIC_PLIGHT, OCC>, k_trace<MATS_GENERIC_PLIGHT, OCC, true>},
    {MATS_BVH_PLIGHT, k_primary<MATS_BVH_PLIGHT | LDS_STK, OCC>, k_trace<MATS_BVH_PLIGHT | LDS_STK, OCC>,
     k_frame<MATS_BVH_PLIGHT | LDS_STK_FRAME, OCC>, k_trace<MATS_BVH_PLIGHT | LDS_STK, OCC, true>},
#endif
};
// Variants for scenes of a given collider sequence (rt_device.h seq_of: the colliders intersected in
// straight-line code); a scene runs one when its colliders have exactly these types in this order
// and its materials are covered.
#ifndef RT_NO_SEQ_VARIANTS
#define RT_SEQ_VARIANTS
#endif
#ifdef RT_SEQ_VARIANTS
constexpr uint32_t seq_bits(std::initializer_list<int> t) {
    uint32_t q = (uint32_t)t.size();
    int k = 0;
    for (int v : t) q |= (uint32_t)v << (4 + 2 * k++);
    return q << SEQ_SHIFT;
}
// example1 / the headline: two spheres, a plane, the sky box (same box, ex1 1080p d5 6 spp: device-
// resident frame 0.837 -> 0.750 ms, k_primary 1.05 -> 0.95 ms; profiles/r05_collider_seq_ab.txt)
constexpr uint32_t MATS_SEQ_SSPC = MATS_GLOSSY_SKY | seq_bits({SRT_SPHERE, SRT_SPHERE, SRT_PLANE, SRT_CUBOID});
// the branching scenes of two other BASELINE configs, whose frames run k_frame: example3 (floor, glass
// cuboid, sky box; same box, ex3 1080p d8 frame 2.81 -> 2.73 ms, k_frame 2.94 -> 2.82 ms) and example4
// (thin-film sphere, sky box; 4K frame 14.08 -> 13.96 ms), profiles/r06_collider_seq_frame_ab.txt.  The
// cornell box's eight colliders in sequence were 1.7 % slower (4024 -> 4092 ms), so it keeps the loop.
constexpr uint32_t MATS_SEQ_PCC = MATS_DIELECTRIC | seq_bits({SRT_PLANE, SRT_CUBOID, SRT_CUBOID});
constexpr uint32_t MATS_SEQ_SC = MATS_FILM | seq_bits({SRT_SPHERE, SRT_CUBOID});
#define RT_SEQ_FRAME_VARIANT(M) {M, k_primary<M, OCC>, k_trace<M, OCC>, k_frame<M, OCC>, k_trace<M, OCC, true>}
const Variant SEQ_VARIANTS[] = {
    {MATS_SEQ_SSPC, k_primary<MATS_SEQ_SSPC, OCC>, k_trace<MATS_SEQ_SSPC, OCC>, k_frame<MATS_SEQ_SSPC, OCC>,
     k_trace<MATS_SEQ_SSPC, OCC, true>, k_primary<MATS_SEQ_SSPC, RT_FUSE_OCC, true>, k_primary_lean<MATS_SEQ_SSPC, RT_FUSE_OCC>,
     k_primary_lean<MATS_SEQ_SSPC, RT_FUSE_OCC, true>},
#ifndef RT_EXP_MIN
    RT_SEQ_FRAME_VARIANT(MATS_SEQ_PCC),
    RT_SEQ_FRAME_VARIANT(MATS_SEQ_SC),
#endif
};
#endif
const Variant& pick_variant(uint32_t mats, uint32_t seq = 0) {
#ifdef RT_SEQ_VARIANTS
    if (seq)
        for (const Variant& v : SEQ_VARIANTS)
            if (seq_of(v.mats) == seq && (v.mats & mats) == mats) return v;
#endif
    for (const Variant& v : VARIANTS)
        if ((v.mats & mats) == mats) return v;
    return VARIANTS[sizeof(VARIANTS) / sizeof(VARIANTS[0]) - 1];
}

// End of a pass (one block): hand the per-depth append counters and the error/overflow flags to
// the host through pinned memory and zero them for the next pass (replaces two memsets and two
// copies per pass; the frame's stream needs no host round trip until its end).
__global__ __launch_bounds__(BLOCK) void k_pass_end(uint32_t* counts, int64_t words, uint32_t* flags,
                                                   uint32_t* host, uint32_t* host_flags) {
    for (int64_t i = threadIdx.x; i < words; i += BLOCK) {
        host[i] = counts[i];
        counts[i] = 0u;
    }
    if (threadIdx.x < 2) {
        host_flags[threadIdx.x] |= flags[threadIdx.x];  // accumulated until the host checks them
        flags[threadIdx.x] = 0u;
    }
}

__global__ __launch_bounds__(BLOCK) void k_resolve(const double* fb, const unsigned long long* fbx, int64_t npix,
                                                  unsigned long long* shadow,
                                                  uint32_t* shadow_host, double spp, double* rgb, uint8_t* u8,
                                                  uint32_t* counts, int64_t words, uint32_t* flags, uint32_t* host,
                                                  uint32_t* host_flags) {
    // block 0 also ends the last pass (the work of k_pass_end, one launch less per frame)
    if (blockIdx.x == 0 && words > 0) {
        for (int64_t i = threadIdx.x; i < words; i += BLOCK) {
            host[i] = counts[i];
            counts[i] = 0u;
        }
        if (threadIdx.x < 2) {
            host_flags[threadIdx.x] |= flags[threadIdx.x];
            flags[threadIdx.x] = 0u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        // the frame's shadow-ray count (NSHARD counters) to the host, zeroed for the next frame (no
        // kernel of this frame adds to them any more): wave 0 reads them in parallel and reduces
        // across lanes
        unsigned long long v = 0;
        for (int k = threadIdx.x; k < NSHARD; k += 64) {
            v += shadow[k];
            shadow[k] = 0ull;
        }
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (threadIdx.x == 0) {
            shadow_host[0] = (uint32_t)v;
            shadow_host[1] = (uint32_t)(v >> 32);
        }
    }
    // wave-uniform trip count: each wave takes 64 consecutive pixels per step
    const int lane = threadIdx.x & 63;
    for (int64_t p0 = (int64_t)blockIdx.x * BLOCK + (threadIdx.x & ~63); p0 < npix; p0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t p = p0 + lane;
        const int n = (int)min<int64_t>(64, npix - p0);
        uint8_t px[3] = {0, 0, 0};
        if (p < npix) {
            double r, g, b;
            if (fbx) {  // every contribution as a fixed-point term (order-independent sums)
                r = fx_value(fbx, npix, 0, p);
                g = fx_value(fbx, npix, 1, p);
                b = fx_value(fbx, npix, 2, p);
                if (fx_suspect(fbx, npix, p)) shadow_host[2] = RETRY_FIXED_RANGE;  // render again with f64
            } else {
                r = fb[p];
                g = fb[npix + p];
                b = fb[2 * npix + p];
            }
            r /= spp;
            g /= spp;
            b /= spp;
            double a0, a1, a2;
            resolve_pixel(r, g, b, a0, a1, a2, px);
            if (rgb) { rgb[p] = r; rgb[npix + p] = g; rgb[2 * npix + p] = b; }
        }
        if (u8) store_u8_chunk(u8 + 3 * p0, px, lane, n);
    }
}

// fb += the fixed-point sums (srt_trace's colours)
__global__ __launch_bounds__(BLOCK) void k_fx_combine(double* fb, const unsigned long long* fbx, int64_t npix,
                                                     uint32_t* flags) {
    bool bad = false;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < npix; p += (int64_t)gridDim.x * BLOCK) {
        for (int ch = 0; ch < 3; ++ch) fb[ch * npix + p] += fx_value(fbx, npix, ch, p);
        bad |= fx_suspect(fbx, npix, p);
    }
    if (bad) atomicOr(flags + 1, RETRY_FIXED_RANGE);
}

// the sample groups' partial sums of a frame-kernel pass into the framebuffer, in group order
__global__ __launch_bounds__(BLOCK) void k_fb_groups(double* fb, const double* fbg, int groups, int64_t npix, int first) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < 3 * npix; i += (int64_t)gridDim.x * BLOCK) {
        double v = fbg[i];
        for (int g = 1; g < groups; ++g) v += fbg[(int64_t)g * 3 * npix + i];
        fb[i] = first ? v : fb[i] + v;
    }
}

__global__ __launch_bounds__(BLOCK) void k_nearest(SceneView S, const double* O, const double* D, int64_t n, double* t,
                                                  int32_t* id, double* orient) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        d3 o = d3{O[i], O[n + i], O[2 * n + i]}, d = d3{D[i], D[n + i], D[2 * n + i]};
        double tn, on;
        bool ties;
        int c = nearest_hit(S, o, d, tn, on, ties);
        if (t) t[i] = tn;
        if (id) id[i] = c;
        if (orient) orient[i] = on;
    }
}

__global__ __launch_bounds__(BLOCK) void k_intersect_one(const srt_collider* c_generic, const double* O,
                                                        const double* D, int64_t n, double* out) {
    // generic pointer in the signature (kernel arguments stay in the global address space),
    // read through the constant address space inside
    const RT_RO srt_collider* c = (const RT_RO srt_collider*)c_generic;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        d3 o = d3{O[i], O[n + i], O[2 * n + i]}, d = d3{D[i], D[n + i], D[2 * n + i]};
        double orient;
        double t = collider_hit(*c, o, d, orient);
        out[i] = t;
        out[n + i] = orient;
    }
}

// Collider.get_Normal / get_uv and Primitive.get_uv at points P (the reference's per-hit plugin
// points, collider.py:12-17, sphere.py:54-64, plane.py:98-105, cuboid.py:142-187, skybox.py:29-32)
__global__ __launch_bounds__(BLOCK) void k_collider_surface(const srt_collider* c_generic, const double* P, int64_t n,
                                                           double* N, double* uv) {
    const RT_RO srt_collider* c = (const RT_RO srt_collider*)c_generic;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const d3 p = d3{P[i], P[n + i], P[2 * n + i]};
        if (N) {
            const d3 v = collider_normal<MAT_VATTR>(*c, p);
            N[i] = v.x;
            N[n + i] = v.y;
            N[2 * n + i] = v.z;
        }
        if (uv) {
            double u = 0.0, v = 0.0;
            collider_uv<MAT_VATTR>(*c, p, u, v);
            uv[i] = u;
            uv[n + i] = v;
        }
    }
}

// Material.get_Normal(hit) (material.py:18-36) at points P: the collider's normal, or with a normal
// map the map's texel (texture 0 of S) through the collider's inverse_basis_matrix, normalised;
// times the hit orientation
__global__ __launch_bounds__(BLOCK) void k_material_normal(SceneView S, const srt_collider* c_generic,
                                                          const srt_material* m_generic, const double* P,
                                                          const double* orient, int64_t n, double* N,
                                                          uint32_t* flags) {
    const RT_RO srt_collider* c = (const RT_RO srt_collider*)c_generic;
    const RT_RO srt_material* m = (const RT_RO srt_material*)m_generic;
    uint32_t err = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const d3 v = shading_normal<MAT_GENERIC | MAT_VATTR>(S, *c, *m, d3{P[i], P[n + i], P[2 * n + i]}, orient[i], err);
        N[i] = v.x;
        N[n + i] = v.y;
        N[2 * n + i] = v.z;
    }
    if (err) atomicOr(flags, err);
}

// image.get_color(hit): the texel of (u, v) through texture 0 of S (texture.py:27-39)
__global__ __launch_bounds__(BLOCK) void k_texture_lookup(SceneView S, const double* uv, int64_t n, double* rgb,
                                                         uint32_t* flags) {
    uint32_t err = 0;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const d3 c = tex_rgb(S, 0, uv[i], uv[n + i], err);
        rgb[i] = c.x;
        rgb[n + i] = c.y;
        rgb[2 * n + i] = c.z;
    }
    if (err) atomicOr(flags, err);
}

__global__ __launch_bounds__(BLOCK) void k_primary_rays(srt_camera cam, const double* J, int64_t n, double* O,
                                                       double* D) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        uint32_t row = (uint32_t)(i / cam.width), col = (uint32_t)(i - (int64_t)row * cam.width);
        double j[4] = {J[i], J[n + i], J[2 * n + i], J[3 * n + i]};
        d3 o, d;
        primary_ray(cam, cam.xs[col], cam.ys[row], j, o, d);
        O[i] = o.x; O[n + i] = o.y; O[2 * n + i] = o.z;
        D[i] = d.x; D[n + i] = d.y; D[2 * n + i] = d.z;
    }
}

// ---- row-band shards (SRT_RENDER_SHARDED, rt_device.h shard_of_row) -----------------------------
// Rank 0 gathers every rank's tiles (RCCL) and k_assemble writes them into the frame.
constexpr int MAX_RANKS = 64;
struct GatherTiles {
    const uint8_t* u8[MAX_RANKS];  // [rows_q][W][3]
    const double* rgb[MAX_RANKS];  // [3][rows_q * W]
    int64_t npix[MAX_RANKS];       // rows_q * W
};

__global__ __launch_bounds__(BLOCK) void k_assemble(GatherTiles T, int nranks, int64_t band, int64_t W,
                                                   int64_t H, uint8_t* u8, double* rgb) {
    const int64_t n = W * H;
    for (int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x; g < n; g += (int64_t)gridDim.x * BLOCK) {
        const int64_t y = g / W, x = g - y * W;
        const int q = shard_of_row(y, nranks, band);
        const int64_t l = shard_local_row(y, nranks, band) * W + x;
        if (u8) {
            const uint8_t* s = T.u8[q] + 3 * l;
            u8[3 * g] = s[0]; u8[3 * g + 1] = s[1]; u8[3 * g + 2] = s[2];
        }
        if (rgb) {
            const double* s = T.rgb[q];
            const int64_t np = T.npix[q];
            rgb[g] = s[l]; rgb[n + g] = s[np + l]; rgb[2 * n + g] = s[2 * np + l];
        }
    }
}

// SRT_RENDER_RGBX: the uint8 image as 4-byte pixels (R, G, B, 255) -- PIL's own layout of an "RGB"
// image, which it then takes in with a word copy per pixel instead of unpacking 3-byte pixels
__global__ __launch_bounds__(BLOCK) void k_rgbx(const uint8_t* rgb, uint32_t* rgbx, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (int64_t)gridDim.x * BLOCK)
        rgbx[i] = (uint32_t)rgb[3 * i] | ((uint32_t)rgb[3 * i + 1] << 8) | ((uint32_t)rgb[3 * i + 2] << 16) | 0xFF000000u;
}

std::vector<int32_t> band_rows(int64_t H, int n, int q, int64_t band) {
    std::vector<int32_t> r;
    for (int64_t y = 0; y < H; ++y)
        if (shard_of_row(y, n, band) == q) r.push_back((int32_t)y);
    return r;
}

template <typename T>
hipError_t dalloc(T** p, int64_t count) {
    return hipMalloc((void**)p, (size_t)std::max<int64_t>(count, 1) * sizeof(T));
}

// One device allocation of `cap` elements, released with its owner.  Converts to the plain pointer,
// so kernels' arguments and HIP calls take it as they take a T*.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            (void)reset();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { (void)reset(); }
    operator T*() const { return p; }
    hipError_t reset() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        return e;
    }
    // room for `count` elements: grows only, and a buffer that grows loses its contents
    int ensure(int64_t count) {
        if (count <= cap && p) return SRT_OK;
        (void)reset();
        if (dalloc(&p, count) != hipSuccess) return fail(SRT_ERR_MEMORY, "device allocation failed");
        cap = count;
        return SRT_OK;
    }
};
// a fixed buffer, allocated once
template <typename T>
hipError_t dalloc(DevBuf<T>* b, int64_t count) {
    (void)b->reset();
    const hipError_t e = dalloc(&b->p, count);
    if (e == hipSuccess) b->cap = count;
    return e;
}

// Device allocations made and released together: the buffers of one API call (freed on every exit
// path, the early HIP_TRY returns included), a scene's tables, a slot's queues or rings
struct DevList {
    std::vector<void*> p;
    DevList() = default;
    DevList(DevList&& o) noexcept : p(std::move(o.p)) { o.p.clear(); }
    DevList& operator=(DevList&& o) noexcept {
        if (this != &o) {
            clear();
            p = std::move(o.p);
            o.p.clear();
        }
        return *this;
    }
    ~DevList() { clear(); }
    void clear() {
        for (void* b : p) (void)hipFree(b);
        p.clear();
    }
    template <typename T>
    hipError_t alloc(T** out, int64_t count) {
        *out = nullptr;
        const hipError_t e = dalloc(out, count);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
    // an input of a call: `count` elements of `src` in a buffer of their own, copied on `st` (without
    // one, before the call returns)
    template <typename T>
    hipError_t in(T** out, const T* src, int64_t count, hipStream_t st = nullptr) {
        const hipError_t e = alloc(out, count);
        return e != hipSuccess ? e : copy(*out, src, count, st);
    }
    // `count` elements of an output back to the caller's `dst`
    template <typename T>
    static hipError_t copy(T* dst, const T* src, int64_t count, hipStream_t st = nullptr) {
        const size_t bytes = (size_t)count * sizeof(T);
        return st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st) : hipMemcpy(dst, src, bytes, hipMemcpyDefault);
    }
};

int grid_for(int64_t n, int max_blocks) {
    int64_t b = (n + BLOCK - 1) / BLOCK;
    if (b < 1) b = 1;
    return (int)std::min<int64_t>(b, max_blocks);
}

// seed the queue from caller rays (get_raycolor): ray i -> shard i % NSHARD, slot i / NSHARD
__global__ __launch_bounds__(BLOCK) void k_seed_queue(Queue q, int64_t seg, const double* O, const double* D,
                                                     const int32_t* med, int64_t n, uint32_t depth, uint32_t dfl,
                                                     uint32_t nmedia) {
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        int64_t dst = (i % NSHARD) * seg + i / NSHARD;
        uint32_t m = med ? (uint32_t)med[i] : 0u;
        if (m >= nmedia) m = 0u;  // out-of-table medium index: scene.n
        queue_store(q, dst, d3{O[i], O[n + i], O[2 * n + i]}, d3{D[i], D[n + i], D[2 * n + i]}, d3{1.0, 1.0, 1.0},
                    (uint32_t)i, pack_meta(m, depth, dfl), mix32(0x7A11u, (uint32_t)i));
    }
}

// srt_shade_level: the children one shading level appended to the queue shards, packed in shard
// order (block b = shard b, its rays at prefix[b] ..) into planar arrays of `total` rays
__global__ __launch_bounds__(BLOCK) void k_gather_children(Queue q, int64_t seg, const uint32_t* cnt,
                                                          const int64_t* prefix, int64_t total, double* O, double* D,
                                                          double* Wt, int32_t* parent, int32_t* medium, int32_t* depth,
                                                          int32_t* dfl) {
    const int s = blockIdx.x;
    const int64_t n = min((int64_t)cnt[s], seg);
    for (int64_t i = threadIdx.x; i < n; i += BLOCK) {
        const Ray r = queue_load(q, (int64_t)s * seg + i);
        const int64_t k = prefix[s] + i;
        O[k] = r.o.x; O[total + k] = r.o.y; O[2 * total + k] = r.o.z;
        D[k] = r.d.x; D[total + k] = r.d.y; D[2 * total + k] = r.d.z;
        Wt[k] = r.w.x; Wt[total + k] = r.w.y; Wt[2 * total + k] = r.w.z;
        parent[k] = (int32_t)r.pix;
        medium[k] = (int32_t)meta_medium(r.meta);
        depth[k] = (int32_t)meta_depth(r.meta);
        dfl[k] = (int32_t)meta_diffuse(r.meta);
    }
}


}  // namespace

// shape of one frame's passes (what the read-back of its counters needs)
struct FramePlan {
    bool frame = false;  // rendered by k_frame (counts are totals, not queue fills)
    int chain_from = 0;  // > 0: k_trace at this depth runs in chain mode and no deeper kernel is launched
    bool fuse = false;   // k_primary traces every depth (single-child scenes): no k_trace launch
    int64_t npix = 0;
    int64_t W = 0, H = 0;  // frame shape (a shard renders npix of W * H)
    bool sharded = false, gather_rgb = false, use_mt = false;
    int spp = 0, batch = 0, npass = 0, dcap = 0, nev = 0;
    int groups = 1;  // k_frame sample groups per tile (the largest pass's)
    int64_t cnt_words = 0, pass_words = 0;
};

constexpr int MAX_FRAME_SLOTS = 8;

// Buffers and stream of one frame in flight.  Synchronous calls use slot 0; pipelined
// (SRT_RENDER_ASYNC) frames rotate over the slots, each with its own stream, so one frame's
// low-occupancy tail (deep depths, resolve) overlaps the next frame's primary kernel.  Measured on
// ex1 1080p (ms/frame, device-resident): 1 slot 1.47, 2 slots 1.308, 3 slots 1.292; 1/8 shard 0.28 /
// 0.202 / 0.199.  HIP gives a process four hardware queues by default, and a stream that shares a
// queue with another waits behind that stream's work: the slot count follows the queues
// (default_slots), and host outputs are copied on the frame's own stream.
struct FrameSlot {
    hipStream_t stream = nullptr;
    hipEvent_t jit_ready = nullptr;  // recorded on the MT stream after this slot's jitter is generated
    hipEvent_t jit_free = nullptr;   // recorded on `stream` after the last kernel that reads the jitter
    hipEvent_t mt_jumped = nullptr;  // recorded on the MT stream after this slot's jump kernel
    bool jit_busy = false;           // `jit_free` guards the jitter buffer
    DevBuf<uint32_t> mt_win;         // segment windows of this slot's numpy-stream generation
    // ray queues: 2 x NSHARD segments of `seg` rays
    Queue q[2]{};
    int64_t seg = 0;
    DevList queue_bufs;
    // frame kernel rings (k_frame): nslot rings of ring_cap rays, one lock word per ring
    Queue ring{};
    int64_t ring_cap = 0;
    int nslot = 0;
    uint32_t* ring_lock = nullptr;  // (in ring_bufs)
    DevList ring_bufs;
    // frame buffers
    DevBuf<double> fb;
    DevBuf<double> fbg;  // k_frame sample groups' partial sums [groups][3][npix]
    DevBuf<unsigned long long> fbx;  // [3][npix] fixed-point sums + [npix] f32 magnitudes (fb_add)
    DevBuf<double> rgb;
    DevBuf<uint8_t> u8;
    DevBuf<double> jit;
    DevBuf<int32_t> hit;
    DevBuf<uint32_t> counts;  // [SRT_MAX_DEPTHS][NSHARD]
    DevBuf<uint32_t> flags;   // [2]
    DevBuf<unsigned long long> shadow;  // [NSHARD]
    std::vector<hipEvent_t> ev;
    uint32_t* host = nullptr;  // pinned: per-pass counters/flags, shadow count
    int64_t host_words = 0;
    // SRT_RENDER_SHARDED on rank 0: every rank's tiles (padded to the largest shard) and the frame
    DevBuf<uint8_t> g_u8;
    DevBuf<double> g_rgb;
    DevBuf<uint8_t> full_u8;
    DevBuf<double> full_rgb;
    // the frame's gather (srt_render_group posts it for all its contexts in one RCCL group)
    struct Gather {
        bool on = false;
        int64_t W = 0, H = 0, npix = 0, maxpix = 0, band = 1;
        bool want_u8 = false, want_rgb = false;
        uint8_t* dst_u8 = nullptr;  // where k_assemble writes (caller's device buffer or full_u8)
        double* dst_rgb = nullptr;
        uint8_t* host_u8 = nullptr;  // caller's host buffer (copied after k_assemble) or null
        double* host_rgb = nullptr;
    } gather;
    // counts/flags/shadow are zeroed by the kernels that consume them (k_pass_end, k_resolve); a
    // frame that did not complete leaves them dirty and the next one clears them first
    bool dirty = true;
    // asynchronous frames queued on this slot since the last synchronisation point
    int pending = 0;
    FramePlan plan;
};

struct srt_ctx {
    int device = 0;
    int max_blocks = 2048;
    int ncu = 256;
    static constexpr int64_t queue_budget = (int64_t)96 << 30;  // bytes for both ray queues
    // scene
    bool has_scene = false;
    SceneView S{};
    int max_depth = 0;
    int has_diffuse = 0;
    int fanout = 1;
    uint32_t mats = 0;  // material types present (selects the kernel variant)
    uint32_t seq = 0;   // the scene's collider sequence (rt_device.h seq_encode; 0: none, or option collider_seq 0)
    bool seq_on = true;  // option "collider_seq": kernels specialised to the scene's collider sequence when built
    // per-hit shading inputs (srt_shade_level_inputs): colliders whose material has SRT_MF_HIT_ALBEDO,
    // the scene's SRT_LIGHT_USER lights; a scene with either is shaded through that entry point only
    std::vector<uint8_t> col_hit_albedo;
    int n_user_lights = 0;
    bool needs_inputs = false;
    DevList scene_bufs;
    // texel pool (outside scene_bufs: survives re-uploads with the same texel_key)
    DevBuf<uint8_t> texels;
    uint64_t texel_key = 0;
    int64_t texel_bytes = 0;
    uint64_t texel_layout = 0;  // hash of the pool layout the records' offsets were remapped to
    bool texels_rgbx = false;  // the resident pool holds 3-channel images as RGBX
    // option "mt_jump_parts": blocks per jump window (0: mt_jump_parts's choice)
    int mt_parts_opt = 0;
    // camera tables (shared by the slots; uploaded only when they change)
    DevBuf<double> xs, ys;
    DevBuf<int32_t> rows;
    std::vector<uint8_t> cam_host[3];  // host copies of what xs / ys / rows hold
    DevBuf<uint32_t> mt;  // MT19937 jump tables (255 x 624), two round keys, two final windows
    // the y words (k_mt_y) of a generation's key: [0] / [1] those of the two final windows (made
    // by the end block that made the window, valid flag per window), [2] scratch for other keys
    DevBuf<uint32_t> mt_y;
    bool mt_y_valid[2] = {false, false};
    // band mode (a shard's rows of the numpy stream, rt_mt_kernel.h MtArgs::bands): per pass shape,
    // the segment list and its jump polynomials (host-made once, kept for the context's life)
    struct MtBandTab {
        int64_t key[6];
        uint64_t rows_hash;
        int nseg;
        int64_t band_len, band_period;  // merged segments store k % band_period < band_len (doubles)
        DevBuf<int64_t> bands;   // [nseg][4]
        DevBuf<uint32_t> polys;  // [nseg][624]
    };
    std::deque<MtBandTab> mt_bandtabs;  // (stable addresses: frames hold pointers into it)
    std::vector<std::pair<int64_t, DevBuf<uint32_t>>> mt_end_polys;  // frame-end jump polynomial per word count
    bool mt_bands_on = true;  // option "mt_bands"
    // option "mt_short": doubles per segment of a whole frame's stream when nothing else is in flight
    // (a synchronous frame -- Scene.render -- or the first of a pipeline): its generation cannot hide
    // behind earlier frames, and a segment's serial generator (624-word blocks, ~0.5 us each) sets the
    // frame's latency: 2^19-word tabulated segments 0.42 ms, 2^17-word ones ~0.1 ms for 4x the jumps,
    // made in band mode (host jump polynomials, cached per frame shape); 0: tabulated segments
    int64_t mt_short = 65536;
    // option "mt_pipe_split": doubles per band-mode segment of a pipelined whole frame behind others in
    // flight (0: the tabulated 2^19-word segments).  Band mode generates exactly the stored planes' runs
    // (a tabulated segment straddling a stored and a skipped plane generates both), each run cut at the
    // split: same box, ex1 1080p pipelined frames 0.84 ms tabulated, 0.794 at 2^18 doubles (the
    // tabulated segments' length), 1.12 at 2^19 (longer generator chains); profiles/r05_pipe_split_ab.txt
    int64_t mt_pipe_split = (int64_t)1 << 18;
    DevBuf<double> mt_out;  // staging for srt_mt19937_uniforms into host memory
    // -1 auto: k_frame for scenes whose rays branch (refractive / thin-film / diffuse fan-out),
    // per-depth wavefront kernels otherwise.  Measured (one MI355X, Mrays/s, wavefront vs frame):
    // ex1 1080p d5 13388 vs 10478, ex3 1080p d8 8950 vs 9585, ex4 4K d6 14081 vs 17494,
    // cornell 800x800 512 spp 3542 vs 4073.
    int use_frame = -1;
    bool use_bvh = true;  // option "bvh": 0 intersects mesh triangles one by one (comparison runs)
    // chain mode of the wavefront path (single-child scenes): from the first depth >= 1 whose ray
    // count in the previous frame of the same shape was below chain_rays
    int64_t chain_rays = 1000000;
    bool chain_ok = true;  // cleared when a tie produced a second child in chain mode
    int64_t hint_key[3] = {-1, -1, -1};
    int64_t hint[SRT_MAX_DEPTHS] = {};
    // frame slots; `f` is the one the current call works on
    FrameSlot slots[MAX_FRAME_SLOTS];
    // pipelined frames: slots they rotate over; the numpy-stream generation of single-pass frames on a
    // stream of its own (round 2-3 options "slots", "mt_stream", "copy_stream", removed in round 6: the
    // host-output copies on a stream of their own did not pay).  ex1 1080p, host outputs, one MI355X,
    // ms/frame: 3 slots 1.83; 2 slots
    // + copy stream 1.83; 3 slots + MT stream 1.82; 2 slots 2.20; 2 slots + MT stream 2.00; one rank's
    // shard of an 8-GPU frame (bench --shard-of 8, same box): 3 slots 0.627, 4 slots 0.544, 3 slots +
    // MT stream 0.857.  Default (default_slots): one slot per hardware queue HIP gives the process
    // but one, at least four: GPU_MAX_HW_QUEUES=7 (bench.py sets it) -> 6 slots: one rank of 8,
    // slowest rank 0.318 -> 0.265 ms per frame, the whole ex1 frame 1.30 -> 1.26 ms (8 slots: 0.41 /
    // 1.28; profiles/r03_slots_ab.txt)
    int nslots = 4;
    // where the numpy-stream generation runs: a high-priority stream of its own for whole frames (ex1
    // 1080p 1.80 -> 1.64 ms/frame, same box), the frame's stream for shards (round 4, same box: one
    // rank of 2 0.87 ms on a stream of its own, 0.67 on a high-priority one, 0.55 on the frame's
    // stream; of 4 0.33 / 0.48 / 0.32; of 8 0.20 / 0.33 / 0.21, profiles/r04_mt_stream_ab.txt).  The
    // generators of a whole pipelined frame run after its jump kernel on that stream (frame k+1's
    // jumps then wait behind frame k's generators); on the frame's own stream or on two high-priority
    // generator streams taken in turn (round-5 option "mt_gen_stream", removed in round 6) pipelined
    // ex1 frames took ~1.05 and 1.014-1.028 ms against 0.940 (profiles/r05_mt_generator_ab.txt).
    // option "deterministic" (default 1): contributions added to a pixel by other threads go into
    // order-independent fixed-point sums (bit-reproducible frames); 0: f64 atomics
    bool deterministic = true;
    bool fx_ok = true;  // cleared when a contribution left the fixed-point range (until the next scene)
    FrameSlot* f = &slots[0];
    bool pipeline = false;  // option "pipeline": size every slot on every frame (no first-use allocation)
    int next_slot = 0;      // slot of the next asynchronous frame
    int last_slot = 0;      // slot of the last asynchronous frame (its stats are reported)
    int async_pending = 0;  // asynchronous frames in flight (all slots)
    srt_stats async_stats{};
    // numpy-stream jitter generated on the device (render args `mt`): the state after the last
    // queued frame stays on the device (mt dump window) while consecutive asynchronous frames pass the
    // same host state, which srt_render_finish then writes
    srt_mt_state* mt_chain = nullptr;
    int mt_pos = 0;
    hipEvent_t mt_done = nullptr;  // recorded after the last frame's stream generation
    int mt_cur = 0;                // which of the two final-window buffers is current (mt_dump)
    // a generation stopped between its jump and its generator launches (an error return) leaves
    // windows that are not zero and possibly a partial end accumulator: every slot's window table,
    // end_acc and end_cnt are cleared before the next generation (mt_win_ensure)
    bool mt_dirty = false;
    // single-pass frames generate their numpy stream on a stream of their own, so the generation of
    // frame k+1 runs beside frame k's trace (their order is this stream's order)
    hipStream_t mt_stream = nullptr;
    bool mt_tables = false;
    // multi-GPU (srt_comm_init / srt_comm_init_all)
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    bool defer_gather = false;  // srt_render_group posts the gathers of all its contexts in one group
    bool retry_frame = false;   // the last finish_async failed only with RETRY_* bits (render the frame again)
    int shard_bands = 0;  // option "shard_bands": most row bands per rank (0: rt_device.h shard_kmax by the scene's fan-out)
    // option "fuse_primary": single-child scenes traced whole-path per pixel in k_primary (same image
    // bit for bit as the per-depth kernels); -1 (default) for frames of at least two resident
    // rounds of threads: ex1 1080p 1.308 -> 1.209 ms per frame, a rank of 4 0.47 -> 0.44, while a rank
    // of 8 (1.3 rounds) is faster per depth, 0.29 vs 0.35 (profiles/r03_fused_ab.txt)
    int fuse_primary = -1;
    // option "rehearse_assemble" = n (diagnostic, one GPU): a frame rendering rank 0's rows of an
    // n-rank job (rows given, not SRT_RENDER_SHARDED) also does rank 0's assembly -- k_assemble of its
    // tile and n - 1 stand-in tiles of the other ranks' shapes into the whole frame -- and hands back
    // the whole frame's uint8 image (host copy of W x H x 3 bytes), as a sharded rank 0 does after the
    // RCCL gather (the transfers themselves are not rehearsed)
    int rehearse_assemble = 0;
    int lean_blocks = 0;  // grid of k_primary_lean in pipelined whole frames (set to 2 blocks per CU)
    // the same for a shard's rows (set to 4 per CU: every rank of 4 rehearsed, slowest 0.321 -> 0.275 ms
    // per frame; of 8 unchanged, profiles/r05_lean_grid_ab.txt)
    int lean_blocks_shard = 0;
    bool sync_lean = false;     // option "sync_lean": synchronous frames run k_primary_lean too (measurement)
    int64_t lean_launches = 0;  // (srt_debug_lean_launches)
    // generator workgroup size of the current generation (mt_gen_launch): 256 for the pipelined frames
    // of a lean k_primary, else MT_GEN_THREADS; option "mt_gen_nt" (0 auto, 256 or 320) forces one
    int gen_nt = rtmt_dev::MT_GEN_THREADS;
    int mt_gen_nt_opt = 0;
    DevBuf<double> red;         // srt_comm_allreduce scratch
    // srt_render_prefetch: the numpy-stream generation of the synchronous whole frame srt_render is
    // about to be called for, queued before the caller lowers and uploads its scene (Scene.render);
    // the next srt_render with the same stream state and frame shape finds it queued and skips its
    // own launch.  Any other call that generates from the stream drops it.
    struct MtPrefetch {
        bool valid = false;
        uint32_t key[rtmt::N];
        int pos = 0;
        int64_t shape[8] = {};       // W, H, spp, batch, plane mask, slot, stream, generation flavour
        const void* bt[2] = {nullptr, nullptr};  // the band tables it used
        int final_pos = 0;
        hipStream_t gen_on = nullptr;
    } pf;
    int64_t pf_used = 0, pf_queued = 0;  // (srt_debug_prefetch_counts)
    DevBuf<unsigned long long> lane_stats;  // (srt_debug_lane_stats) [SRT_MAX_DEPTHS][2] or null
    // streams, events and the communicator (after the frames in flight; the context's device is
    // current); the members above then release the device memory
    ~srt_ctx();
};

namespace {

// the twelve arrays of a ray queue, `n` rays each (recorded in `bufs`)
int alloc_queue(Queue& q, int64_t n, DevList& bufs, const char* what) {
    double** dptr[9] = {&q.ox, &q.oy, &q.oz, &q.dx, &q.dy, &q.dz, &q.wr, &q.wg, &q.wb};
    for (double** p : dptr)
        if (bufs.alloc(p, n) != hipSuccess) return fail(SRT_ERR_MEMORY, what);
    uint32_t** uptr[3] = {&q.pix, &q.meta, &q.path};
    for (uint32_t** p : uptr)
        if (bufs.alloc(p, n) != hipSuccess) return fail(SRT_ERR_MEMORY, what);
    return SRT_OK;
}

// segment length of queues for `rays` queued rays per depth (spread over the shards with slack)
int64_t queue_seg_for(int64_t rays) {
    const int64_t seg = (rays + NSHARD - 1) / NSHARD;
    return seg + seg / 8 + 1024;
}

// make room for `rays` queued rays per depth
int ensure_queues(FrameSlot& f, int64_t rays) {
    const int64_t seg = queue_seg_for(rays);
    if (seg <= f.seg) return SRT_OK;
    f.queue_bufs.clear();
    f.seg = 0;
    for (Queue& q : f.q)
        if (int rc = alloc_queue(q, seg * NSHARD, f.queue_bufs, "ray queue allocation failed")) return rc;
    f.seg = seg;
    return SRT_OK;
}

// rings of the frame kernel: more rings than waves can ever be resident (32 per CU), so a wave
// always finds a free one; `cap` rays each (power of two)
int64_t ring_cap_for(int64_t cap) {
    int64_t k = 256;
    while (k < cap) k <<= 1;
    return k;
}
int ring_slots(const srt_ctx* c) { return std::max(1024, 2 * 32 * c->ncu); }

int ensure_ring(srt_ctx* c, FrameSlot& f, int64_t cap) {
    cap = ring_cap_for(cap);
    const int nslot = ring_slots(c);
    if (cap <= f.ring_cap && nslot <= f.nslot) return SRT_OK;
    f.ring_bufs.clear();
    f.ring_cap = 0;
    f.nslot = 0;
    if (int rc = alloc_queue(f.ring, cap * nslot, f.ring_bufs, "ray ring allocation failed")) return rc;
    if (f.ring_bufs.alloc(&f.ring_lock, nslot) != hipSuccess) return fail(SRT_ERR_MEMORY, "ring lock allocation failed");
    HIP_TRY(hipMemset(f.ring_lock, 0, (size_t)nslot * 4));
    f.ring_cap = cap;
    f.nslot = nslot;
    return SRT_OK;
}

template <typename T>
int upload(srt_ctx* c, const T* src, int64_t count, T** dst) {
    *dst = nullptr;
    if (count <= 0 || !src) return SRT_OK;
    HIP_TRY(c->scene_bufs.in(dst, src, count));
    return SRT_OK;
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}

// 0: null, 1: device memory, 2: pinned host memory (hipHostMalloc / registered), 3: other host memory
int ptr_kind(const void* p) {
    if (!p) return 0;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return 3;
    }
    if (a.type == hipMemoryTypeDevice) return 1;
    if (a.type == hipMemoryTypeHost) return 2;
    return 3;
}

#define NCCL_TRY(expr)                                                                          \
    do {                                                                                        \
        ncclResult_t _r = (expr);                                                               \
        if (_r != ncclSuccess)                                                                  \
            return fail(SRT_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(_r));      \
    } while (0)

// A scene with an SRT_MF_HIT_ALBEDO material or an SRT_LIGHT_USER light is shaded only by
// srt_shade_level_inputs (the hot kernels have no path for it): every other entry point refuses it
// before any launch
int refuse_inputs_scene(const char* who) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: the scene needs per-hit inputs (an SRT_MF_HIT_ALBEDO material or an "
             "SRT_LIGHT_USER light): it is shaded through srt_shade_level_inputs only", who);
    return fail(SRT_ERR_ARG, msg);
}

int check_flags(uint32_t f0) {
    if (f0 & ERR_INDEX)
        return fail(SRT_ERR_INDEX, "index out of bounds in a texture/table lookup (reference raises IndexError)");
    if (f0 & ERR_UNSUPPORTED) return fail(SRT_ERR_ARG, "uv requested on a Triangle (undefined in the reference)");
    if (f0 & ERR_NAME)
        return fail(SRT_ERR_NAME, "name 'M' is not defined (PointLight.get_L at a Glossy hit, as the reference "
                                  "sightpy/lights.py:30-31 raises)");
    return SRT_OK;
}

TraceParams base_params(const srt_ctx* c, const FrameSlot& f, uint64_t seed) {
    TraceParams P{};
    P.S = c->S;
    P.flags = f.flags;
    P.shadow = f.shadow;
    P.seg = f.seg;
    P.seed = seed;
    P.lane_stats = c->lane_stats;  // (read by k_primary_lean<.., true> only)
    return P;
}

// deepest depth index that can hold rays: max_ray_depth, +2 diffuse bounces without depth check
// (a child is made only while depth < max_ray_depth, so depth max_ray_depth is the last with rays;
// Diffuse bounces ignore max_ray_depth (diffuse.py:25-124) and add at most two more)
int depth_cap(const srt_ctx* c) { return std::min(SRT_MAX_DEPTHS - 2, c->max_depth + (c->has_diffuse ? 2 : 0)); }

// threads the fused paths want per pass: two rounds of the resident threads (4 SIMDs x OCC waves per CU)
int64_t fused_items(const srt_ctx* c) { return 2 * (int64_t)c->ncu * 4 * OCC * 64; }

// k_primary's sample groups per pixel (TraceParams::pix_groups): the fewest (a power of two, at most
// the pass's samples and 64) that give the pass enough threads
int pix_groups(const srt_ctx* c, int64_t npix, int ns, bool fused) {
    const int64_t want = fused ? fused_items(c) : (int64_t)c->max_blocks * 64;
    int g = 1;
    while (g * 2 <= std::min(ns, 64) && npix * g < want) g *= 2;
    // a BVH scene's paths differ widely in length (mesh hits traverse, the rest do not): one sample
    // per lane where the spp allows (up to 4 groups, dividing the samples evenly) gives the GPU twice
    // the waves to balance -- mesh 1080p 2 spp 5.94 -> 4.33 ms per frame, same box
    // (profiles/r04_mesh_pix_groups_ab.txt)
    if (c->mats & MAT_BVH)
        while (g * 2 <= std::min(ns, 4) && ns % (g * 2) == 0) g *= 2;
    // the fused paths take two groups whenever the samples split evenly: ex1 1080p 6 spp, same box,
    // the fused kernel 1.095 -> 1.050 ms per launch, device-resident frame 0.841 -> 0.830 ms
    // (profiles/r04_pix_groups_ab.txt)
    if (fused && g < 2 && ns % 2 == 0) g = 2;
    // the fused paths' tiles of 8 x 64 / g pixels (rt_primary_body.inc) need g <= 8
    if (fused && !(c->mats & MAT_BVH)) g = std::min(g, 8);
    return g;
}

size_t lut_bytes(const srt_ctx* c) { return (size_t)c->S.nlut_lds * 256 * sizeof(double); }

int trace_grid(const srt_ctx* c) { return std::max(NSHARD, (c->max_blocks / NSHARD) * NSHARD); }

int64_t depth_total(const uint32_t* cnt, int64_t seg) {
    int64_t t = 0;
    for (int s = 0; s < NSHARD; ++s) t += std::min<int64_t>(cnt[s], seg);
    return t;
}

}  // namespace

namespace {

// ---- numpy's stream on the device (rt_mt.h): scratch c->mt = jump tables | key 0 | key 1 | dump ----
constexpr int64_t MT_NTAB = rtmt::TABLE_WORDS;
uint32_t* mt_key0(srt_ctx* c) { return c->mt + MT_NTAB; }
// the final window of the last queued generation (two alternate, so the next frame's generation
// reads the previous one in place while writing its own)
uint32_t* mt_dump(srt_ctx* c) { return c->mt + MT_NTAB + (2 + c->mt_cur) * rtmt::N; }

int mt_ensure(srt_ctx* c) {
    if (c->mt) return SRT_OK;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mt_jump),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)MT_LDS_BYTES));
    // jump tables | two round keys | two final windows | the end window's accumulator + its counter
    HIP_TRY(dalloc(&c->mt, MT_NTAB + 5 * rtmt::N + 1));
    HIP_TRY(hipMemcpy(c->mt, rtmt::tables_flat(), MT_NTAB * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(c->mt + MT_NTAB + 4 * rtmt::N, 0, (rtmt::N + 1) * 4));
    HIP_TRY(dalloc(&c->mt_y, (int64_t)3 * MT_YBLOCKS * rtmt::N));
    return SRT_OK;
}

uint32_t* mt_dump_at(srt_ctx* c, int d) { return c->mt + MT_NTAB + (2 + d) * rtmt::N; }
uint32_t* mt_end_acc(srt_ctx* c) { return c->mt + MT_NTAB + 4 * rtmt::N; }
uint32_t* mt_end_cnt(srt_ctx* c) { return c->mt + MT_NTAB + 5 * rtmt::N; }
uint32_t* mt_ybuf(srt_ctx* c, int i) { return c->mt_y + (int64_t)i * MT_YBLOCKS * rtmt::N; }
int mt_end_reset(srt_ctx* c) {
    if (c->mt) HIP_TRY(hipMemset(mt_end_acc(c), 0, (rtmt::N + 1) * 4));  // end_acc [624] and end_cnt [1]
    return SRT_OK;
}

// The segment-window table of a slot's numpy-stream generation: zero when (re)allocated; from then
// on every window a jump XORs into is zeroed again by the generator that reads it.  After a
// generation that stopped between its jump and generator launches (srt_ctx::mt_dirty) every slot's
// table and the end accumulator are cleared first (device-synchronous: an error path only).
int mt_win_ensure(srt_ctx* c, FrameSlot& f, int64_t count) {
    if (c->mt_dirty) {
        HIP_TRY(hipDeviceSynchronize());
        for (FrameSlot& s : c->slots)
            if (s.mt_win) HIP_TRY(hipMemset(s.mt_win, 0, (size_t)s.mt_win.cap * 4));
        int rc = mt_end_reset(c);
        if (rc) return rc;
        c->mt_dirty = false;
    }
    if (count <= f.mt_win.cap && f.mt_win) return SRT_OK;
    int rc = f.mt_win.ensure(count);
    if (rc) return rc;
    HIP_TRY(hipMemset(f.mt_win, 0, (size_t)count * 4));
    return SRT_OK;
}

// Blocks per jump window (k_mt_jump parts): the option, else 4 (final build, same box, against 8:
// device-side whole frame 0.988 -> 0.979 ms, a rank of 8 0.204 -> 0.202, of 4 0.328 -> 0.318;
// profiles/r04_jump_parts_ab.txt)
int mt_jump_parts(const srt_ctx* c) { return c->mt_parts_opt ? c->mt_parts_opt : 4; }

// The y words of `key` for a generation on `st`: those an end block made with the key (a final
// window), else k_mt_y into the scratch buffer (one workgroup, ~34 blocks).  Generations of
// different frames are ordered by the key they hand on, so one scratch buffer suffices.
const uint32_t* mt_y_for(srt_ctx* c, hipStream_t st, const uint32_t* key) {
    for (int d = 0; d < 2; ++d)
        if (key == mt_dump_at(c, d) && c->mt_y_valid[d]) return mt_ybuf(c, d);
    hipLaunchKernelGGL(k_mt_y, dim3(1), dim3(MT_THREADS), 0, st, key, mt_ybuf(c, 2));
    return mt_ybuf(c, 2);
}

// x^end_jump(n_words) mod phi on the device, made once per word count (a few shapes per context)
int mt_end_poly_for(srt_ctx* c, int64_t n_words, const uint32_t** out) {
    for (auto& e : c->mt_end_polys)
        if (e.first == n_words) { *out = e.second; return SRT_OK; }
    DevBuf<uint32_t> d;
    HIP_TRY(dalloc(&d, rtmt::N));
    const std::vector<uint32_t> poly = rtmt::xpow_mod(rtmt::end_jump(n_words));
    HIP_TRY(hipMemcpy(d, poly.data(), rtmt::N * 4, hipMemcpyHostToDevice));
    *out = d;
    c->mt_end_polys.emplace_back(n_words, std::move(d));
    return SRT_OK;
}

// The generators of `nseg` segments, one workgroup each: five waves, or four (one per SIMD) for the
// frames of a lean k_primary (srt_ctx::gen_nt), which leaves room for exactly that beside its waves
void mt_gen_launch(srt_ctx* c, const MtArgs& G, int nseg, hipStream_t st, uint32_t* win) {
    if (c->gen_nt == 256)
        hipLaunchKernelGGL(k_mt_gen<256>, dim3(nseg), dim3(256), 0, st, G, win);
    else
        hipLaunchKernelGGL(k_mt_gen<MT_GEN_THREADS>, dim3(nseg), dim3(MT_GEN_THREADS), 0, st, G, win);
}

// Band mode table of one pass shape: the rows' runs of `ns` samples' stored planes, each segment
// with its jump polynomial x^(2 d0 - 1) mod phi (xpow_mod, ~2.5 ms each, over a few host threads).
// Regular runs (a shard's row bands: equal length, equal spacing) with short gaps are merged while
// a segment spans at most MT_MERGE_DOUBLES: it then generates through the other ranks' rows between
// them (stores masked by band_len / band_period), trading one jump (~110 us of a CU) for a few
// hundred generated blocks (a CU fraction); other runs are split at `split` doubles (2^18 for a
// shard's rows, srt_ctx::mt_short for a whole frame generated with nothing else in flight).
constexpr int MT_MAX_BANDS = 2048;
constexpr int64_t MT_MERGE_DOUBLES = 150000;
int mt_band_table(srt_ctx* c, int64_t W, int64_t Hf, int ns, int plane_mask, const int32_t* rows, int n_rows,
                  int64_t split, const srt_ctx::MtBandTab** out) {
    uint64_t h = 1469598103934665603ull;
    for (int k = 0; k < n_rows; ++k) h = (h ^ (uint64_t)(uint32_t)rows[k]) * 1099511628211ull;
    const int64_t key[6] = {W, Hf, ns, plane_mask, n_rows, split};
    for (auto& t : c->mt_bandtabs)
        if (!memcmp(t.key, key, sizeof key) && t.rows_hash == h) { *out = &t; return SRT_OK; }
    // runs of consecutive rows (first row, count)
    std::vector<std::pair<int, int>> runs;
    for (int k = 0; k < n_rows;) {
        int e = k + 1;
        while (e < n_rows && rows[e] == rows[e - 1] + 1) ++e;
        runs.emplace_back(rows[k], e - k);
        k = e;
    }
    // the regular pattern (the first run's length and the spacing of the first two runs), if any
    const int rlen = runs[0].second;
    const int rper = runs.size() > 1 ? runs[1].first - runs[0].first : 0;
    // merged only when the gaps are no longer than the runs (N = 2 shards): the merged segments' longer
    // generation is on the frame's critical path, and with longer gaps it cost more than the jumps it
    // saves (same box, ms per rank-frame, ex1 1080p, unmerged vs merged: N = 2 1.076 vs 0.991, N = 4
    // 0.579 vs 0.614, N = 8 0.339 vs 0.422)
    const bool regular_ok = rper > rlen && rper - rlen <= rlen;
    // local row of each run's first row (the shard's compact jitter layout [s][plane][rows][W])
    std::vector<int64_t> run_lrow(runs.size(), 0);
    for (size_t k = 1; k < runs.size(); ++k) run_lrow[k] = run_lrow[k - 1] + runs[k - 1].second;
    const int64_t npix = (int64_t)n_rows * W;
    std::vector<int64_t> segs;  // (first double, doubles, masked, local offset)
    for (int s = 0; s < ns; ++s)
        for (int j = 0; j < 4; ++j) {
            if (!((plane_mask >> j) & 1)) continue;
            const int64_t pbase = (int64_t)(s * 4 + j) * Hf;
            const int64_t lbase = (int64_t)(s * 4 + j) * npix;
            for (size_t k = 0; k < runs.size();) {
                size_t e = k + 1;
                if (regular_ok && runs[k].second == rlen)
                    while (e < runs.size() && runs[e].second == rlen && runs[e].first - runs[e - 1].first == rper &&
                           (int64_t)(runs[e].first + rlen - runs[k].first) * W <= MT_MERGE_DOUBLES)
                        ++e;
                int64_t d0 = (pbase + runs[k].first) * W;
                int64_t l0 = lbase + run_lrow[k] * W;
                if (e > k + 1) {
                    segs.insert(segs.end(), {d0, (int64_t)(runs[e - 1].first + rlen - runs[k].first) * W, 1, l0});
                } else {
                    int64_t n = (int64_t)runs[k].second * W;
                    while (n > 0) {
                        const int64_t m = std::min<int64_t>(n, split);
                        segs.insert(segs.end(), {d0, m, 0, l0});
                        d0 += m;
                        l0 += m;
                        n -= m;
                    }
                }
                k = e;
            }
        }
    const int nseg = (int)(segs.size() / 4);
    *out = nullptr;
    if (nseg > MT_MAX_BANDS || nseg == 0) return SRT_OK;  // (the tabulated segments instead)
    std::vector<uint32_t> polys((size_t)nseg * rtmt::N, 0u);
    // (xpow_mod ~2.5 ms per polynomial: up to 16 host threads, the GPU boxes' CPU share per GPU)
    const int nth = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (int w = 0; w < nth; ++w)
        th.emplace_back([&, w] {
            for (int i = w; i < nseg; i += nth) {
                if (segs[4 * i] == 0) continue;  // starts from the key
                const std::vector<uint32_t> p = rtmt::xpow_mod((uint64_t)(2 * segs[4 * i] - 1));
                std::copy(p.begin(), p.end(), polys.begin() + (size_t)i * rtmt::N);
            }
        });
    for (auto& t : th) t.join();
    srt_ctx::MtBandTab T{};
    memcpy(T.key, key, sizeof key);
    T.rows_hash = h;
    T.nseg = nseg;
    T.band_len = (int64_t)rlen * W;
    T.band_period = (int64_t)std::max(rper, 1) * W;
    HIP_TRY(dalloc(&T.bands, (int64_t)segs.size()));
    HIP_TRY(dalloc(&T.polys, (int64_t)polys.size()));
    HIP_TRY(hipMemcpy(T.bands, segs.data(), segs.size() * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(T.polys, polys.data(), polys.size() * 4, hipMemcpyHostToDevice));
    c->mt_bandtabs.push_back(std::move(T));
    *out = &c->mt_bandtabs.back();
    return SRT_OK;
}

// Band mode generation of n_words words from (key, pos): only the table's segments are generated
// (their doubles at their place in `out`, the whole pass's layout), every one jumped to from the key;
// the final window (next key) and its y come from the jump kernel's end block.
int mt_launch_bands(srt_ctx* c, hipStream_t st, uint32_t* win, const uint32_t* key, int pos, int64_t n_words,
                    const srt_ctx::MtBandTab& T, double* out, int* final_pos, const uint32_t* end_poly,
                    hipEvent_t key_ready, hipStream_t gst = nullptr, hipEvent_t jumped = nullptr,
                    hipStream_t* gen_on = nullptr) {
    const int64_t abs_end = pos + n_words;
    const int64_t dump_abs = ((abs_end + rtmt::N - 1) / rtmt::N - 1) * rtmt::N;
    MtArgs A{};
    A.key = key;
    A.tab = T.polys;
    A.bands = T.bands;
    A.band_len = T.band_len;
    A.band_period = T.band_period;
    A.out = out;
    A.words = n_words;
    A.double_base = 0;
    A.n_out = INT64_MAX;
    A.pos = pos;
    A.dump_at = dump_abs;
    A.dump_dst = mt_dump_at(c, c->mt_cur ^ 1);
    A.end_poly = end_poly;
    A.end_at = (int64_t)rtmt::end_jump(n_words);
    A.key_in_win = 1;
    A.compact = 1;  // the shard's own layout (srt_render reads it by local pixel)
    A.y = mt_y_for(c, st, key);
    A.y_next = mt_ybuf(c, c->mt_cur ^ 1);
    A.end_acc = mt_end_acc(c);
    A.end_cnt = mt_end_cnt(c);
    A.parts = mt_jump_parts(c);
    // the segment windows are XOR-accumulated by their jump parts into the table, which is zero here:
    // zeroed when allocated (mt_win_ensure), and every generator zeroes the window it read
    c->mt_dirty = true;  // (until the generators that zero the windows are queued)
    hipLaunchKernelGGL(k_mt_jump, dim3((T.nseg + 1) * A.parts), dim3(MT_THREADS), mt_jump_lds_bytes(A.parts), st, A,
                       win);
    HIP_TRY(hipGetLastError());
    if (key_ready) HIP_TRY(hipEventRecord(key_ready, st));
    MtArgs G = A;
    G.dump_dst = nullptr;
    G.y_next = nullptr;
    if (gst && gst != st) {  // the generators on their own stream, after the windows they start from
        HIP_TRY(hipEventRecord(jumped, st));
        HIP_TRY(hipStreamWaitEvent(gst, jumped, 0));
    } else {
        gst = st;
    }
    mt_gen_launch(c, G, T.nseg, gst, win);
    HIP_TRY(hipGetLastError());
    if (gen_on) *gen_on = gst;
    c->mt_dirty = false;
    c->mt_y_valid[c->mt_cur ^ 1] = true;
    c->mt_cur ^= 1;
    *final_pos = (int)(abs_end - dump_abs);
    return SRT_OK;
}

// Queue on `st`: from the key window `key` (device) at position `pos`, n_out doubles into `out`
// (device) and n_skip more draws; the window holding the last consumed word becomes mt_dump(c).  Returns the
// numpy position of that window in *final_pos.  `plane` > 0: only the doubles of the planes
// (index % 4) in `plane_mask` are stored (a pinhole camera reads no lens-disk pair).
// `win`: the segment-window table of this generation (SEGS x 624 words; per frame slot, as pipelined
// frames generate concurrently).  `end_poly` (x^end_at mod phi, device) on a one-round generation:
// k_mt_jump also makes the final window, and `key_ready` is recorded right after it -- the next
// frame's generation may start then, beside this one's generators.
int mt_launch(srt_ctx* c, hipStream_t st, uint32_t* win, const uint32_t* key, int pos, int64_t n_out, int64_t n_skip,
              double* out, int* final_pos, int64_t plane = 0, int plane_mask = 15, const uint32_t* end_poly = nullptr,
              int64_t end_at = 0, hipEvent_t key_ready = nullptr, hipStream_t gst = nullptr,
              hipEvent_t jumped = nullptr, hipStream_t* gen_on = nullptr) {
    if (gen_on) *gen_on = st;
    uint32_t* keys[2] = {c->mt + MT_NTAB, c->mt + MT_NTAB + rtmt::N};
    const rtmt::Plan plan = rtmt::make_plan(pos, 2 * (n_out + n_skip));
    if (plan.rounds.size() != 1) end_poly = nullptr;
    for (size_t r = 0; r < plan.rounds.size(); ++r) {
        const rtmt::Round& R = plan.rounds[r];
        MtArgs A{};
        A.key = r == 0 ? key : keys[r & 1];
        A.tab = c->mt;
        A.out = out;
        A.chain_dst = R.chain ? keys[(r + 1) & 1] : nullptr;
        A.dump_dst = R.dump_at >= 0 ? c->mt + MT_NTAB + (2 + (c->mt_cur ^ 1)) * rtmt::N : nullptr;
        A.words = R.words;
        A.double_base = R.double_base;
        A.n_out = n_out;
        A.dump_at = R.dump_at;
        A.pos = R.pos;
        // the block's doubles span at most two planes when a plane holds >= 312 of them
        A.plane = plane >= 1024 ? plane : 0;
        A.plane_mask = plane_mask;
        // segment windows (and the final window), then the generators
        const bool end = end_poly && A.dump_dst;
        if (end) {
            A.end_poly = end_poly;
            A.end_at = end_at;
        }
        const int jump_blocks = (R.nseg - 1) + (end ? 1 : 0);
        A.key_in_win = jump_blocks > 0;
        if (A.dump_dst) {
            A.y_next = end ? mt_ybuf(c, c->mt_cur ^ 1) : nullptr;
            c->mt_y_valid[c->mt_cur ^ 1] = end;  // (a generator segment makes the window, not its y)
        }
        if (jump_blocks > 0) {
            c->mt_dirty = true;  // (until the generators that zero the windows are queued)
            A.y = mt_y_for(c, st, A.key);
            A.end_acc = mt_end_acc(c);
            A.end_cnt = mt_end_cnt(c);
            A.parts = mt_jump_parts(c);
            // the segment windows are XOR-accumulated by their jump parts (into zeroed windows: see
            // mt_launch_bands)
            hipLaunchKernelGGL(k_mt_jump, dim3(jump_blocks * A.parts), dim3(MT_THREADS), mt_jump_lds_bytes(A.parts),
                               st, A, win);
            HIP_TRY(hipGetLastError());
        }
        if (end && key_ready) HIP_TRY(hipEventRecord(key_ready, st));
        MtArgs G = A;
        G.y_next = nullptr;
        if (end) G.dump_dst = nullptr;  // (made by the jump kernel)
        // the generators on their own stream when the jump kernel made the final window (a one-round
        // generation with the frame-end jump): nothing after them on `st` reads what they write
        hipStream_t g = st;
        if (gst && gst != st && end && plan.rounds.size() == 1) {
            HIP_TRY(hipEventRecord(jumped, st));
            HIP_TRY(hipStreamWaitEvent(gst, jumped, 0));
            g = gst;
        }
        mt_gen_launch(c, G, R.nseg, g, win);
        HIP_TRY(hipGetLastError());
        if (gen_on) *gen_on = g;
        c->mt_dirty = false;
    }
    c->mt_cur ^= 1;
    *final_pos = plan.final_pos;
    return SRT_OK;
}

// Read back a completed frame (its stream has been synchronised): error/overflow flags OR-ed over
// every pass (and every asynchronous frame since the last synchronisation point), per-depth counts
// and kernel times of the frame's passes.  Returns SRT_RETRY_OVERFLOW when a queue shard overflowed.
// `retry` receives the RETRY_* bits of every pass.
constexpr int SRT_RETRY = 1;
int collect_frame(srt_ctx* c, const FrameSlot& f, const FramePlan& F, srt_stats& S, uint32_t* retry = nullptr) {
    uint32_t bits = 0;
    for (int p = 0; p < F.npass; ++p) {
        const uint32_t* hp = f.host + p * F.pass_words;
        int rc;
        if ((rc = check_flags(hp[F.cnt_words]))) return rc;
        bits |= hp[F.cnt_words + 1];
    }
    bits |= f.host[F.npass * F.pass_words + 2];
    if (bits & RETRY_CHAIN_TIE) c->chain_ok = false;  // no chain mode for this scene any more
    if (bits & RETRY_FIXED_RANGE) c->fx_ok = false;   // f64 atomics for this scene
    if (retry) *retry = bits;
    if (bits) return SRT_RETRY;
    double ms_trace = 0.0, ms_primary = 0.0;
    for (int d = 0; d < SRT_MAX_DEPTHS; ++d) S.rays_per_depth[d] = 0;
    for (int p = 0; p < F.npass; ++p) {
        const uint32_t* hp = f.host + p * F.pass_words;
        if (depth_total(hp + (int64_t)(F.dcap + 1) * NSHARD, (F.frame || F.fuse) ? INT64_MAX : f.seg) != 0)
            return fail(SRT_ERR_DEPTH, "rays alive after the depth cap");
        if (F.frame) {
            // k_frame counts every ray it traces (per shard), depth 0 included
            for (int d = 0; d <= F.dcap; ++d)
                for (int k = 0; k < NSHARD; ++k) S.rays_per_depth[d] += hp[(int64_t)d * NSHARD + k];
        } else {
            S.rays_per_depth[0] += (int64_t)std::min(F.batch, F.spp - p * F.batch) * F.npix;
            for (int d = 1; d <= F.dcap; ++d)
                S.rays_per_depth[d] += depth_total(hp + (int64_t)d * NSHARD, F.fuse ? INT64_MAX : f.seg);
        }
        const hipEvent_t* ev = f.ev.data() + (int64_t)p * F.nev;
        float ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ms_primary += ms;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[F.chain_from > 0 ? F.chain_from + 1 : F.dcap + 1]));
        ms_trace += ms;
    }
    const uint32_t* hshadow = f.host + F.npass * F.pass_words;
    S.passes = F.npass;
    S.ms_trace_kernels = ms_trace;
    S.ms_primary_kernel = ms_primary;
    S.ms_device = ms_trace;
    S.shadow_rays = (int64_t)(hshadow[0] | (uint64_t)hshadow[1] << 32);
    S.n_depths = F.dcap + 1;
    S.kernel_path = F.frame ? 1 : (F.fuse ? 2 : 0);
    S.chain_from = F.chain_from;
    S.total_rays = 0;
    for (int d = 0; d <= F.dcap; ++d) S.total_rays += S.rays_per_depth[d];
    // per-pass ray counts of this frame shape: the next frame's chain-mode plan
    c->hint_key[0] = F.npix; c->hint_key[1] = F.spp; c->hint_key[2] = F.batch;
    for (int d = 0; d < SRT_MAX_DEPTHS; ++d) c->hint[d] = S.rays_per_depth[d] / std::max(1, F.npass);
    return SRT_OK;
}

// zero the pinned flag words of every pass (only while no frame is in flight)
void clear_host_flags(FrameSlot& f, const FramePlan& F) {
    for (int p = 0; p < F.npass; ++p) {
        f.host[p * F.pass_words + F.cnt_words] = 0u;
        f.host[p * F.pass_words + F.cnt_words + 1] = 0u;
    }
    f.host[F.npass * F.pass_words + 2] = 0u;  // k_resolve's fixed-point range check
}

// Stream and counters of a slot, created on first use.
int ensure_slot(FrameSlot& f) {
    if (f.stream) return SRT_OK;
    HIP_TRY(hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&f.jit_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.jit_free, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.mt_jumped, hipEventDisableTiming));
    HIP_TRY(dalloc(&f.counts, SRT_MAX_DEPTHS * NSHARD));
    HIP_TRY(dalloc(&f.flags, 2));
    HIP_TRY(dalloc(&f.shadow, NSHARD));
    f.dirty = true;
    return SRT_OK;
}

void free_slot(FrameSlot& f) {
    if (!f.stream) return;
    (void)hipStreamSynchronize(f.stream);
    // the device memory first (its owners release it), then the events, the pinned memory and the stream
    const std::vector<hipEvent_t> ev = f.ev;
    const hipEvent_t own[3] = {f.jit_ready, f.jit_free, f.mt_jumped};
    uint32_t* const host = f.host;
    const hipStream_t stream = f.stream;
    f = FrameSlot{};
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    if (host) (void)hipHostFree(host);
    for (hipEvent_t e : own) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(stream);
}

// Wait for the asynchronous frames in flight and check them (flags accumulated over all of them,
// stats of the last).  An overflow grows the queues and is reported as an error: those frames are
// wrong and must be rendered again.
int wait_frames(srt_ctx* c, srt_stats* st) {
    c->retry_frame = false;
    if (c->async_pending == 0) {
        if (st) *st = c->async_stats;
        return SRT_OK;
    }
    for (FrameSlot& f : c->slots)
        if (f.stream) HIP_TRY(hipStreamSynchronize(f.stream));
    c->async_pending = 0;
    if (c->mt_chain) {  // numpy's state after the last asynchronous frame's draws
        HIP_TRY(hipMemcpy(c->mt_chain->key, mt_dump(c), rtmt::N * 4, hipMemcpyDeviceToHost));
        c->mt_chain->pos = c->mt_pos;
        c->mt_chain = nullptr;
    }
    int first_err = SRT_OK;
    bool overflow = false;
    srt_stats last{};
    for (int k = 0; k < MAX_FRAME_SLOTS; ++k) {
        FrameSlot& f = c->slots[(c->last_slot + 1 + k) % MAX_FRAME_SLOTS];  // the last frame's slot last
        if (!f.pending) continue;
        srt_stats S{};
        uint32_t bits = 0;
        int rc = collect_frame(c, f, f.plan, S, &bits);
        clear_host_flags(f, f.plan);
        f.pending = 0;
        if (rc == SRT_RETRY) {
            overflow = true;
            if ((bits & RETRY_OVERFLOW) &&
                (rc = f.plan.frame ? ensure_ring(c, f, 2 * f.ring_cap) : ensure_queues(f, 2 * f.seg * NSHARD))) {
                first_err = first_err ? first_err : rc;
            }
        } else if (rc) {
            first_err = first_err ? first_err : rc;
        } else {
            last = S;
        }
    }
    if (first_err) return first_err;
    c->retry_frame = overflow;
    if (overflow)
        return fail(SRT_ERR_MEMORY, "a ray queue overflowed (queues grown), a tie met chain mode (chain mode "
                                    "off) or a colour left the fixed-point range (f64 sums from now on) during an "
                                    "asynchronous frame: render that frame again");
    c->async_stats = last;
    if (st) *st = last;
    return SRT_OK;
}

// wait_frames for the entry points: leaves slot 0 current
int finish_async(srt_ctx* c, srt_stats* st) {
    const int rc = wait_frames(c, st);
    c->f = &c->slots[0];
    return rc;
}

// copy `bytes` from host `src` to device `dst` (on `st`) unless `shadow` (the host copy of what dst
// holds) already equals it.  The shadow is invalidated whenever the buffer is reallocated (DevBuf::ensure).
// The camera tables are shared by the frame slots: the frames in flight are waited for before a change.
int upload_if_changed(srt_ctx* c, hipStream_t st, void* dst, std::vector<uint8_t>& shadow, const void* src,
                      size_t bytes) {
    const bool dev = is_device_ptr(src);
    if (!dev && shadow.size() == bytes && !memcmp(shadow.data(), src, bytes)) return SRT_OK;
    int rc = c->async_pending > 0 ? wait_frames(c, nullptr) : SRT_OK;
    if (rc) return rc;
    if (dev)
        shadow.clear();
    else
        shadow.assign((const uint8_t*)src, (const uint8_t*)src + bytes);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    return SRT_OK;
}

int64_t shard_npix(const FrameSlot::Gather& G, int nranks, int q) {
    return shard_rank_rows(G.H, nranks, q, G.band) * G.W;
}

// Post this rank's part of the frame's gather on its stream (inside an RCCL group): rank 0 receives
// every other rank's uint8 (and linear-RGB) tile, the others send theirs.
int gather_post(srt_ctx* c) {
    const FrameSlot::Gather& G = c->f->gather;
    if (!G.on || c->nranks == 1 || !c->comm) return SRT_OK;  // (no communicator: a rehearsed shard)
    hipStream_t st = c->f->stream;
    if (c->rank == 0) {
        for (int q = 1; q < c->nranks; ++q) {
            const int64_t np = shard_npix(G, c->nranks, q);
            NCCL_TRY(ncclRecv(c->f->g_u8 + (int64_t)q * G.maxpix * 3, (size_t)(3 * np), ncclUint8, q, c->comm, st));
            if (G.want_rgb)
                NCCL_TRY(ncclRecv(c->f->g_rgb + (int64_t)q * G.maxpix * 3, (size_t)(3 * np), ncclFloat64, q, c->comm, st));
        }
    } else {
        NCCL_TRY(ncclSend(c->f->u8, (size_t)(3 * G.npix), ncclUint8, 0, c->comm, st));
        if (G.want_rgb) NCCL_TRY(ncclSend(c->f->rgb, (size_t)(3 * G.npix), ncclFloat64, 0, c->comm, st));
    }
    return SRT_OK;
}

// Rank 0, after the gather: the tiles into the frame, then to the caller's host buffers if any.
int gather_finish(srt_ctx* c) {
    const FrameSlot::Gather& G = c->f->gather;
    if (!G.on || c->rank != 0 || (c->nranks > 1 && !c->comm)) return SRT_OK;
    GatherTiles T{};
    for (int q = 0; q < c->nranks; ++q) {
        T.u8[q] = q == 0 ? c->f->u8 : c->f->g_u8 + (int64_t)q * G.maxpix * 3;
        T.rgb[q] = q == 0 ? c->f->rgb : c->f->g_rgb + (int64_t)q * G.maxpix * 3;
        T.npix[q] = shard_npix(G, c->nranks, q);
    }
    hipStream_t st = c->f->stream;
    hipLaunchKernelGGL(k_assemble, dim3(grid_for(G.W * G.H, c->max_blocks)), dim3(BLOCK), 0, st, T, c->nranks, G.band, G.W, G.H,
                       G.want_u8 ? G.dst_u8 : nullptr, G.want_rgb ? G.dst_rgb : nullptr);
    HIP_TRY(hipGetLastError());
    if (G.host_u8) HIP_TRY(hipMemcpyAsync(G.host_u8, G.dst_u8, (size_t)3 * G.W * G.H, hipMemcpyDeviceToHost, st));
    if (G.host_rgb)
        HIP_TRY(hipMemcpyAsync(G.host_rgb, G.dst_rgb, (size_t)3 * G.W * G.H * 8, hipMemcpyDeviceToHost, st));
    return SRT_OK;
}

// The frame's gather on its own (one rank per process): post it in a group, assemble on rank 0.
int gather_frame(srt_ctx* c) {
    if (c->nranks > 1) {
        NCCL_TRY(ncclGroupStart());
        int rc = gather_post(c);
        NCCL_TRY(ncclGroupEnd());
        if (rc) return rc;
    }
    return gather_finish(c);
}

}  // namespace

srt_ctx::~srt_ctx() {
    for (FrameSlot& s : slots) free_slot(s);
    scene_bufs.clear();
    if (comm) (void)ncclCommDestroy(comm);
    if (mt_done) (void)hipEventDestroy(mt_done);
    if (mt_stream) (void)hipStreamDestroy(mt_stream);
}

extern "C" {

int srt_abi_version(void) { return SRT_ABI_VERSION; }

const char* srt_last_error(void) { return g_err.c_str(); }

int srt_device_count(int* count) {
    if (!count) return fail(SRT_ERR_ARG, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(SRT_ERR_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return SRT_OK;
}

// frame slots by default: HIP's hardware queues per process (GPU_MAX_HW_QUEUES, default 4) but one
// for the generation stream, at least 4, at most MAX_FRAME_SLOTS
static int default_slots() {
    const char* e = getenv("GPU_MAX_HW_QUEUES");
    const int q = e ? atoi(e) : 4;
    return std::max(4, std::min(MAX_FRAME_SLOTS, q - 1));
}

int srt_create(int device, srt_ctx** out) {
    if (!out) return fail(SRT_ERR_ARG, "out is null");
    *out = nullptr;
    HIP_TRY(hipSetDevice(device));
    srt_ctx* c = new srt_ctx();
    c->nslots = default_slots();
    c->device = device;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    c->ncu = prop.multiProcessorCount;
    // 4 x OCC blocks per CU = the CU's resident wave slots (OCC per SIMD): one wave-sized block
    // (the frame kernel) per slot, or four rounds of the OCC resident 256-thread blocks of the
    // grid-stride kernels
    c->max_blocks = prop.multiProcessorCount * 4 * OCC;
    c->lean_blocks = prop.multiProcessorCount * 2;
    c->lean_blocks_shard = prop.multiProcessorCount * 4;
    int rc = ensure_slot(c->slots[0]);
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return SRT_OK;
}

int srt_destroy(srt_ctx* c) {
    if (!c) return SRT_OK;
    (void)hipSetDevice(c->device);
    (void)finish_async(c, nullptr);
    delete c;  // (~srt_ctx, then the members that own device memory)
    return SRT_OK;
}

int srt_set_option(srt_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return fail(SRT_ERR_ARG, "null ctx/key");
    c->pf.valid = false;  // (an option may change the streams or the generation a prefetch assumed)
    if (!strcmp(key, "pipeline")) { c->pipeline = value != 0; return SRT_OK; }
    if (!strcmp(key, "bvh")) { c->use_bvh = value != 0; return SRT_OK; }
    if (!strcmp(key, "mt_bands")) { c->mt_bands_on = value != 0; return SRT_OK; }
    if (!strcmp(key, "collider_seq")) { c->seq_on = value != 0; return SRT_OK; }
    if (!strcmp(key, "mt_pipe_split")) {
        if (value != 0 && (value < 4096 || value > ((int64_t)1 << 24)))
            return fail(SRT_ERR_ARG, "mt_pipe_split: 0 or 4096 .. 2^24 doubles");
        c->mt_pipe_split = value;
        return SRT_OK;
    }
    if (!strcmp(key, "mt_gen_nt")) {
        if (value != 0 && value != 256 && value != 320) return fail(SRT_ERR_ARG, "mt_gen_nt: 0 (auto), 256 or 320");
        c->mt_gen_nt_opt = (int)value;
        return SRT_OK;
    }
    if (!strcmp(key, "sync_lean")) { c->sync_lean = value != 0; return SRT_OK; }
    if (!strcmp(key, "rehearse_assemble")) {
        if (value != 0 && (value < 2 || value > MAX_RANKS)) return fail(SRT_ERR_ARG, "rehearse_assemble: 0 or 2 .. 64");
        c->rehearse_assemble = (int)value;
        return SRT_OK;
    }
    if (!strcmp(key, "mt_short")) {
        if (value != 0 && (value < 4096 || value > ((int64_t)1 << 24))) return fail(SRT_ERR_ARG, "mt_short: 0 or 4096 .. 2^24 doubles");
        c->mt_short = value;
        return SRT_OK;
    }
    if (!strcmp(key, "mt_jump_parts")) {
        if (value != 0 && (value < MT_MIN_PARTS || value > MT_MAX_PARTS))
            return fail(SRT_ERR_ARG, "mt_jump_parts: 0 (auto) or 2 .. 8");
        c->mt_parts_opt = (int)value;
        return SRT_OK;
    }
    if (!strcmp(key, "shard_bands")) {
        if (value < 0 || value > 4096) return fail(SRT_ERR_ARG, "shard_bands: 0 (auto) .. 4096");
        c->shard_bands = (int)value;
        return SRT_OK;
    }
    if (!strcmp(key, "chain_rays")) { c->chain_rays = value; return SRT_OK; }
    if (!strcmp(key, "fuse_primary")) { c->fuse_primary = (int)value; return SRT_OK; }
    if (!strcmp(key, "frame_kernel")) { c->use_frame = value < 0 ? -1 : (value != 0); return SRT_OK; }
    if (!strcmp(key, "deterministic")) {
        HIP_TRY(hipSetDevice(c->device));
        int rc = finish_async(c, nullptr);
        if (rc) return rc;
        c->deterministic = value != 0;
        return SRT_OK;
    }
    if (!strcmp(key, "rehearse_shard")) {
        // diagnostic: act as rank (value & 255) of (value >> 8) ranks without a communicator, so one
        // GPU can render the shards of an N-rank frame in turn (no gather; SRT_RENDER_RGB_ROWS still
        // writes the rank's rows into the host frame).  0 ends the rehearsal.
        if (c->comm) return fail(SRT_ERR_ARG, "the context has a communicator");
        const int n = value ? (int)(value >> 8) : 1, r = value ? (int)(value & 255) : 0;
        if (n < 1 || n > MAX_RANKS || r >= n) return fail(SRT_ERR_ARG, "rehearse_shard: (nranks << 8) | rank");
        HIP_TRY(hipSetDevice(c->device));
        int rc = finish_async(c, nullptr);
        if (rc) return rc;
        c->nranks = n;
        c->rank = r;
        return SRT_OK;
    }
    return fail(SRT_ERR_ARG, std::string("unknown option ") + key);
}

// ---- srt_upload_scene, step by step ----
// 1. the descriptor's own consistency (no HIP call)
static int check_scene_desc(const srt_scene_desc* d) {
    if (d->n_colliders < 0 || d->n_materials < 0 || d->n_media < 1 || d->n_media > 255)
        return fail(SRT_ERR_ARG, "scene needs 1 <= n_media <= 255 (row 0 = scene.n)");
    for (int i = 0; i < d->n_colliders; ++i) {
        const srt_collider& cc = d->colliders[i];
        if (cc.type < 0 || cc.type > 3) return fail(SRT_ERR_ARG, "bad collider type");
        if (cc.material < 0 || cc.material >= d->n_materials) return fail(SRT_ERR_ARG, "collider material out of range");
    }
    if (!d->media) return fail(SRT_ERR_ARG, "media table is null");
    if (d->n_lights > 0 && d->n_colliders > 0 && !d->light_local) return fail(SRT_ERR_ARG, "light_local is null");
    if (d->n_importance > 0 && !d->importance) return fail(SRT_ERR_ARG, "importance table is null");
    if (d->n_textures > 0 && (!d->textures || (d->texel_bytes > 0 && !d->texels)))
        return fail(SRT_ERR_ARG, "texture tables are null");
    for (int i = 0; i < d->n_textures; ++i) {
        const srt_texture& t = d->textures[i];
        if (t.height <= 0 || t.width <= 0 || t.channels < 3 || t.channel0 < 0 || t.channel0 + 3 > t.channels ||
            t.idx_h <= 0 || t.idx_w <= 0 || t.offset < 0 ||
            t.offset + (int64_t)t.height * t.width * t.channels > d->texel_bytes)
            return fail(SRT_ERR_ARG, "texture record out of the texel pool");
    }
    for (int i = 0; i < d->n_materials; ++i) {
        const srt_material& m = d->materials[i];
        if (m.type == SRT_GLOSSY && !d->glossy_f0) return fail(SRT_ERR_ARG, "glossy_f0 table is null");
        int texs[4] = {m.tex, m.tex_aux0, m.tex_aux1, m.normalmap};
        for (int t : texs)
            if (t >= d->n_textures) return fail(SRT_ERR_ARG, "material texture index out of range");
        if (m.type == SRT_REFRACTIVE && (m.medium < 0 || m.medium >= d->n_media))
            return fail(SRT_ERR_ARG, "refractive medium out of range");
        if ((m.type == SRT_SKY && m.tex < 0) || (m.type == SRT_THINFILM && (m.tex_aux0 < 0 || m.tex_aux1 < 0)))
            return fail(SRT_ERR_ARG, "material is missing a required texture");
        if (m.type == SRT_DIFFUSE && (m.ival < 1 || m.ival > 255)) return fail(SRT_ERR_ARG, "diffuse_rays must be 1..255");
        if ((m.flags & SRT_MF_HIT_ALBEDO) &&
            ((m.type != SRT_GLOSSY && m.type != SRT_DIFFUSE && m.type != SRT_EMISSIVE) || m.tex >= 0))
            return fail(SRT_ERR_ARG, "SRT_MF_HIT_ALBEDO: a Glossy / Diffuse / Emissive material with tex = -1");
    }
    for (int i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type < SRT_LIGHT_DIRECTIONAL || d->lights[i].type > SRT_LIGHT_POSITIONAL)
            return fail(SRT_ERR_ARG, "bad light type");
    // the per-hit-input shaders (srt_shade_level_inputs) have no positional-light instantiation
    bool positional = false, inputs = false;
    for (int i = 0; i < d->n_lights; ++i) {
        positional |= d->lights[i].type == SRT_LIGHT_POSITIONAL;
        inputs |= d->lights[i].type == SRT_LIGHT_USER;
    }
    for (int i = 0; i < d->n_materials; ++i) inputs |= (d->materials[i].flags & SRT_MF_HIT_ALBEDO) != 0;
    if (positional && inputs)
        return fail(SRT_ERR_ARG, "an SRT_LIGHT_POSITIONAL light in a scene shaded with per-hit inputs "
                                 "(SRT_MF_HIT_ALBEDO material or SRT_LIGHT_USER light) is not supported");
    // ... and no kernel variant holds both the positional lights and the per-vertex triangle attributes
    if (positional)
        for (int i = 0; i < d->n_colliders; ++i)
            if (d->colliders[i].type == SRT_TRIANGLE && (d->colliders[i].flags & (SRT_CF_VNORMAL | SRT_CF_VUV)))
                return fail(SRT_ERR_ARG, "an SRT_LIGHT_POSITIONAL light in a scene with SRT_CF_VNORMAL / SRT_CF_VUV "
                                         "triangles (a smooth or textured mesh) is not supported");
    return SRT_OK;
}

// 2. the texel pool in HBM: 3-channel images as 4-byte texels (RGBX), so that a texel is one aligned
// dword load (texel_rgb) instead of three byte loads; the records point into that layout
struct TexelPool {
    std::vector<srt_texture> tex;              // the texture records, their offsets in the pool's layout
    std::vector<std::array<int64_t, 4>> imgs;  // (offset, bytes, new offset, expand) per image
    bool rgbx = false;                         // repacked (else the caller's pool as given)
    int64_t bytes = 0;
    uint64_t layout = 0;  // hash of the layout
};

// the pool's layout (no HIP call); `host_texels`: the caller's texels can be repacked on the host
static TexelPool plan_texel_pool(const srt_scene_desc* d, bool host_texels) {
    TexelPool tp;
    tp.tex.assign(d->textures, d->textures + std::max(0, d->n_textures));
    auto& imgs = tp.imgs;
    bool rgbx = host_texels;
    if (rgbx) {
        for (const srt_texture& t : tp.tex) {
            const int64_t bytes = (int64_t)t.height * t.width * t.channels;
            bool seen = false;
            for (auto& im : imgs)
                if (im[0] == t.offset) {
                    seen = true;
                    rgbx = rgbx && im[1] == bytes;  // (one image per offset, else the pool stays as given)
                }
            if (!seen) imgs.push_back({t.offset, bytes, 0, t.channels == 3 ? 1 : 0});
        }
        std::sort(imgs.begin(), imgs.end());
        for (size_t k = 1; k < imgs.size(); ++k) rgbx = rgbx && imgs[k][0] >= imgs[k - 1][0] + imgs[k - 1][1];
    }
    tp.bytes = d->texel_bytes;
    if (rgbx) {
        tp.bytes = 0;
        for (auto& im : imgs) {
            im[2] = tp.bytes;
            tp.bytes += ((im[3] ? im[1] / 3 * 4 : im[1]) + 3) / 4 * 4;
        }
        for (srt_texture& t : tp.tex)
            for (auto& im : imgs)
                if (im[0] == t.offset) {
                    t.offset = im[2];
                    if (im[3]) t.channels = 4;
                }
    }
    tp.rgbx = rgbx;
    // the pool's layout: the images (caller offset, bytes, pool offset, expanded) it holds, or the
    // caller's pool as given -- a key reused with another image set must not reuse the pool
    uint64_t layout = 1469598103934665603ull;
    auto mix = [&layout](int64_t v) { layout = (layout ^ (uint64_t)v) * 1099511628211ull; };
    mix(tp.bytes);
    mix(rgbx);
    if (rgbx)
        for (const auto& im : imgs)
            for (int64_t v : im) mix(v);
    tp.layout = layout;
    return tp;
}

// the caller's texels in the planned layout (host memory)
static std::vector<uint8_t> pack_texel_pool(const srt_scene_desc* d, const TexelPool& tp) {
    std::vector<uint8_t> h((size_t)tp.bytes, 0);
    for (const auto& im : tp.imgs) {
        const uint8_t* src = d->texels + im[0];
        uint8_t* dst = h.data() + im[2];
        if (im[3]) {
            for (int64_t i = 0, n = im[1] / 3; i < n; ++i) memcpy(dst + 4 * i, src + 3 * i, 3);
        } else {
            memcpy(dst, src, (size_t)im[1]);
        }
    }
    return h;
}

// the pool on the device: kept in HBM across uploads while the caller's key and size and the layout
// are unchanged (it is no scene buffer), else packed and copied
static int upload_texel_pool(srt_ctx* c, const srt_scene_desc* d, const TexelPool& tp) {
    if (d->texel_key != 0 && d->texel_key == c->texel_key && d->texel_bytes == c->texel_bytes && c->texels &&
        tp.rgbx == c->texels_rgbx && tp.layout == c->texel_layout)
        return SRT_OK;
    (void)c->texels.reset();
    c->texel_key = 0;
    c->texel_bytes = 0;
    if (d->texel_bytes <= 0 || !d->texels) return SRT_OK;
    HIP_TRY(dalloc(&c->texels, tp.bytes));
    if (tp.rgbx)
        HIP_TRY(hipMemcpy(c->texels, pack_texel_pool(d, tp).data(), (size_t)tp.bytes, hipMemcpyHostToDevice));
    else
        HIP_TRY(hipMemcpy(c->texels, d->texels, (size_t)d->texel_bytes, hipMemcpyDefault));
    c->texel_key = d->texel_key;
    c->texel_bytes = d->texel_bytes;
    c->texels_rgbx = tp.rgbx;
    c->texel_layout = tp.layout;
    return SRT_OK;
}

// 3. the scene's tables and the BVH over its Triangle colliders into scene_bufs, the texel pool (step 2)
// planned and uploaded between them; `S` receives the view the kernels read, `lin_tri` whether a
// Triangle stays outside the BVH
static int upload_tables(srt_ctx* c, const srt_scene_desc* d, SceneView& S, bool& lin_tri) {
    int rc;
    srt_collider* col;
    srt_material* mat;
    srt_texture* tex;
    srt_light* lights;
    double *media, *f0, *ll, *imp;
    if ((rc = upload(c, d->colliders, d->n_colliders, &col))) return rc;
    if ((rc = upload(c, d->materials, d->n_materials, &mat))) return rc;
    const TexelPool tp = plan_texel_pool(d, d->texel_bytes > 0 && d->texels && !is_device_ptr(d->texels));
    if ((rc = upload(c, tp.tex.data(), d->n_textures, &tex))) return rc;
    if ((rc = upload_texel_pool(c, d, tp))) return rc;
    // the light table in the kernels' layout (rt_device.h DevLight: the common fields, then the
    // positional lights' extension rows; the table's bytes in all)
    std::vector<srt_light> packed((size_t)std::max(0, d->n_lights));
    if (d->n_lights > 0) pack_lights(d->lights, d->n_lights, packed.data());
    if ((rc = upload(c, packed.data(), d->n_lights, &lights))) return rc;
    if ((rc = upload(c, d->media, (int64_t)d->n_media * 6, &media))) return rc;
    if ((rc = upload(c, d->glossy_f0, (int64_t)d->n_materials * d->n_media * 3, &f0))) return rc;
    if ((rc = upload(c, d->light_local, (int64_t)d->n_lights * d->n_colliders * 3, &ll))) return rc;
    if ((rc = upload(c, d->importance, (int64_t)d->n_importance * 4, &imp))) return rc;
    // (casts: in the device compilation the SceneView fields are constant-address-space pointers)
    S.col = (decltype(S.col))col; S.mat = (decltype(S.mat))mat; S.tex = (decltype(S.tex))tex;
    S.texels = (decltype(S.texels))c->texels.p; S.lights = (decltype(S.lights))lights;
    S.media = (decltype(S.media))media; S.glossy_f0 = (decltype(S.glossy_f0))f0;
    S.light_local = (decltype(S.light_local))ll; S.importance = (decltype(S.importance))imp;
    S.ncol = d->n_colliders; S.nmat = d->n_materials; S.ntex = d->n_textures; S.nlights = d->n_lights;
    S.nmedia = d->n_media; S.nimp = d->n_importance;
    S.sky_col = sky_collider(d->colliders, d->n_colliders, d->materials);
    // triangle meshes: BVH over the Triangle colliders, the rest intersected one by one
    BvhBuild B;
    if (c->use_bvh) {
        bvh_build(d->colliders, d->n_colliders, B);
    } else {
        for (int i = 0; i < d->n_colliders; ++i) B.lin.push_back(i);
    }
    int32_t *lin, *tri;
    BvhNode* nodes;
    if ((rc = upload(c, B.lin.data(), (int64_t)B.lin.size(), &lin))) return rc;
    if ((rc = upload(c, B.tri.data(), (int64_t)B.tri.size(), &tri))) return rc;
    if ((rc = upload(c, B.nodes.data(), (int64_t)B.nodes.size(), &nodes))) return rc;
    S.nlin = (int)B.lin.size();
    S.lin = (decltype(S.lin))lin;
    S.bvh_tri = (decltype(S.bvh_tri))tri;
    S.bvh = (decltype(S.bvh))nodes;
    S.bvh_nodes = (int)B.nodes.size();
    S.bvh_bound = B.bound;
    lin_tri = false;
    for (int k : B.lin) lin_tri |= d->colliders[k].type == SRT_TRIANGLE;
    S.nshadow = 0;
    for (int i = 0; i < d->n_colliders; ++i)
        if (d->colliders[i].flags & SRT_CF_SHADOW) S.nshadow++;
    for (int k = 0; k < 3; ++k) S.ambient[k] = d->ambient[k];
    S.lut_lds = nullptr;
    S.nlut_lds = std::min(d->n_textures, MAX_LUT_LDS);
    return SRT_OK;
}

// 4. what the context keeps of the scene besides its view: depth and fan-out, the materials present
// (the kernel variant), the collider sequence, who needs per-hit inputs
static void derive_scene_facts(srt_ctx* c, const srt_scene_desc* d, const SceneView& S, bool lin_tri) {
    int fan = 1;
    c->has_diffuse = 0;
    for (int i = 0; i < d->n_materials; ++i) {
        const srt_material& m = d->materials[i];
        if (m.type == SRT_REFRACTIVE || m.type == SRT_THINFILM) fan = std::max(fan, 2);
        if (m.type == SRT_DIFFUSE) { fan = std::max(fan, std::max(1, (int)m.ival)); c->has_diffuse = 1; }
    }
    c->S = S;
    c->max_depth = std::max(0, (int)d->max_ray_depth);
    c->fanout = fan;
    c->mats = 0;
    for (int i = 0; i < d->n_materials; ++i) c->mats |= mat_bit(d->materials[i].type);
    if (S.bvh_nodes > 0) c->mats |= MAT_BVH | MAT_TRI;  // (a tied ray re-tests its colliders, triangles too)
    if (lin_tri) c->mats |= MAT_TRI;  // Triangle colliders outside the BVH
    for (int i = 0; i < d->n_materials; ++i)
        if (d->materials[i].normalmap >= 0) c->mats |= MAT_NMAP;
    for (int i = 0; i < d->n_colliders; ++i)
        if (d->colliders[i].type == SRT_TRIANGLE && (d->colliders[i].flags & (SRT_CF_VNORMAL | SRT_CF_VUV)))
            c->mats |= MAT_VATTR;
    for (int i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type == SRT_LIGHT_POSITIONAL) c->mats |= MAT_PLIGHT;
    c->seq = 0;
    if (S.bvh_nodes == 0 && d->n_colliders <= SEQ_MAX) {
        int types[SEQ_MAX];
        for (int i = 0; i < d->n_colliders; ++i) types[i] = d->colliders[i].type;
        c->seq = seq_encode(types, d->n_colliders);
    }
    c->col_hit_albedo.assign((size_t)std::max(0, d->n_colliders), 0);
    c->n_user_lights = 0;
    c->needs_inputs = false;
    for (int i = 0; i < d->n_colliders; ++i)
        if (d->materials[d->colliders[i].material].flags & SRT_MF_HIT_ALBEDO) c->col_hit_albedo[i] = 1;
    for (int i = 0; i < d->n_materials; ++i)
        if (d->materials[i].flags & SRT_MF_HIT_ALBEDO) c->needs_inputs = true;
    for (int i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type == SRT_LIGHT_USER) c->n_user_lights++;
    if (c->n_user_lights > 0) c->needs_inputs = true;
    c->chain_ok = true;
    c->hint_key[0] = -1;  // ray counts of another scene are no plan for this one
    c->fx_ok = true;
}

int srt_upload_scene(srt_ctx* c, const srt_scene_desc* d) {
    if (!c || !d) return fail(SRT_ERR_ARG, "null ctx/scene");
    int rc;
    if ((rc = check_scene_desc(d))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = finish_async(c, nullptr))) return rc;  // frames in flight read the scene tables freed below
    HIP_TRY(hipStreamSynchronize(c->f->stream));
    c->scene_bufs.clear();
    c->has_scene = false;
    SceneView S{};
    bool lin_tri = false;
    if ((rc = upload_tables(c, d, S, lin_tri))) return rc;
    derive_scene_facts(c, d, S, lin_tri);
    c->has_scene = true;
    return SRT_OK;
}


}  // extern "C"
#include "rt_render.h"  // render_impl: srt_render and srt_render_prefetch

extern "C" {
int srt_render(srt_ctx* c, const srt_camera* cam, const srt_render_args* a, srt_stats* st) {
    return render_impl(c, cam, a, st, false);
}

int srt_render_prefetch(srt_ctx* c, const srt_camera* cam, const srt_render_args* a) {
    return render_impl(c, cam, a, nullptr, true);
}

int srt_render_finish(srt_ctx* c, srt_stats* st) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    return finish_async(c, st);
}

int srt_stream(srt_ctx* c, void** stream) {
    if (!c || !stream) return fail(SRT_ERR_ARG, "null argument");
    *stream = (void*)c->f->stream;
    return SRT_OK;
}

}  // extern "C"

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

#include "rt_api_entry.h"
#include "rt_api_group.h"
#include "rt_api_misc.h"
