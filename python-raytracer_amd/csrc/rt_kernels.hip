// rt_kernels.hip -- gfx950 ray tracer behind the C ABI of include/sightpy_rt.h: the one translation
// unit of libsightpy_hip.so.  The device code, the owners of device memory, the host side of srt_render
// and most entry points are fragments of this unit, included in place (source map, in order):
//   rt_trace_common.h   fail / HIP_TRY, Queue, TraceParams, key_pix, the fixed-point sums, PixAcc, GpuEmit
//   rt_trace_kernels.h  trace_one, ChainEmit, FusedEmit, k_primary, k_primary_lean, k_trace, k_shade_forced*
//   rt_frame_kernel.h   FrameLds, FrameEmit, FrameEmitFx, k_frame
//   rt_variants.h       MATS_*, Variant, VARIANTS, SEQ_VARIANTS, pick_variant
//   rt_aux_kernels.h    k_pass_end, k_resolve, the API kernels, k_assemble, k_rgbx, k_seed_queue, k_gather_children
//   rt_devmem.h         DevBuf / DevList, dalloc, grid_for
//   (rt_pose.h, with the headers above: pose_triangle_record, k_pose_triangles, k_bvh_refit)
//   (rt_deform.h, likewise: deform_triangle_record, k_deform_face_cross / _vertex_normals / _triangles)
//   (this file)         the context and its frame slots, the MT host side, frame collection and gather,
//                       srt_create and the options, scene upload
//   rt_render.h         render_impl, before srt_render and its siblings
//   rt_api_trace.h      trace_impl, srt_trace and srt_shade*
//   rt_api_entry.h      the single-kernel entry points, AOVs and denoise, device memory, srt_mt19937_uniforms
//   rt_api_anim.h       srt_pose_colliders, srt_deform_topology, srt_deform_colliders over srt_ctx::mesh
//   rt_api_group.h      communicators, srt_render_group*, allreduce, barrier
//   rt_api_misc.h       host memory, the srt_debug_* hooks, srt_synchronize
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
#include "rt_pose.h"
#include "rt_deform.h"

using namespace rt;
using namespace rtmt_dev;

#include "rt_trace_common.h"

#include "rt_trace_kernels.h"
#include "rt_frame_kernel.h"
#include "rt_variants.h"
#include "rt_aux_kernels.h"
#include "rt_devmem.h"

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

// Times of the N stages of an entry point's last call, between events on its stream (srt_debug_*_times), and how
// many calls completed.  The events are made at their first mark and destroyed by ~srt_ctx.
template <int N>
struct StageTimer {
    hipEvent_t ev[N + 1] = {};
    double ms[N] = {};
    int64_t calls = 0;
    hipError_t mark(int k, hipStream_t st) {
        if (!ev[k])
            if (const hipError_t e = hipEventCreate(&ev[k])) return e;
        return hipEventRecord(ev[k], st);
    }
    // after the stream is synchronised
    hipError_t collect() {
        for (int k = 0; k < N; ++k) {
            float v = 0.0f;
            if (const hipError_t e = hipEventElapsedTime(&v, ev[k], ev[k + 1])) return e;
            ms[k] = v;
        }
        calls++;
        return hipSuccess;
    }
};

// A mesh registered by srt_deform_topology: `P` is DeformMesh::P for the copy in, `normals` whether any corner's
// normal is recomputed
struct DeformTopo {
    DeformMesh m;
    double* P = nullptr;
    bool normals = false;
};

// The state of the animated triangle meshes (srt_pose_colliders, srt_deform_topology, srt_deform_colliders:
// rt_api_anim.h, rt_pose.h, rt_deform.h).  Everything here belongs to the resident scene and starts afresh with an
// upload (reset), except what reset() names.
//   in scene_bufs (released with the scene): the collider table the kernels read (S.col) and its copy in the
//     rest pose (as uploaded, or as last deformed), the BVH's nodes and leaf slots as plain pointers, the nodes
//     grouped by height (rt_bvh.h BvhLevels), the registered meshes' tables and vertex arrays (allocated after
//     every table of the upload)
//   on the host: the rest table, the groups' offsets, the rest shape's bvh_bound, what the last pose call derived
//     from its ranges alone, whether it left a range in another pose than the identity
//   of the context: the pose call's range table and the two calls' stage timers
struct MeshTables {
    srt_collider* col_live = nullptr;
    srt_collider* col_rest = nullptr;
    BvhNode* bvh_dev = nullptr;
    int32_t* bvh_tri_dev = nullptr;
    int32_t* bvh_level_nodes = nullptr;
    int bvh_ntri = 0;
    std::vector<int32_t> bvh_level_offset;
    std::vector<srt_collider> col_host;
    float bvh_bound_rest = 0.0f;
    PoseLayout pose_layout;
    bool pose_active = false;
    std::vector<DeformTopo> deform_meshes;
    DevBuf<PoseRange> pose_ranges;
    StageTimer<2> pose_timer;    // k_pose_triangles, the refit
    StageTimer<3> deform_timer;  // the normals, the records, the refit
    void reset() {
        MeshTables fresh;
        fresh.pose_ranges = std::move(pose_ranges);
        fresh.pose_timer = pose_timer;
        fresh.deform_timer = deform_timer;
        *this = std::move(fresh);
    }
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
    MeshTables mesh;  // what srt_pose_colliders / srt_deform_* rewrite of the scene (rt_api_anim.h)
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
    for (hipEvent_t e : mesh.pose_timer.ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : mesh.deform_timer.ev)
        if (e) (void)hipEventDestroy(e);
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
    c->mesh.col_live = col;
    c->mesh.col_host.assign(d->colliders, d->colliders + std::max(0, d->n_colliders));
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
    // what srt_pose_colliders (rt_api_anim.h) needs, after every table the trace kernels read (whose allocations, and so
    // addresses, stay what they were without it): the rest pose's copy of the collider table, the refit order
    if ((rc = upload(c, d->colliders, d->n_colliders, &c->mesh.col_rest))) return rc;
    BvhLevels lv;
    bvh_levels(B.nodes, lv);
    if ((rc = upload(c, lv.nodes.data(), (int64_t)lv.nodes.size(), &c->mesh.bvh_level_nodes))) return rc;
    c->mesh.bvh_level_offset = lv.offset;
    c->mesh.bvh_dev = nodes;
    c->mesh.bvh_tri_dev = tri;
    c->mesh.bvh_ntri = (int)B.tri.size();
    c->mesh.bvh_bound_rest = B.bound;
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
    c->mesh.reset();
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

#include "rt_api_trace.h"
#include "rt_api_entry.h"
#include "rt_api_anim.h"
#include "rt_api_group.h"
#include "rt_api_misc.h"
