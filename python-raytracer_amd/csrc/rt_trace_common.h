// rt_trace_common.h -- what every trace kernel shares: the error helpers (fail, HIP_TRY), the block and
// shard constants, the ray queue (Queue, queue_load / queue_store), the kernels' argument block
// (TraceParams, HitPtrs), key_pix, the order-independent fixed-point sums (fx_*, fb_add), wave_reserve,
// PixAcc, the wavefront emitter GpuEmit, and the primary uniforms and jitter.
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: the system and
// project includes of rt_kernels.hip (rt_device.h above all) and its two `using` lines.
namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(SRT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)

constexpr int BLOCK = 256;
#ifndef RT_NSHARD
#define RT_NSHARD 256
#endif
// queue shards, one append counter each: blocks b, b + NSHARD, ... share one.  Appends are
// device-scope atomics executed at the memory side; with 16 counters their serialisation cost the
// depth-0 kernel ~40 % (1.39 vs 0.87 ms, ex1 1080p), 64-256 counters remove it.
constexpr int NSHARD = RT_NSHARD;
constexpr size_t TRACE_PARAMS_BYTES = 864;
constexpr int MAX_LUT_LDS = 12;  // texture tables staged in LDS per block (2 KiB each)
// retry bits of flags[1]: a queue shard / ring overflowed (re-render with bigger queues); a tie gave
// a chained ray a second child (re-render without chain mode)
constexpr uint32_t RETRY_OVERFLOW = 1u;
constexpr uint32_t RETRY_CHAIN_TIE = 2u;
constexpr uint32_t RETRY_FIXED_RANGE = 4u;  // a contribution beyond the fixed-point range (fx_add)

struct Queue {
    double *ox, *oy, *oz, *dx, *dy, *dz, *wr, *wg, *wb;
    uint32_t *pix, *meta, *path;
};
constexpr int64_t RAY_BYTES = 9 * 8 + 3 * 4;  // 84 B per queued ray

struct TraceParams {
    SceneView S;
    Queue qin, qout;
    const uint32_t* cnt_in;  // [NSHARD] rays per input shard (depth d)
    uint32_t* cnt_out;       // [NSHARD] append counters of the output shards (depth d+1)
    uint32_t* flags;         // [0] error bits, [1] overflow
    unsigned long long* shadow;
    double* fb;              // [3][npix] depth-0 colour (stored by the pixel's own thread)
    unsigned long long* fbx; // [3][npix] fixed-point sums of every added contribution (fb_add), or null:
                             // f64 atomics into fb (option "deterministic" 0, order-dependent rounding)
    int64_t npix;
    int64_t seg;             // capacity of one queue shard (rays)
    uint64_t seed;
    int depth;
    int fb_first;  // depth 0 of the first pass: store the pixel instead of adding (no memset)
    // primary generation
    int64_t n_primary;
    srt_camera cam;
    const int32_t* rows;
    const double* jitter;  // [spp][4][jit_plane] (device) or null
    int64_t jit_plane;     // doubles per jitter plane: npix, or width*height when jit_global
    int jit_global;        // 1: jitter indexed by the global pixel (the whole frame's numpy stream)
    int sample_base;
    int spp;           // samples of this pass (k_primary)
    int pix_groups;    // k_primary: sample groups per pixel (a power of two <= 64; lanes of one wave)
    int chain;         // k_trace: trace each ray's whole (single-child) chain in-thread, see k_trace
    int32_t* hit_out;  // [spp][npix] or null
    // frame kernel (k_frame): per-wave ray rings in HBM, slot s = rays [s * ring_cap, (s+1) * ring_cap)
    Queue ring;
    uint32_t* ring_lock;  // [nslot] 0 = free, 1 = owned by a running wave
    int64_t ring_cap;     // rays per ring (power of two)
    double* out_rgb;      // fused resolve (single-pass frames): [3][npix] linear RGB or null
    uint8_t* out_u8;      //                                     [npix][3] sRGB8 or null
    int nslot;
    int dcap;             // deepest depth traced; deeper children are counted and dropped
    int fuse_resolve;     // 1: k_frame resolves its pixels (no framebuffer); 0: adds to fb
    int spp_total;        // samples of the frame (resolve average)
    // k_shade_forced (srt_shade, Material.get_color): the first depth's hit per ray (index = pix)
    const int32_t* force_id;
    const double* force_t;
    const double* force_o;
    // k_frame sample groups: block b takes tile b % ntiles and the samples [g spg, (g+1) spg) of the
    // pass, g = b / ntiles; groups > 1 store their partial sums to fbg[g][3][npix] (k_fb_groups adds them)
    double* fbg;
    int groups;
    int ntiles;
    // srt_debug_lane_stats: [depth][2] u64 = (wave iterations that traced the depth, live lanes in
    // them) of the fused paths' depth loop, or null (counting off)
    unsigned long long* lane_stats;
};
// k_shade_forced_inputs (srt_shade_level_inputs): what the user's texture / Light methods returned per
// ray (index = pix, batch of npix), or null.  A kernel argument of its own: the kernels that take
// TraceParams alone keep their argument block (several copy it to scratch: 24 bytes more there grew
// their scratch size).
struct HitPtrs {
    const double* albedo;  // [3][npix]
    const double* ldist;   // [user lights][npix]
    const double* lirr;    // [user lights][3][npix]
};
// kernel argument: host and device passes must agree on the layout (catches address-space pointer
// size differences, see SceneView)
static_assert(sizeof(TraceParams) == TRACE_PARAMS_BYTES, "TraceParams layout");

// Pixel identity that keys the Monte-Carlo draws: the global pixel row * width + col of the frame
// (`pix` indexes the rows this call renders), so that an image sharded over any number of GPUs draws
// the same numbers as the single-GPU render; srt_trace (no rows) keys by the ray's batch index.
__device__ __forceinline__ uint32_t key_pix(const TraceParams& P, uint32_t pix) {
    if (!P.rows) return pix;
    const uint32_t W = (uint32_t)P.cam.width;
    const uint32_t lr = pix / W;
    return (uint32_t)P.rows[lr] * W + (pix - lr * W);
}

__device__ __forceinline__ void queue_store(const Queue& q, int64_t i, d3 o, d3 d, d3 w, uint32_t pix,
                                            uint32_t meta, uint32_t path) {
    q.ox[i] = o.x; q.oy[i] = o.y; q.oz[i] = o.z;
    q.dx[i] = d.x; q.dy[i] = d.y; q.dz[i] = d.z;
    q.wr[i] = w.x; q.wg[i] = w.y; q.wb[i] = w.z;
    q.pix[i] = pix; q.meta[i] = meta; q.path[i] = path;
}

__device__ __forceinline__ Ray queue_load(const Queue& q, int64_t i) {
    Ray r;
    r.o = d3{q.ox[i], q.oy[i], q.oz[i]};
    r.d = d3{q.dx[i], q.dy[i], q.dz[i]};
    r.w = d3{q.wr[i], q.wg[i], q.wb[i]};
    r.pix = q.pix[i]; r.meta = q.meta[i]; r.path = q.path[i];
    return r;
}

// Contributions added to a pixel by other threads (depth >= 1, split samples) go into an
// order-independent fixed-point sum, so a frame is bit-reproducible (the reference is
// deterministic; f64 atomics are not, their rounding depends on arrival order): each contribution
// rounded to a multiple of 2^-FX_BITS and summed with one int64 atomic per channel (the count of f64
// atomics it replaces); the resolve adds sum 2^-FX_BITS to the depth-0 colour.  Rounding error
// <= 2^-45 = 2.8e-14 per contribution; a contribution of magnitude >= 2^17 (sums up to 2^19 stay in
// range) raises RETRY_FIXED_RANGE and the frame is rendered again with f64 atomics.
constexpr int FX_BITS = 44;
constexpr double FX_SCALE = (double)(1ull << FX_BITS);
constexpr double FX_UNIT = 1.0 / FX_SCALE;
constexpr double FX_MAX = 131072.0;                 // 2^17

// Range of the sums: a pixel-channel sum wraps only beyond 2^20 (2^64 scaled).  Besides the three
// sums, every pixel keeps a coarse magnitude -- the f32 sum of |r| + |g| + |b| of its terms, one
// more fire-and-forget atomic (fx_mag, behind the sums in the same buffer) -- and the resolve
// distrusts a pixel whose magnitude reached FX_MAG_LIMIT (2^16; f32 rounding keeps it within a factor
// 1 + n 2^-24 of the true magnitude, so no sum of fewer than 2^23 terms gets near 2^20 unseen).
// A returning atomic per term (checking each partial sum) cost 6.6 % of the device frame.
constexpr float FX_MAG_LIMIT = 65536.0f;
RT_HD int64_t fx_words(int64_t npix) { return 3 * npix + (npix + 1) / 2; }  // u64 words of fbx
__device__ __forceinline__ float* fx_mag(unsigned long long* fbx, int64_t npix) {
    return reinterpret_cast<float*>(fbx + 3 * npix);
}
__device__ __forceinline__ const float* fx_mag(const unsigned long long* fbx, int64_t npix) {
    return reinterpret_cast<const float*>(fbx + 3 * npix);
}

__device__ __forceinline__ bool fx_add(unsigned long long* acc, double v) {
    if (!(fabs(v) < FX_MAX)) return false;  // (also NaN)
    atomicAdd(acc, (unsigned long long)__double2ll_rn(v * FX_SCALE));
    return true;
}

__device__ __forceinline__ void fb_add(double* fb, unsigned long long* fbx, uint32_t* flags, int64_t npix,
                                       uint32_t pix, d3 w, d3 c) {
    if (is_zero(c)) return;  // adding an exact zero is a no-op
#ifdef RT_ABL_FB  // diagnostic build only: no framebuffer atomics
    if (w.x * c.x == 12345.678) fb[pix] = 0.0;
    return;
#endif
    if (fbx) {
        // all three channels added (no short-circuit), then one range check
        const double tx = w.x * c.x, ty = w.y * c.y, tz = w.z * c.z;
        const int ok = (int)fx_add(fbx + pix, tx) & (int)fx_add(fbx + npix + pix, ty) & (int)fx_add(fbx + 2 * npix + pix, tz);
        if (!ok) atomicOr(flags + 1, RETRY_FIXED_RANGE);
        unsafeAtomicAdd(fx_mag(fbx, npix) + pix, (float)((fabs(tx) + fabs(ty)) + fabs(tz)));
    } else {
        unsafeAtomicAdd(fb + pix, w.x * c.x);
        unsafeAtomicAdd(fb + npix + pix, w.y * c.y);
        unsafeAtomicAdd(fb + 2 * npix + pix, w.z * c.z);
    }
}

__device__ __forceinline__ double fx_value(const unsigned long long* fbx, int64_t npix, int ch, int64_t p) {
    return (double)(long long)fbx[ch * npix + p] * FX_UNIT;
}

// a pixel the resolve must not trust: its coarse magnitude reached FX_MAG_LIMIT (or is NaN), or a
// channel sum lies in [2^61, 2^64) scaled (>= 2^17 in colour units; negative = wrapped)
__device__ __forceinline__ bool fx_suspect(const unsigned long long* fbx, int64_t npix, int64_t p) {
    bool bad = !(fx_mag(fbx, npix)[p] < FX_MAG_LIMIT);
    for (int ch = 0; ch < 3; ++ch) bad |= (fbx[ch * npix + p] >> 61) != 0;
    return bad;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Reserve `cnt` consecutive slots of the output shard for every active lane: one atomic per wave.
// The exclusive prefix of the (small) per-lane counts is assembled from one ballot per bit, which
// is exact in divergent code (inactive lanes contribute nothing).
__device__ __forceinline__ uint32_t wave_reserve(uint32_t* ctr, uint32_t cnt) {
    uint32_t total = 0, below = 0;
    uint64_t any = __ballot(cnt != 0);
    if (!any) return 0;
    for (int b = 0; b < 8; ++b) {
        uint64_t m = __ballot((cnt >> b) & 1u);
        total += (uint32_t)__builtin_popcountll(m) << b;
        below += lanes_below(m) << b;
    }
    uint32_t base = 0;
#ifdef RT_ABL_NOATOMIC  // diagnostic build only: no counter traffic at all
    return below + (total & 0u);
#endif
#ifdef RT_ABL_APPEND  // diagnostic build only: counts kept, slots not waited for (wrong images)
    if (lanes_below(__ballot(1)) == 0) atomicAdd(ctr, total);
    return ((blockIdx.x * 256u + threadIdx.x) * 2u + below % 2u) % 400000u;
#endif
    if (lanes_below(__ballot(1)) == 0) base = atomicAdd(ctr, total);  // first active lane
    base = __builtin_amdgcn_readfirstlane(base);
    return base + below;
}

// the exclusive prefix of `cnt` over the active lanes below this one (wave_reserve's `below`)
__device__ __forceinline__ uint32_t wave_below(uint32_t cnt) {
    uint32_t below = 0;
    for (int b = 0; b < 8; ++b) below += lanes_below(__ballot((cnt >> b) & 1u)) << b;
    return below;
}

// A pixel's colour summed in the thread that traces (some of) its samples, in one of two forms
// sharing the same registers:
//  * fixed point (P.fbx set, the default): every term -- depth 0 included -- rounded to a multiple of
//    2^-FX_BITS and summed as an integer (unsigned: wrapping is defined), exactly fb_add's terms, plus
//    fb_add's coarse magnitude (the f32 sum of |r| + |g| + |b| of the terms, independent of the sums).
//    Integer sums do not depend on the order or grouping of the terms, so a pixel's samples may be
//    split over any number of threads (sample groups, k_primary) or GPUs and the totals are the same
//    bits.  A term of magnitude >= 2^17 (or NaN) is left out of the sums and shows in the magnitude
//    (>= FX_MAG_LIMIT or NaN): the frame is then rendered again in f64.
//  * f64 (option deterministic 0, or that fallback): the f64 sums, in the words' bits.
struct PixAcc {
    unsigned long long w[3] = {0ull, 0ull, 0ull};
    float mag = 0.0f;

    __device__ __forceinline__ void add(bool fx, d3 t) {
        if (fx) {
            const double m = (fabs(t.x) + fabs(t.y)) + fabs(t.z);
            if (m < FX_MAX) {  // every |term| < 2^17: the conversions are in range (NaN fails too)
                w[0] += (unsigned long long)__double2ll_rn(t.x * FX_SCALE);
                w[1] += (unsigned long long)__double2ll_rn(t.y * FX_SCALE);
                w[2] += (unsigned long long)__double2ll_rn(t.z * FX_SCALE);
            }
            mag += (float)m;
        } else {
            w[0] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)w[0]) + t.x);
            w[1] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)w[1]) + t.y);
            w[2] = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)w[2]) + t.z);
        }
    }
    __device__ __forceinline__ double value(bool fx, int k) const {
        return fx ? (double)(long long)w[k] * FX_UNIT : __longlong_as_double((long long)w[k]);
    }
    // the pixel's fixed-point totals the resolve must not trust (fx_suspect's rule)
    __device__ __forceinline__ bool suspect() const {
        return !(mag < FX_MAG_LIMIT) || ((w[0] | w[1] | w[2]) >> 61) != 0;
    }
    // sum over the lanes l ^ off, off = 32, 16, .. >= lo (the sample groups of a pixel, k_primary):
    // integer sums exactly; f64 sums pairwise, commutative, so every lane ends with the same value
    __device__ __forceinline__ void reduce_lanes(bool fx, int lo) {
        for (int off = 32; off >= lo; off >>= 1) {
            for (int k = 0; k < 3; ++k) {
                const unsigned long long o = __shfl_xor(w[k], off);
                w[k] = fx ? w[k] + o
                          : (unsigned long long)__double_as_longlong(__longlong_as_double((long long)w[k]) +
                                                                     __longlong_as_double((long long)o));
            }
            mag += __shfl_xor(mag, off);
        }
    }
};


// Emitter of the GPU trace step: colour -> framebuffer atomics, children -> output queue shard.
struct GpuEmit {
    const TraceParams& P;
    const Ray& r;
    uint32_t shard;
    uint32_t round;
    uint32_t* shadow_acc;
    PixAcc* acc;  // depth 0: the pixel's sums in the thread (no framebuffer atomics)

    __device__ void local(d3 c) const {
        if (acc) {
            if (!is_zero(c)) acc->add(P.fbx != nullptr, mul(r.w, c));
        } else {
            fb_add(P.fb, P.fbx, P.flags, P.npix, r.pix, r.w, c);
        }
    }
    __device__ void shadow(int n) const { *shadow_acc += (uint32_t)n; }
    __device__ void store(uint32_t slot, const Child& c, uint32_t path) const {
#if defined(RT_ABL_QSTORE) || defined(RT_ABL_NOATOMIC)  // diagnostic build only: no queue stores
        if (c.o.x == 12345.678) P.flags[1] = path;
        return;
#endif
        if (slot < (uint64_t)P.seg) {
            queue_store(P.qout, (int64_t)shard * P.seg + slot, c.o, c.d, mul(r.w, c.w), r.pix,
                        pack_meta(c.medium, meta_depth(r.meta) + 1, c.dfl), path);
        } else {
            atomicOr(&P.flags[1], RETRY_OVERFLOW);
        }
    }
    __device__ void child(const Child& c) const {
        uint32_t slot = wave_reserve(P.cnt_out + shard, 1u);
        store(slot, c, child_path(r.path, c.slot, round));
    }
    // the fan-out child-major: the k-th children of the wave's lanes take consecutive slots, so every
    // store of a child is one coalesced run (lane-major slots scattered each store over 64 lines)
    __device__ void diffuse(const DiffuseGen& g, int mi) const {
        const uint32_t cnt = (uint32_t)g.count;
        const uint32_t base = wave_reserve(P.cnt_out + shard, cnt) - wave_below(cnt);
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

__device__ __forceinline__ double mc_uniform(const TraceParams& P, const Ray& r, int cid, uint32_t round) {
    if (!(P.S.col[cid].flags & SRT_CF_MC)) return 0.0;
    Rng g;
    g.init(P.seed, key_pix(P, r.pix), r.path, 0x3C000000u | (meta_depth(r.meta) << 8) | round);
    return g.one();
}

// Uniforms for primary ray of sample s at local pixel p.
__device__ __forceinline__ void primary_uniforms(const TraceParams& P, int s, uint32_t p, uint32_t gpix,
                                                 double j[4]) {
    if (P.jitter) {
        const int64_t plane = P.jit_plane;
        const double* base = P.jitter + (int64_t)s * 4 * plane + (P.jit_global ? gpix : p);
        j[0] = base[0]; j[1] = base[plane];
        // the lens-disk pair is read only by a thin-lens camera (pinhole: primary_ray skips it)
        if (P.cam.lens_radius != 0.0) { j[2] = base[2 * plane]; j[3] = base[3 * plane]; }
    } else {
        Rng g;
        g.init(P.seed, gpix, (uint32_t)(P.sample_base + s), 0xCA3E0000u);
        g.two(j[0], j[1]);
        g.two(j[2], j[3]);
    }
}

// k_primary's split of primary_uniforms: the pixel-jitter pair (prefetched a sample ahead) and the
// lens-disk pair (thin-lens cameras only), the same values
__device__ __forceinline__ void primary_jitter(const TraceParams& P, int s, uint32_t p, uint32_t gpix, double j[2]) {
#ifdef RT_ABL_JIT  // diagnostic build only: no jitter loads (wrong images; timing only)
    j[0] = 0.5 + 1e-9 * (double)(s & 7);
    j[1] = 0.5;
    return;
#endif
    if (P.jitter) {
        const int64_t plane = P.jit_plane;
        const double* base = P.jitter + (int64_t)s * 4 * plane + (P.jit_global ? gpix : p);
        j[0] = base[0];
        j[1] = base[plane];
    } else {
        double j4[4];
        primary_uniforms(P, s, p, gpix, j4);
        j[0] = j4[0];
        j[1] = j4[1];
    }
}
__device__ __forceinline__ void lens_jitter(const TraceParams& P, int s, uint32_t p, uint32_t gpix, double j[4]) {
    double j4[4] = {0.0, 0.0, 0.0, 0.0};
    primary_uniforms(P, s, p, gpix, j4);
    j[2] = j4[2];
    j[3] = j4[3];
}

// an emitter whose child replaces the traced ray in place (Em::kInPlace)
template <class Em, class = void>
struct em_in_place : std::false_type {};
template <class Em>
struct em_in_place<Em, std::void_t<decltype(Em::kInPlace)>> : std::bool_constant<Em::kInPlace> {};

}  // namespace
