// rt_aux_kernels.h -- the small kernels around the trace paths.  Ends of a pass and of a frame: k_pass_end,
// k_resolve, k_fx_combine, k_fb_groups.  One per single-kernel entry point: k_nearest, k_intersect_one,
// k_collider_surface, k_material_normal, k_texture_lookup, k_primary_rays.  Row-band shards: MAX_RANKS,
// GatherTiles, k_assemble.  k_rgbx.  For srt_trace and the shade levels: k_seed_queue, k_gather_children.
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: rt_trace_common.h
// (the queue, the fixed-point sums, the primary uniforms) and rt_trace_kernels.h (store_u8_chunk).
namespace {

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
