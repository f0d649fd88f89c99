// rt_variants.h -- which instantiations of the trace kernels the library holds, and the choice among them:
// the material sets MATS_*, Variant (one row of kernel pointers), the build-time knobs RT_OCC, RT_FUSE_OCC,
// RT_BVH_LDS_STACK and RT_MESH_FUSE_OCC, the table VARIANTS, the collider-sequence table SEQ_VARIANTS with
// seq_bits (under RT_SEQ_VARIANTS), and pick_variant.  RT_EXP_MIN keeps the headline rows only.  Host data;
// the rows instantiate the kernels, so the tables' order is the order of the device code.
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: rt_trace_kernels.h
// (k_primary, k_primary_lean, k_trace) and rt_frame_kernel.h (k_frame).
namespace {

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

}  // namespace
