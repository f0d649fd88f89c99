// rt_deform.h -- deformed triangle meshes: the collider records of a mesh, and the area-weighted vertex normals
// of a smooth one, recomputed on the device from a new vertex array (srt_deform_colliders in rt_api_anim.h; the
// CPU check harness rt_hostcheck.cpp runs the same functions).  The BVH's boxes are then refitted by rt_pose.h's
// k_bvh_refit, and the trace kernels read the rewritten tables as they read uploaded ones.
//
// A registered mesh (srt_deform_topology) is its range of the collider table, the corner table corner[3 f + k]
// (the vertex index of corner k of face f, checked on the host against n_verts), one byte per corner saying whether
// its normal is recomputed, the mesh's center, and the corners naming each vertex as a CSR list in ascending
// corner -- so ascending face -- order.  Vertex i of the array P is rendered at P[i] + center, componentwise
// (TriangleMesh's verts[i] + center).  Three steps, none with an atomic:
//   face products   (P[b] - P[a]) x (P[c] - P[a]) per face, unnormalised and without center, numpy.cross's order
//   vertex sums     per vertex, 0 plus the products of the corners naming it in list order (TriangleMesh's
//                   _vertex_normals adds a face once per corner that names the vertex, in file order)
//   records         every field from the three corners as sightpy's Triangle_Collider computes it
//                   (rt_pose.h triangle_record_geometry / _bary); a recomputed corner normal is normalize(sum), or where
//                   the sum is exactly zero normalize(the new face normal), as the constructor's substitution
//                   goes through Triangle_Collider's normalisation; the other normals, the uvs, type, flags,
//                   material and the integer fields are the rest record's
#pragma once

#include "rt_pose.h"

namespace rt {

// What the kernels need of one registered mesh (device pointers; on the host check harness, host pointers).
struct DeformMesh {
    int32_t first, count, n_verts;     // colliders [first, first + count), one per face
    const int32_t* corner;             // [3 * count]
    const uint8_t* recompute;          // [3 * count]
    const int32_t* csr_offset;         // [n_verts + 1]
    const int32_t* csr_corner;         // [3 * count]
    double center[3];
    const double* P;                   // [3 * n_verts], the current vertex array
    double* face_cross;                // [3 * count] scratch
    double* vertex_sum;                // [3 * n_verts] scratch
};

RT_HD d3 deform_vertex(const double* P, int i) { return d3{P[3 * i], P[3 * i + 1], P[3 * i + 2]}; }

// numpy.cross(P[b] - P[a], P[c] - P[a]) of face f
RT_HD void deform_face_cross(const DeformMesh& M, int f) {
    const int a = M.corner[3 * f], b = M.corner[3 * f + 1], c = M.corner[3 * f + 2];
    if (a < 0 || a >= M.n_verts || b < 0 || b >= M.n_verts || c < 0 || c >= M.n_verts) return;
    const d3 u = sub(deform_vertex(M.P, b), deform_vertex(M.P, a)), v = sub(deform_vertex(M.P, c), deform_vertex(M.P, a));
    pose_put(M.face_cross + 3 * f, d3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x});
}

// the sum over the corners naming vertex v, in list order
RT_HD void deform_vertex_sum(const DeformMesh& M, int v) {
    d3 s{0.0, 0.0, 0.0};
    const int begin = M.csr_offset[v], end = M.csr_offset[v + 1];
    if (begin < 0 || end > 3 * M.count) return;
    for (int j = begin; j < end; ++j) {
        const int corner = M.csr_corner[j];
        if (corner < 0 || corner >= 3 * M.count) return;
        const double* x = M.face_cross + 3 * (corner / 3);
        s = add(s, d3{x[0], x[1], x[2]});
    }
    pose_put(M.vertex_sum + 3 * v, s);
}

// The record of face f of the mesh from the rest record (whose copied fields it keeps) and the new vertices.
RT_HD void deform_triangle_record(const DeformMesh& M, int f, const srt_collider& rest, srt_collider& out) {
    out = rest;
    const int32_t* cn = M.corner + 3 * f;
    for (int k = 0; k < 3; ++k)
        if (cn[k] < 0 || cn[k] >= M.n_verts) return;
    const d3 ctr{M.center[0], M.center[1], M.center[2]};
    const d3 p1 = add(deform_vertex(M.P, cn[0]), ctr), p2 = add(deform_vertex(M.P, cn[1]), ctr),
             p3 = add(deform_vertex(M.P, cn[2]), ctr);
    triangle_record_bary(rest.flags, triangle_record_geometry(p1, p2, p3, out.p), p1, p2, p3, out.p);
    if (!(rest.flags & SRT_CF_VNORMAL)) return;
    const d3 face{out.p[3], out.p[4], out.p[5]};
    for (int k = 0; k < 3; ++k)
        if (M.recompute[3 * f + k]) {
            const d3 s = deform_vertex(M.vertex_sum, cn[k]);
            const bool any = s.x != 0.0 || s.y != 0.0 || s.z != 0.0;
            pose_put(out.p + 24 + 3 * k, normalize(any ? s : face));
        }
}

// The corners naming each vertex in ascending corner order (a counting sort): offset[n_verts + 1], list[3 * count].
inline void deform_csr(const int32_t* corner, int count, int n_verts, std::vector<int32_t>& offset,
                       std::vector<int32_t>& list) {
    offset.assign((size_t)n_verts + 1, 0);
    for (int j = 0; j < 3 * count; ++j) offset[corner[j] + 1]++;
    for (int v = 0; v < n_verts; ++v) offset[v + 1] += offset[v];
    list.assign((size_t)3 * count, 0);
    std::vector<int32_t> at(offset.begin(), offset.end() - 1);
    for (int j = 0; j < 3 * count; ++j) list[at[corner[j]]++] = j;
}

#if defined(__HIPCC__)
// One thread per face.
__global__ void __launch_bounds__(256) k_deform_face_cross(DeformMesh M) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= M.count) return;
    deform_face_cross(M, f);
}

// One thread per vertex: a gather over its corner list.
__global__ void __launch_bounds__(256) k_deform_vertex_normals(DeformMesh M) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= M.n_verts) return;
    deform_vertex_sum(M, v);
}

// One thread per face: its record into the rest table and the live one (the range returns to the identity pose).
__global__ void __launch_bounds__(256) k_deform_triangles(DeformMesh M, srt_collider* __restrict__ rest,
                                                           srt_collider* __restrict__ live, int ncol) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= M.count) return;
    const int64_t i = (int64_t)M.first + f;
    if (i < 0 || i >= ncol) return;
    srt_collider out;
    deform_triangle_record(M, f, rest[i], out);
    rest[i] = out;
    live[i] = out;
}
#endif

}  // namespace rt
