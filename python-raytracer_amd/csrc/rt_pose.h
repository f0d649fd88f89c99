// rt_pose.h -- rigidly posed triangle meshes: the collider records of a mesh recomputed on the device
// from a resident copy in the pose the scene was uploaded in (the rest pose), and the BVH's boxes refitted
// over the posed vertices (srt_pose_colliders in rt_api_anim.h; the CPU check harness rt_hostcheck.cpp
// runs the same functions).  The trace kernels read the rewritten tables as they read uploaded ones.
//
// A pose is 12 doubles, R row-major then T (the layout of srt_temporal_accumulate's motion rows).  A vertex
// moves as x'_k = ((R[k][0] x + R[k][1] y) + R[k][2] z) + T[k]; a vertex normal as normalize(R n) with the
// same sums without T.  Every other field of the record is recomputed from the three posed vertices as
// sightpy's Triangle_Collider computes it (geometry/triangle.py, _lower.collider_record), in its
// operation order, contraction off.  The identity pose (R = I and T = 0 exactly) copies the rest record.
#pragma once

#include <array>
#include <string>
#include <vector>

#include "rt_bvh.h"
#include "rt_device.h"

namespace rt {

constexpr int POSE_DOUBLES = 12;

template <class P>
RT_HD bool pose_is_identity(P pose) {
    bool id = true;
    for (int k = 0; k < 9; ++k) id = id && pose[k] == ((k & 3) == 0 ? 1.0 : 0.0);
    for (int k = 9; k < 12; ++k) id = id && pose[k] == 0.0;
    return id;
}

template <class P>
RT_HD d3 pose_rotate(P R, d3 v) {
    return d3{(R[0] * v.x + R[1] * v.y) + R[2] * v.z, (R[3] * v.x + R[4] * v.y) + R[5] * v.z,
              (R[6] * v.x + R[7] * v.y) + R[8] * v.z};
}
template <class P>
RT_HD d3 pose_point(P pose, d3 v) {
    const d3 r = pose_rotate(pose, v);
    return d3{r.x + pose[9], r.y + pose[10], r.z + pose[11]};
}
// vec3.cross (utils/vector3.py)
RT_HD d3 pose_cross(d3 a, d3 b) { return d3{a.y * b.z - a.z * b.y, -a.x * b.z + a.z * b.x, a.x * b.y - a.y * b.x}; }
RT_HD void pose_put(double* p, d3 v) {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
}

// The fields of a triangle's record that follow from its three vertices alone, as Triangle_Collider computes
// them, written to the record's parameters `p` in two steps (shared with the deformed meshes of rt_deform.h; every
// other slot of `p` stays as it is): centroid, normal, the vertices, n31, n12, n23 ...
struct TriangleEdges {
    d3 n31, n12;
};
RT_HD TriangleEdges triangle_record_geometry(d3 p1, d3 p2, d3 p3, double* p) {
    const d3 nrm = normalize(pose_cross(sub(p2, p1), sub(p3, p1)));
    const d3 n31 = pose_cross(sub(p3, p1), nrm), n12 = pose_cross(sub(p1, p2), nrm);
    pose_put(p + 0, divs(add(add(p1, p2), p3), 3.0));
    pose_put(p + 3, nrm);
    pose_put(p + 6, p1);
    pose_put(p + 9, p2);
    pose_put(p + 12, p3);
    pose_put(p + 15, n31);
    pose_put(p + 18, n12);
    pose_put(p + 21, pose_cross(sub(p2, p3), nrm));
    return TriangleEdges{n31, n12};
}
// ... and, with an attribute flag among `flags`, d2 and d3 (the uvs p[33..38] stay as copied)
RT_HD void triangle_record_bary(uint32_t flags, TriangleEdges e, d3 p1, d3 p2, d3 p3, double* p) {
    if (flags & (SRT_CF_VNORMAL | SRT_CF_VUV)) {
        p[39] = dot(e.n31, sub(p2, p1));
        p[40] = dot(e.n12, sub(p3, p2));
    }
}

// The record of triangle `rest` under `pose` (type, flags, material and the other integer fields copied).
template <class P>
RT_HD void pose_triangle_record(const srt_collider& rest, P pose, srt_collider& out) {
    out = rest;
    if (pose_is_identity(pose)) return;
    const double* q = rest.p;
    const d3 p1 = pose_point(pose, d3{q[6], q[7], q[8]});
    const d3 p2 = pose_point(pose, d3{q[9], q[10], q[11]});
    const d3 p3 = pose_point(pose, d3{q[12], q[13], q[14]});
    const TriangleEdges e = triangle_record_geometry(p1, p2, p3, out.p);
    if (rest.flags & SRT_CF_VNORMAL)
        for (int i = 0; i < 3; ++i)
            pose_put(out.p + 24 + 3 * i, normalize(pose_rotate(pose, d3{q[24 + 3 * i], q[25 + 3 * i], q[26 + 3 * i]})));
    triangle_record_bary(rest.flags, e, p1, p2, p3, out.p);
}

// One slot of a BVH node from what lies below it: a leaf slot's box is the union of its triangles' boxes
// (bvh_triangle_box over the live records) rounded outward, an inner slot's the union of the child node's
// slot boxes (already refitted: rt_bvh.h BvhLevels), an empty slot's stays empty.  Rounding to float is
// monotone, so the float unions equal the build's rounded f64 unions.
RT_HD void bvh_refit_slot(BvhNode* nodes, const int32_t* tri, const srt_collider* col, int node, int k) {
    BvhNode& nd = nodes[node];
    const int32_t ch = nd.child[k];
    if (ch == BVH_EMPTY) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (ch < 0) {
        const int first = -ch - 1;
        for (int i = 0; i < nd.count[k]; ++i) {
            double tlo[3], thi[3];
            bvh_triangle_box(col[tri[first + i]].p, tlo, thi);
            for (int a = 0; a < 3; ++a) {
                const float l = bvh_round_down(tlo[a]), h = bvh_round_up(thi[a]);
                lo[a] = l < lo[a] ? l : lo[a];
                hi[a] = hi[a] < h ? h : hi[a];
            }
        }
    } else {
        const BvhNode& c = nodes[ch];
        for (int j = 0; j < 4; ++j)
            for (int a = 0; a < 3; ++a) {
                lo[a] = c.lo[a][j] < lo[a] ? c.lo[a][j] : lo[a];
                hi[a] = hi[a] < c.hi[a][j] ? c.hi[a][j] : hi[a];
            }
    }
    for (int a = 0; a < 3; ++a) {
        nd.lo[a][k] = lo[a];
        nd.hi[a][k] = hi[a];
    }
}

// A posed range of the collider table: colliders [first, first + count), thread offset `start` in
// k_pose_triangles' grid (the counts' running sum), the pose.
struct PoseRange {
    int32_t first, count;
    int64_t start;
    double pose[POSE_DOUBLES];
};

// A bound of the |coordinate| a point of the box [lo, hi] can take under `pose`: the largest over its eight
// corners (the map is affine), plus the rounding of the six operations on terms of the size of the
// products and T (which may cancel: a far mesh moved to the origin)
inline double pose_box_reach(const double* lo, const double* hi, const double* pose) {
    double m = 0.0;
    for (int c = 0; c < 8; ++c) {
        const d3 x{(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
        const d3 v = pose_point(pose, x);
        const double out[3] = {v.x, v.y, v.z};
        for (int k = 0; k < 3; ++k) {
            const double terms = std::fabs(pose[3 * k] * x.x) + std::fabs(pose[3 * k + 1] * x.y) +
                                 std::fabs(pose[3 * k + 2] * x.z) + std::fabs(pose[9 + k]);
            m = std::max(m, std::fabs(out[k]) + 1e-15 * terms);
        }
    }
    return m;
}

// the vertex box (lo[3], hi[3], not inflated) of the triangles col[first, first + count)
inline void pose_range_box(const srt_collider* col, int first, int count, double* box) {
    for (int k = 0; k < 3; ++k) box[k] = INFINITY, box[3 + k] = -INFINITY;
    for (int i = first; i < first + count; ++i)
        for (int v = 6; v < 15; ++v) {
            box[v % 3] = std::min(box[v % 3], col[i].p[v]);
            box[3 + v % 3] = std::max(box[3 + v % 3], col[i].p[v]);
        }
}
// max |vertex coordinate| of the triangles among col[0, ncol) that `posed` does not mark (null: marks none)
inline double pose_static_reach(const srt_collider* col, int ncol, const uint8_t* posed) {
    double reach = 0.0;
    for (int i = 0; i < ncol; ++i)
        if (!(posed && posed[i]) && col[i].type == SRT_TRIANGLE)
            for (int v = 6; v < 15; ++v) reach = std::max(reach, std::fabs(col[i].p[v]));
    return reach;
}
// SceneView::bvh_bound for a tree refitted over vertices within `reach` of the origin: the build's inflation
// twice over (the refit inflates by its own, rounded vertices' reach), rounded up
inline float pose_bound(double reach) { return bvh_round_up(reach * (1.0 + 1e-12) + 2e-9 * (1.0 + reach)); }

// ---- SceneView::bvh_bound after a pose or a deformation: the host-side rule, which srt_pose_colliders and
// srt_deform_colliders (rt_api_anim.h) and the CPU check harness (rt_hostcheck.cpp) both run ----
// Why col[first, first + count) is no range of Triangle colliders of the table col[0, ncol), as the words that
// follow the refusal's subject ("a range", "the range"); null when it is one.
inline const char* triangle_range_fault(const srt_collider* col, int ncol, int first, int count) {
    if (first < 0 || count < 1 || (int64_t)first + count > ncol) return " lies outside the collider table";
    for (int i = first; i < first + count; ++i)
        if (col[i].type != SRT_TRIANGLE) return " covers a collider that is no Triangle";
    return nullptr;
}

// What a set of posed ranges fixes whatever their poses are (so it is kept while the ranges stay the same: `key`).
struct PoseLayout {
    std::vector<int32_t> key;                // first, count per range: valid for these, over an unchanged rest table
    std::vector<std::array<double, 6>> box;  // rest vertex box per range
    double static_reach = 0.0;               // max |coordinate| of the triangles in no range
};
// The layout of `n_ranges` ranges over the rest table col[0, ncol), each range checked in turn (inside the table,
// triangles only, no overlap with an earlier one).  Returns the refusal, or an empty string with `PL` filled.
inline std::string pose_layout_build(const srt_collider* col, int ncol, int n_ranges, const int32_t* first,
                                     const int32_t* count, PoseLayout& PL) {
    PL = PoseLayout{};
    std::vector<uint8_t> posed((size_t)ncol, 0);
    std::vector<std::array<double, 6>> box((size_t)n_ranges);
    for (int r = 0; r < n_ranges; ++r) {
        if (const char* fault = triangle_range_fault(col, ncol, first[r], count[r])) return std::string("a range") + fault;
        for (int i = first[r]; i < first[r] + count[r]; ++i) {
            if (posed[i]) return "the ranges overlap";
            posed[i] = 1;
        }
        pose_range_box(col, first[r], count[r], box[r].data());
    }
    for (int r = 0; r < n_ranges; ++r) PL.key.insert(PL.key.end(), {first[r], count[r]});
    PL.static_reach = pose_static_reach(col, ncol, posed.data());
    PL.box = std::move(box);
    return std::string();
}
// The bound of the tree refitted with the layout's ranges under `poses` (POSE_DOUBLES each); `rest_bound` is the
// bound of the rest shape's tree, which holds again when every pose is the identity (`all_identity`).
inline float pose_layout_bound(const PoseLayout& PL, const double* poses, float rest_bound, bool& all_identity) {
    double reach = PL.static_reach;
    all_identity = true;
    for (size_t r = 0; r < PL.box.size(); ++r) {
        const double* pose = poses + r * POSE_DOUBLES;
        all_identity = all_identity && pose_is_identity(pose);
        reach = std::max(reach, pose_box_reach(PL.box[r].data(), PL.box[r].data() + 3, pose));
    }
    return all_identity ? rest_bound : pose_bound(reach);
}
// The bound of the tree refitted over the table col[0, ncol) as it stands (a deformation's new rest shape).
inline float rest_table_bound(const srt_collider* col, int ncol) { return pose_bound(pose_static_reach(col, ncol, nullptr)); }

#if defined(__HIPCC__)
// One thread per triangle of the posed ranges (`total` in all): the live record from the rest record.
__global__ void __launch_bounds__(256) k_pose_triangles(const srt_collider* __restrict__ rest,
                                                         srt_collider* __restrict__ live,
                                                         const PoseRange* __restrict__ ranges, int n_ranges,
                                                         int64_t total, int ncol) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    int lo = 0, hi = n_ranges - 1;  // the last range with start <= t
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ranges[mid].start <= t) lo = mid; else hi = mid - 1;
    }
    const PoseRange& r = ranges[lo];
    const int64_t i = r.first + (t - r.start);
    if (t - r.start >= r.count || i < 0 || i >= ncol) return;
    srt_collider out;
    pose_triangle_record(rest[i], r.pose, out);
    live[i] = out;
}

// One thread per slot of the nodes list[0, n) (one height group of BvhLevels).
__global__ void __launch_bounds__(256) k_bvh_refit(BvhNode* nodes, int n_nodes, const int32_t* __restrict__ tri,
                                                    int n_tri, const srt_collider* __restrict__ col, int ncol,
                                                    const int32_t* __restrict__ list, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * n) return;
    const int node = list[t >> 2], k = t & 3;
    if (node < 0 || node >= n_nodes) return;
    // (the tables are the library's own: these bounds only keep a damaged one from a stray access)
    const int32_t ch = nodes[node].child[k];
    if (ch >= n_nodes) return;
    if (ch < 0 && ch != BVH_EMPTY) {
        const int first = -ch - 1, cnt = nodes[node].count[k];
        if (cnt < 0 || first + cnt > n_tri) return;
        for (int i = 0; i < cnt; ++i)
            if (tri[first + i] < 0 || tri[first + i] >= ncol) return;
    }
    bvh_refit_slot(nodes, tri, col, node, k);
}
#endif

}  // namespace rt
