// rt_api_anim.h -- the entry points that animate the resident scene's triangle meshes without an upload:
// srt_pose_colliders (rt_pose.h), srt_deform_topology and srt_deform_colliders (rt_deform.h), their srt_debug_*_times.
// All of them work on srt_ctx::mesh (MeshTables), which srt_upload_scene fills and resets.
// A fragment of rt_kernels.hip, included at its end and not compiled alone.  Before it: what stands above
// its include in rt_kernels.hip; it uses (finish_async).
namespace {

// the refusal of a call without a resident scene (`who`: the entry point, the message's prefix)
int need_scene(const srt_ctx* c, const char* who) {
    if (c->has_scene && c->mesh.col_live && c->mesh.col_rest) return SRT_OK;
    return fail(SRT_ERR_ARG, std::string(who) + ": no scene is resident");
}

// Before a call rewrites the collider table or the BVH: nothing on the device reads them any more.
int begin_table_rewrite(srt_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = finish_async(c, nullptr)) return rc;  // frames in flight read the tables rewritten below
    HIP_TRY(hipStreamSynchronize(c->f->stream));
    return SRT_OK;
}

// The BVH's boxes over the live table as it stands, height by height, leaves' parents first: a group reads the
// boxes the groups before it wrote.  Nothing to launch for a scene without a tree.
int refit_bvh(srt_ctx* c, hipStream_t st) {
    const MeshTables& M = c->mesh;
    if (c->S.bvh_nodes == 0) return SRT_OK;
    for (size_t h = 0; h + 1 < M.bvh_level_offset.size(); ++h) {
        const int off = M.bvh_level_offset[h], n = M.bvh_level_offset[h + 1] - off;
        if (n <= 0) continue;
        hipLaunchKernelGGL(k_bvh_refit, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, st, M.bvh_dev, c->S.bvh_nodes,
                           M.bvh_tri_dev, M.bvh_ntri, M.col_live, (int)M.col_host.size(), M.bvh_level_nodes + off, n);
        HIP_TRY(hipGetLastError());
    }
    return SRT_OK;
}

// what depends on the ranges alone, made once per set of ranges (rt_pose.h pose_layout_build)
int pose_layout_for(srt_ctx* c, int32_t n_ranges, const int32_t* first, const int32_t* count) {
    MeshTables& M = c->mesh;
    std::vector<int32_t> key;
    for (int r = 0; r < n_ranges; ++r) key.insert(key.end(), {first[r], count[r]});
    if (!M.pose_layout.key.empty() && M.pose_layout.key == key) return SRT_OK;
    const std::string refusal =
        pose_layout_build(M.col_host.data(), (int)M.col_host.size(), n_ranges, first, count, M.pose_layout);
    return refusal.empty() ? SRT_OK : fail(SRT_ERR_ARG, "srt_pose_colliders: " + refusal);
}

}  // namespace

extern "C" {

int srt_pose_colliders(srt_ctx* c, int32_t n_ranges, const int32_t* first, const int32_t* count, const double* poses) {
    if (!c) return fail(SRT_ERR_ARG, "srt_pose_colliders: null ctx");
    int rc;
    if ((rc = need_scene(c, "srt_pose_colliders"))) return rc;
    if (n_ranges < 1 || !first || !count || !poses) return fail(SRT_ERR_ARG, "srt_pose_colliders: needs n_ranges >= 1 ranges and their poses");
    for (int64_t k = 0; k < (int64_t)n_ranges * POSE_DOUBLES; ++k)
        if (!std::isfinite(poses[k])) return fail(SRT_ERR_ARG, "srt_pose_colliders: a pose entry is not finite");
    if ((rc = pose_layout_for(c, n_ranges, first, count))) return rc;
    if ((rc = begin_table_rewrite(c))) return rc;
    MeshTables& M = c->mesh;
    const hipStream_t st = c->f->stream;
    std::vector<PoseRange> R((size_t)n_ranges);
    int64_t total = 0;
    for (int r = 0; r < n_ranges; ++r) {
        R[r].first = first[r];
        R[r].count = count[r];
        R[r].start = total;
        total += count[r];
        memcpy(R[r].pose, poses + (size_t)r * POSE_DOUBLES, sizeof R[r].pose);
    }
    bool all_identity = true;
    const float bound = pose_layout_bound(M.pose_layout, poses, M.bvh_bound_rest, all_identity);
    if ((rc = M.pose_ranges.ensure(n_ranges))) return rc;
    HIP_TRY(hipMemcpyAsync(M.pose_ranges, R.data(), R.size() * sizeof(PoseRange), hipMemcpyHostToDevice, st));
    HIP_TRY(M.pose_timer.mark(0, st));
    hipLaunchKernelGGL(k_pose_triangles, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, M.col_rest, M.col_live,
                       M.pose_ranges.p, n_ranges, total, (int)M.col_host.size());
    HIP_TRY(hipGetLastError());
    HIP_TRY(M.pose_timer.mark(1, st));
    if ((rc = refit_bvh(c, st))) return rc;
    if (c->S.bvh_nodes > 0) c->S.bvh_bound = bound;
    M.pose_active = !all_identity;
    HIP_TRY(M.pose_timer.mark(2, st));
    HIP_TRY(hipStreamSynchronize(st));  // the next frame may run on another slot's stream
    HIP_TRY(M.pose_timer.collect());
    return SRT_OK;
}

int srt_debug_pose_times(srt_ctx* c, double* ms_pose, double* ms_refit, int64_t* calls) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    const StageTimer<2>& T = c->mesh.pose_timer;
    if (ms_pose) *ms_pose = T.ms[0];
    if (ms_refit) *ms_refit = T.ms[1];
    if (calls) *calls = T.calls;
    return SRT_OK;
}

int srt_deform_topology(srt_ctx* c, int32_t first, int32_t count, int32_t n_verts, const int32_t* corners,
                        const double* center, const uint8_t* recompute) {
    if (!c) return fail(SRT_ERR_ARG, "srt_deform_topology: null ctx");
    if (int rc = need_scene(c, "srt_deform_topology")) return rc;
    if (!corners || !center || !recompute) return fail(SRT_ERR_ARG, "srt_deform_topology: needs corners, center and the corner flags");
    MeshTables& M = c->mesh;
    if (const char* fault = triangle_range_fault(M.col_host.data(), (int)M.col_host.size(), first, count))
        return fail(SRT_ERR_ARG, std::string("srt_deform_topology: the range") + fault);
    for (const DeformTopo& t : M.deform_meshes)
        if (first < t.m.first + t.m.count && t.m.first < first + count)
            return fail(SRT_ERR_ARG, "srt_deform_topology: the range overlaps a registered one");
    if (n_verts < 1) return fail(SRT_ERR_ARG, "srt_deform_topology: needs n_verts >= 1");
    bool normals = false;
    for (int64_t j = 0; j < 3 * (int64_t)count; ++j) {
        if (corners[j] < 0 || corners[j] >= n_verts)
            return fail(SRT_ERR_ARG, "srt_deform_topology: a corner index lies outside [0, n_verts)");
        normals = normals || recompute[j];
    }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(center[k])) return fail(SRT_ERR_ARG, "srt_deform_topology: center is not finite");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> offset, list;
    deform_csr(corners, count, n_verts, offset, list);
    DeformTopo t;
    int32_t *d_corner, *d_offset, *d_list;
    uint8_t* d_flag;
    HIP_TRY(c->scene_bufs.in(&d_corner, corners, 3 * (int64_t)count));
    HIP_TRY(c->scene_bufs.in(&d_flag, recompute, 3 * (int64_t)count));
    HIP_TRY(c->scene_bufs.in(&d_offset, (const int32_t*)offset.data(), (int64_t)offset.size()));
    HIP_TRY(c->scene_bufs.in(&d_list, (const int32_t*)list.data(), (int64_t)list.size()));
    HIP_TRY(c->scene_bufs.alloc(&t.P, 3 * (int64_t)n_verts));
    HIP_TRY(c->scene_bufs.alloc(&t.m.face_cross, 3 * (int64_t)count));
    HIP_TRY(c->scene_bufs.alloc(&t.m.vertex_sum, 3 * (int64_t)n_verts));
    t.m.first = first, t.m.count = count, t.m.n_verts = n_verts;
    t.m.corner = d_corner, t.m.recompute = d_flag, t.m.csr_offset = d_offset, t.m.csr_corner = d_list;
    t.m.P = t.P;
    for (int k = 0; k < 3; ++k) t.m.center[k] = center[k];
    t.normals = normals;
    M.deform_meshes.push_back(t);
    return SRT_OK;
}

int srt_deform_colliders(srt_ctx* c, int32_t n_meshes, const int32_t* first, const int32_t* count,
                         const double* const* verts) {
    if (!c) return fail(SRT_ERR_ARG, "srt_deform_colliders: null ctx");
    int rc;
    if ((rc = need_scene(c, "srt_deform_colliders"))) return rc;
    if (n_meshes < 1 || !first || !count || !verts) return fail(SRT_ERR_ARG, "srt_deform_colliders: needs n_meshes >= 1 ranges and their vertex arrays");
    MeshTables& M = c->mesh;
    std::vector<const DeformTopo*> meshes((size_t)n_meshes, nullptr);
    for (int r = 0; r < n_meshes; ++r) {
        for (const DeformTopo& t : M.deform_meshes)
            if (t.m.first == first[r] && t.m.count == count[r]) meshes[r] = &t;
        if (!meshes[r]) return fail(SRT_ERR_ARG, "srt_deform_colliders: a range is not registered (srt_deform_topology)");
        for (int q = 0; q < r; ++q)
            if (meshes[q] == meshes[r]) return fail(SRT_ERR_ARG, "srt_deform_colliders: a range is named twice");
        if (!verts[r]) return fail(SRT_ERR_ARG, "srt_deform_colliders: a vertex array is null");
        const int64_t n = 3 * (int64_t)meshes[r]->m.n_verts;
        for (int64_t j = 0; j < n; ++j)
            if (!std::isfinite(verts[r][j])) return fail(SRT_ERR_ARG, "srt_deform_colliders: a coordinate is not finite");
    }
    if ((rc = begin_table_rewrite(c))) return rc;
    const hipStream_t st = c->f->stream;
    const int ncol = (int)M.col_host.size();
    for (int r = 0; r < n_meshes; ++r) {
        const DeformTopo& t = *meshes[r];
        HIP_TRY(hipMemcpyAsync(t.P, verts[r], sizeof(double) * 3 * (size_t)t.m.n_verts, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(M.deform_timer.mark(0, st));
    for (const DeformTopo* t : meshes) {
        if (!t->normals) continue;
        hipLaunchKernelGGL(k_deform_face_cross, dim3((unsigned)((t->m.count + 255) / 256)), dim3(256), 0, st, t->m);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_deform_vertex_normals, dim3((unsigned)((t->m.n_verts + 255) / 256)), dim3(256), 0, st, t->m);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(M.deform_timer.mark(1, st));
    for (const DeformTopo* t : meshes) {
        hipLaunchKernelGGL(k_deform_triangles, dim3((unsigned)((t->m.count + 255) / 256)), dim3(256), 0, st, t->m,
                           M.col_rest, M.col_live, ncol);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(M.deform_timer.mark(2, st));
    if ((rc = refit_bvh(c, st))) return rc;
    HIP_TRY(M.deform_timer.mark(3, st));
    // the host's copy of the rest table follows (a later pose call takes its boxes and reach from it)
    for (const DeformTopo* t : meshes)
        HIP_TRY(hipMemcpyAsync(M.col_host.data() + t->m.first, M.col_rest + t->m.first, sizeof(srt_collider) * (size_t)t->m.count,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // the next frame may run on another slot's stream
    M.pose_layout = PoseLayout{};
    if (c->S.bvh_nodes > 0) {
        const float bound = rest_table_bound(M.col_host.data(), ncol);
        // (ranges outside this call may still be posed: the bound that held for their boxes goes on holding)
        c->S.bvh_bound = M.pose_active ? std::max(c->S.bvh_bound, bound) : bound;
        M.bvh_bound_rest = bound;
    }
    HIP_TRY(M.deform_timer.collect());
    return SRT_OK;
}

int srt_debug_deform_times(srt_ctx* c, double* ms_normals, double* ms_records, double* ms_refit, int64_t* calls) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    const StageTimer<3>& T = c->mesh.deform_timer;
    if (ms_normals) *ms_normals = T.ms[0];
    if (ms_records) *ms_records = T.ms[1];
    if (ms_refit) *ms_refit = T.ms[2];
    if (calls) *calls = T.calls;
    return SRT_OK;
}

}  // extern "C"
