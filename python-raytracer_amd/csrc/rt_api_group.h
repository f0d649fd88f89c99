// rt_api_group.h -- several GPUs: the RCCL communicators (srt_comm_*), a frame sharded over the contexts of
// one process (gather_group, finish_group, render_group_once / _async, srt_render_group and
// srt_render_group_finish), srt_comm_allreduce and srt_comm_barrier.
// A fragment of rt_kernels.hip, included at its end and not compiled alone.  Before it: what stands above
// its include in rt_kernels.hip; it uses (srt_create, srt_destroy, srt_render, srt_render_finish, gather_post,
// gather_finish, finish_async, NCCL_TRY).
extern "C" {

// ---- multi-GPU ------------------------------------------------------------------------------
int srt_comm_unique_id(uint8_t* id) {
    if (!id) return fail(SRT_ERR_ARG, "null id");
    static_assert(sizeof(ncclUniqueId) == SRT_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    NCCL_TRY(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return SRT_OK;
}

int srt_comm_init(srt_ctx* c, int nranks, int rank, const uint8_t* id) {
    if (!c || !id || nranks < 1 || nranks > MAX_RANKS || rank < 0 || rank >= nranks)
        return fail(SRT_ERR_ARG, "bad communicator arguments");
    if (c->comm) return fail(SRT_ERR_ARG, "context already has a communicator");
    HIP_TRY(hipSetDevice(c->device));
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    NCCL_TRY(ncclCommInitRank(&c->comm, nranks, u, rank));
    c->nranks = nranks;
    c->rank = rank;
    return SRT_OK;
}

int srt_comm_init_all(int ndev, const int* devs, srt_ctx** ctxs) {
    if (ndev < 1 || ndev > MAX_RANKS || !devs || !ctxs) return fail(SRT_ERR_ARG, "bad device list");
    for (int q = 0; q < ndev; ++q) ctxs[q] = nullptr;
    for (int q = 0; q < ndev; ++q) {
        int rc = srt_create(devs[q], &ctxs[q]);
        if (rc) {
            for (int k = 0; k < q; ++k) srt_destroy(ctxs[k]);
            return rc;
        }
    }
    std::vector<ncclComm_t> comms(ndev);
    ncclResult_t r = ncclCommInitAll(comms.data(), ndev, devs);
    if (r != ncclSuccess) {
        for (int k = 0; k < ndev; ++k) srt_destroy(ctxs[k]);
        return fail(SRT_ERR_HIP, std::string("ncclCommInitAll: ") + ncclGetErrorString(r));
    }
    for (int q = 0; q < ndev; ++q) {
        ctxs[q]->comm = comms[q];
        ctxs[q]->nranks = ndev;
        ctxs[q]->rank = q;
    }
    return SRT_OK;
}

int srt_comm_rank(srt_ctx* c, int* nranks, int* rank) {
    if (!c || !nranks || !rank) return fail(SRT_ERR_ARG, "null argument");
    *nranks = c->nranks;
    *rank = c->rank;
    return SRT_OK;
}

}  // extern "C"

// The gathers of all the group's contexts posted in one RCCL group, then the frame assembled on rank 0
static int gather_group(srt_ctx** ctxs, int n) {
    int rc = SRT_OK;
    if (n > 1) {
        ncclResult_t r = ncclGroupStart();
        for (int q = 0; q < n && !rc && r == ncclSuccess; ++q) {
            (void)hipSetDevice(ctxs[q]->device);
            rc = gather_post(ctxs[q]);
        }
        ncclResult_t r2 = ncclGroupEnd();
        if (!rc && (r != ncclSuccess || r2 != ncclSuccess))
            rc = fail(SRT_ERR_HIP, std::string("RCCL group gather: ") + ncclGetErrorString(r != ncclSuccess ? r : r2));
    }
    if (!rc) {
        (void)hipSetDevice(ctxs[0]->device);
        rc = gather_finish(ctxs[0]);
    }
    return rc;
}

// srt_render_finish on every context (whatever `rc` the frame had so far: no rank is left with frames
// in flight); `sum`: rank 0's stats with the ray counts of all ranks.  Returns the first error.
static int finish_group(srt_ctx** ctxs, int n, srt_stats& sum, int rc) {
    for (int q = 0; q < n; ++q) {
        srt_stats sq{};
        const int r = srt_render_finish(ctxs[q], &sq);
        if (!rc) rc = r;
        if (q == 0) {
            sum = sq;
        } else {
            for (int d = 0; d < SRT_MAX_DEPTHS; ++d) sum.rays_per_depth[d] += sq.rays_per_depth[d];
            sum.total_rays += sq.total_rays;
            sum.shadow_rays += sq.shadow_rays;
            sum.n_depths = std::max(sum.n_depths, sq.n_depths);
        }
    }
    return rc;
}

static int render_group_once(srt_ctx** ctxs, int n, const srt_camera* cam, const srt_render_args* a, srt_stats* st) {
    const bool want_rgb = a->out_rgb != nullptr;
    int rc = SRT_OK;
    srt_render_args aq = *a;
    aq.flags = SRT_RENDER_ASYNC | SRT_RENDER_SHARDED | (want_rgb ? SRT_RENDER_GATHER_RGB : (a->flags & SRT_RENDER_RGB_LOCAL));
    aq.out_rgb = nullptr;  // rank 0 assembles into its slot buffers; copied to the caller's below
    aq.out_srgb8 = nullptr;
    for (int q = 0; q < n && !rc; ++q) {
        if ((rc = finish_async(ctxs[q], nullptr))) break;
        ctxs[q]->defer_gather = true;
        rc = srt_render(ctxs[q], cam, &aq, nullptr);
    }
    FrameSlot* f0 = ctxs[0]->f;
    if (!rc) rc = gather_group(ctxs, n);
    for (int q = 0; q < n; ++q) ctxs[q]->defer_gather = false;
    srt_stats sum{};
    rc = finish_group(ctxs, n, sum, rc);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctxs[0]->device));
    const int64_t np = (int64_t)cam->width * cam->height;
    if (a->out_srgb8) HIP_TRY(hipMemcpy(a->out_srgb8, f0->full_u8, (size_t)3 * np, hipMemcpyDefault));
    if (want_rgb) HIP_TRY(hipMemcpy(a->out_rgb, f0->full_rgb, (size_t)3 * np * 8, hipMemcpyDefault));
    if (st) *st = sum;
    return SRT_OK;
}

// A pipelined group frame (SRT_RENDER_ASYNC): every context queues its shard (asynchronous
// srt_render, SRT_RENDER_SHARDED), the uint8 tiles' RCCL gather is posted for all of them in one
// group, rank 0 assembles the frame and copies it to the caller's out_srgb8 (pinned host memory or
// device memory of rank 0); the linear RGB goes to out_rgb (pinned host memory visible to every
// context, srt_host_alloc) either gathered to rank 0 or, with SRT_RENDER_RGB_ROWS, as every rank's
// rows over its own PCIe link.  Nothing waits: srt_render_group_finish checks every context.
static int render_group_async(srt_ctx** ctxs, int n, const srt_camera* cam, const srt_render_args* a) {
    srt_render_args aq = *a;
    const bool rows = (a->flags & SRT_RENDER_RGB_ROWS) != 0;
    aq.flags = SRT_RENDER_ASYNC | SRT_RENDER_SHARDED | (a->flags & SRT_RENDER_RGB_LOCAL) |
               (rows ? SRT_RENDER_RGB_ROWS : (a->out_rgb ? SRT_RENDER_GATHER_RGB : 0));
    int rc = SRT_OK;
    int queued = 0;
    for (int q = 0; q < n && !rc; ++q) {
        aq.out_srgb8 = q == 0 ? a->out_srgb8 : nullptr;
        aq.out_rgb = (rows || q == 0) ? a->out_rgb : nullptr;
        ctxs[q]->defer_gather = true;
        rc = srt_render(ctxs[q], cam, &aq, nullptr);
        if (!rc) ++queued;
    }
    if (!rc) rc = gather_group(ctxs, n);
    for (int q = 0; q < n; ++q) ctxs[q]->defer_gather = false;
    if (rc && queued < n) {
        // a context refused the frame: the others' shards are queued without the gather; wait for them
        // (their frames are dropped) so that no rank is left a send without its receive
        for (int q = 0; q < queued; ++q) (void)srt_render_finish(ctxs[q], nullptr);
    }
    return rc;
}

extern "C" {

int srt_render_group(srt_ctx** ctxs, int n, const srt_camera* cam, const srt_render_args* a, srt_stats* st) {
    if (!ctxs || n < 1 || !cam || !a) return fail(SRT_ERR_ARG, "null argument");
    for (int q = 0; q < n; ++q)
        if (!ctxs[q] || ctxs[q]->nranks != n || ctxs[q]->rank != q)
            return fail(SRT_ERR_ARG, "contexts must be the ranks 0..n-1 of one srt_comm_init_all group");
    for (int q = 0; q < n; ++q) ctxs[q]->pf.valid = false;
    for (int q = 0; q < n; ++q)
        if (ctxs[q]->has_scene && ctxs[q]->needs_inputs) return refuse_inputs_scene("srt_render_group");
    if (a->jitter) return fail(SRT_ERR_ARG, "a group frame draws its jitter on the devices (mt or Philox)");
    if (a->out_hit_id) return fail(SRT_ERR_ARG, "hit ids of a sharded frame are not gathered");
    if (a->flags & ~(SRT_RENDER_ASYNC | SRT_RENDER_RGB_ROWS | SRT_RENDER_RGB_LOCAL))
        return fail(SRT_ERR_ARG, "group flags: ASYNC, RGB_ROWS, RGB_LOCAL");
    if ((a->flags & SRT_RENDER_RGB_LOCAL) && (a->out_rgb || (a->flags & SRT_RENDER_RGB_ROWS)))
        return fail(SRT_ERR_ARG, "SRT_RENDER_RGB_LOCAL needs out_rgb NULL and no SRT_RENDER_RGB_ROWS");
    if (a->flags & SRT_RENDER_ASYNC) return render_group_async(ctxs, n, cam, a);
    // A frame whose passes overflowed a queue/ring, met a chain-mode tie or left the fixed-point range
    // is rendered again on every context (the gather pairs the ranks' tiles), from the same numpy
    // state, as the synchronous single-GPU path does; the contexts already grew their queues or
    // dropped chain mode / fixed-point sums in finish_async.
    srt_mt_state mt0{};
    if (a->mt) mt0 = *a->mt;
    int rc = SRT_OK;
    for (int attempt = 0;; ++attempt) {
        if (a->mt) *a->mt = mt0;
        // (a flag left by an earlier frame must not make a failure of this one look retryable)
        for (int q = 0; q < n; ++q) ctxs[q]->retry_frame = false;
        rc = render_group_once(ctxs, n, cam, a, st);
        bool again = false;
        for (int q = 0; q < n; ++q) again |= ctxs[q]->retry_frame;
        if (rc == SRT_OK && st) st->retries += attempt;  // frames rendered again, as srt_render counts them
        if (rc == SRT_OK || !again || attempt >= 8) return rc;
    }
}


int srt_render_group_finish(srt_ctx** ctxs, int n, srt_stats* st) {
    if (!ctxs || n < 1) return fail(SRT_ERR_ARG, "null argument");
    srt_stats sum{};
    const int rc = finish_group(ctxs, n, sum, SRT_OK);
    if (st && !rc) *st = sum;
    return rc;
}

int srt_comm_allreduce(srt_ctx* c, double* vals, int n, int op) {
    if (!c || !vals || n < 1 || n > 64 || op < 0 || op > 1) return fail(SRT_ERR_ARG, "bad allreduce arguments");
    if (c->nranks == 1 || !c->comm) return SRT_OK;
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_async(c, nullptr);
    if (rc) return rc;
    if (!c->red) HIP_TRY(dalloc(&c->red, 64));
    hipStream_t st = c->f->stream;
    HIP_TRY(hipMemcpyAsync(c->red, vals, (size_t)n * 8, hipMemcpyHostToDevice, st));
    NCCL_TRY(ncclAllReduce(c->red, c->red, (size_t)n, ncclFloat64, op == 0 ? ncclSum : ncclMax, c->comm, st));
    HIP_TRY(hipMemcpyAsync(vals, c->red, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SRT_OK;
}

int srt_comm_barrier(srt_ctx* c) {
    double v = 0.0;
    return srt_comm_allreduce(c, &v, 1, 0);
}

}  // extern "C"
