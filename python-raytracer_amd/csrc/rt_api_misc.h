// rt_api_misc.h -- the remaining entry points: pinned host memory (srt_host_*), the srt_debug_* hooks,
// srt_synchronize.
// A fragment of rt_kernels.hip, included at its end and not compiled alone.  Before it: what stands above
// its include in rt_kernels.hip; it uses (finish_async, mt_end_acc).
extern "C" {

// (hipHostMalloc places the buffer on the GPU's NUMA node: tools/pcie_probe.py, 56 GB/s either way
// the calling process is pinned)
int srt_host_alloc(srt_ctx* c, int64_t bytes, void** out) {
    if (!c || !out || bytes <= 0) return fail(SRT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocPortable));  // (pinned for every context's device)
    return SRT_OK;
}

int srt_host_register(srt_ctx* c, void* p, int64_t bytes) {
    if (!c || !p || bytes <= 0) return fail(SRT_ERR_ARG, "null ctx/pointer or bad size");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostRegister(p, (size_t)bytes, hipHostRegisterPortable));
    return SRT_OK;
}

int srt_host_unregister(srt_ctx* c, void* p) {
    if (!c || !p) return fail(SRT_ERR_ARG, "null ctx/pointer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_async(c, nullptr);  // frames in flight may still write into it
    if (rc) return rc;
    HIP_TRY(hipHostUnregister(p));
    return SRT_OK;
}

int srt_host_free(srt_ctx* c, void* p) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    if (p) HIP_TRY(hipHostFree(p));
    return SRT_OK;
}

#ifdef RT_PROF
// diagnostic build only: section counters of rt_device.h (64 words: 32 cycle sums, 32 counts)
int srt_debug_prof(srt_ctx* c, unsigned long long* out, int reset) {
    if (!c || !out) return fail(SRT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->f->stream));
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rt_prof), sizeof(unsigned long long) * 64));
    if (reset) {
        unsigned long long z[64] = {};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rt_prof), z, sizeof(z)));
    }
    return SRT_OK;
}
#endif

int srt_debug_lean_launches(srt_ctx* c, int64_t* launches) {
    if (!c || !launches) return fail(SRT_ERR_ARG, "null argument");
    *launches = c->lean_launches;
    return SRT_OK;
}

int srt_debug_lane_stats(srt_ctx* c, int mode, int64_t* out, int n) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    if (mode != 0 && mode != 1) return fail(SRT_ERR_ARG, "lane stats mode: 1 start, 0 read and stop");
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_async(c, nullptr);  // (the frames in flight were queued with the old pointer)
    if (rc) return rc;
    const size_t bytes = (size_t)SRT_MAX_DEPTHS * 2 * sizeof(unsigned long long);
    if (mode == 1) {
        if (!c->lane_stats) HIP_TRY(dalloc(&c->lane_stats, SRT_MAX_DEPTHS * 2));
        HIP_TRY(hipMemset(c->lane_stats, 0, bytes));
        return SRT_OK;
    }
    if (!out || n < 0 || n > SRT_MAX_DEPTHS) return fail(SRT_ERR_ARG, "lane stats: out[n][2], n <= SRT_MAX_DEPTHS");
    if (!c->lane_stats) return fail(SRT_ERR_ARG, "lane stats were not started");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->lane_stats, (size_t)n * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(c->lane_stats.reset());
    return SRT_OK;
}

int srt_debug_prefetch_counts(srt_ctx* c, int64_t* used, int64_t* queued) {
    if (!c || !used || !queued) return fail(SRT_ERR_ARG, "null argument");
    *used = c->pf_used;
    *queued = c->pf_queued;
    return SRT_OK;
}

int srt_debug_mt_residue(srt_ctx* c, int64_t* nonzero_words) {
    if (!c || !nonzero_words) return fail(SRT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    int rc = finish_async(c, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    int64_t nz = 0;
    std::vector<uint32_t> h;
    auto count = [&](const uint32_t* d, int64_t words) -> int {
        h.resize((size_t)words);
        HIP_TRY(hipMemcpy(h.data(), d, (size_t)words * 4, hipMemcpyDeviceToHost));
        for (uint32_t w : h) nz += w != 0u;
        return SRT_OK;
    };
    // (window 0 of a table holds a copy of the key, written by a plain store at every generation that
    // jumps -- never an XOR target -- and left there when no segment starts at the key: not counted)
    for (FrameSlot& f : c->slots)
        if (f.mt_win && f.mt_win.cap > rtmt::N && (rc = count(f.mt_win + rtmt::N, f.mt_win.cap - rtmt::N))) return rc;
    if (c->mt && (rc = count(mt_end_acc(c), rtmt::N + 1))) return rc;
    *nonzero_words = nz;
    return SRT_OK;
}

int srt_synchronize(srt_ctx* c) {
    if (!c) return fail(SRT_ERR_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    for (FrameSlot& f : c->slots)
        if (f.stream) HIP_TRY(hipStreamSynchronize(f.stream));
    return SRT_OK;
}

}  // extern "C"
