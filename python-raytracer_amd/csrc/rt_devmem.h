// rt_devmem.h -- the owners of device memory and two host helpers beside them: band_rows (a shard's rows),
// dalloc, DevBuf (one allocation with a capacity, released with its owner), DevList (allocations made and
// released together, with the copies in and out of a call), grid_for.  Host code only.
// A fragment of rt_kernels.hip, included in place and not compiled alone.  Before it: rt_trace_common.h
// (fail, BLOCK) and rt_device.h (shard_of_row).
namespace {

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

}  // namespace
