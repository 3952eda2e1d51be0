// hc_scratch.h — the one owner of device and page-locked host memory in the library: every hipMalloc / hipHostMalloc and every free
// is in here (hc_host_alloc / hc_host_free apart, which hand memory to the caller).  Internal: nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

#include "../../include/hcedge.h"

namespace hc {
int set_last_error(int status, const std::string& what);  // thread-local text behind hc_last_error()
}

#define HC_HIP(call)                                                                                   \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return hc::set_last_error(HC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
    } while (0)

// A block of device memory — or, made with hipHostMalloc flags, of page-locked host memory — that frees itself.  A member of a context or
// a block is grow-only (allocating and freeing per call costs more than most of the kernels here); a local is a temporary of one call.
// The destructor does not pick a device and waits for no stream: whoever destroys one has the owner's device current and the work that
// uses the block behind it.
struct hc_scratch {
    void* p = nullptr;
    size_t cap = 0;
    bool host = false;                     // hipHostMalloc(flags) instead of hipMalloc
    unsigned flags = hipHostMallocMapped;  // (fixed when the block is made)
    hc_scratch() = default;
    explicit hc_scratch(unsigned host_flags) : host(true), flags(host_flags) {}
    hc_scratch(const hc_scratch&) = delete;
    hc_scratch& operator=(const hc_scratch&) = delete;
    hc_scratch(hc_scratch&& o) noexcept : p(o.p), cap(o.cap), host(o.host), flags(o.flags) {  // (the emptied block keeps its kind)
        o.p = nullptr;
        o.cap = 0;
    }
    hc_scratch& operator=(hc_scratch&& o) noexcept {
        if (this != &o) {
            release();
            host = o.host;
            flags = o.flags;
            std::swap(p, o.p);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    ~hc_scratch() { release(); }
    // a new block of exactly `bytes` in the old one's place (contents are not kept); empty when the runtime refuses
    hipError_t alloc(size_t bytes) {
        release();
        const hipError_t e = host ? hipHostMalloc(&p, bytes, flags) : hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    int ensure(size_t bytes) {  // grow-only, with an eighth of headroom; contents are not kept
        if (bytes <= cap) return HC_OK;
        HC_HIP(alloc(bytes + bytes / 8));
        return HC_OK;
    }
    int ensure_exact(size_t bytes) {  // the same without the headroom: a block sized once per read set
        if (bytes <= cap) return HC_OK;
        HC_HIP(alloc(bytes));
        return HC_OK;
    }
    // A new block of exactly `new_bytes` that keeps the first `live_bytes`: what `stream` still writes lands in the old block first, the
    // copy runs on it, and the old block is freed once the copy is through.
    int grow_keep(size_t new_bytes, size_t live_bytes, hipStream_t stream) {
        hc_scratch bigger;
        bigger.host = host;
        bigger.flags = flags;
        HC_HIP(hipStreamSynchronize(stream));
        HC_HIP(bigger.alloc(new_bytes));
        if (live_bytes && p) HC_HIP(hipMemcpyAsync(bigger.p, p, live_bytes, hipMemcpyDeviceToDevice, stream));
        HC_HIP(hipStreamSynchronize(stream));
        swap(bigger);
        return HC_OK;
    }
    void swap(hc_scratch& o) {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        std::swap(host, o.host);
        std::swap(flags, o.flags);
    }
    void release() {
        if (p) (void)(host ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as() const { return (T*)p; }
};
