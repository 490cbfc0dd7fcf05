// Move-only owners of what HIP hands out: device and pinned buffers, streams, events.  Each frees in its destructor and
// converts to the raw pointer or handle, so launches and copies read as with bare fields.  An owner does not wait for work
// that still uses what it frees: whoever holds it drains first and declares its streams after its memory.
// g_live_resources counts what the owners (and Allocs, prover_gpu.hip) hold: p2_debug_live_resources().
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <utility>

inline std::atomic<size_t> g_live_resources{0};

template <class T, bool Pinned>
class OwnedBuf {
    T* p = nullptr;
    size_t bytes_ = 0;

public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        std::swap(p, o.p), std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~OwnedBuf() { reset(); }
    operator T*() const { return p; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (!p) return;
        (void)(Pinned ? hipHostFree(p) : hipFree(p));
        g_live_resources--;
        p = nullptr, bytes_ = 0;
    }
    // Frees the old block first, then allocates exactly `bytes` / `count` elements; null and empty after a failure.
    hipError_t alloc_bytes(size_t bytes) {
        reset();
        const hipError_t e = Pinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) return p = nullptr, e;
        g_live_resources++;
        bytes_ = bytes;
        return e;
    }
    hipError_t alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
    // Grow-only, with a quarter of headroom so that a slowly growing batch does not reallocate every call.
    bool grow(size_t count) { return bytes_ >= count * sizeof(T) || alloc(count + count / 4) == hipSuccess; }
};
template <class T>
using DevBuf = OwnedBuf<T, false>;
template <class T>
using PinBuf = OwnedBuf<T, true>;

// A device buffer and its pinned host mirror, sized in bytes and growing together; both null after a failed grow.
template <class T>
struct Staged {
    DevBuf<T> d;
    PinBuf<T> h;
    bool grow(size_t bytes) {
        if (d.bytes() >= bytes) return true;
        d.reset(), h.reset();
        if (d.alloc_bytes(bytes + bytes / 4) == hipSuccess && h.alloc_bytes(bytes + bytes / 4) == hipSuccess) return true;
        d.reset();
        return false;
    }
};

template <class H, hipError_t (*Destroy)(H)>
class OwnedHandle {
protected:
    H h = nullptr;
    hipError_t adopt(hipError_t e) {
        if (e == hipSuccess) g_live_resources++;
        else h = nullptr;
        return e;
    }

public:
    OwnedHandle() = default;
    OwnedHandle(OwnedHandle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    OwnedHandle& operator=(OwnedHandle&& o) noexcept {
        std::swap(h, o.h);
        return *this;
    }
    ~OwnedHandle() { reset(); }
    operator H() const { return h; }
    void reset() {
        if (!h) return;
        (void)Destroy(h);
        g_live_resources--;
        h = nullptr;
    }
};
// create(flags): the default flags go through the plain create call, as the code always did
struct Stream : OwnedHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return reset(), adopt(flags == hipStreamDefault ? hipStreamCreate(&h) : hipStreamCreateWithFlags(&h, flags)); }
};
struct Event : OwnedHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags) { return reset(), adopt(flags == hipEventDefault ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, flags)); }
};
