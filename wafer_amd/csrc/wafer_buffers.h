// wafer_buffers.h -- owning holders for the host engine's device and pinned buffers (plain C++: no HIP header, so a host test
// instantiates them with a counting fake).  A memory policy is two static functions, alloc(void **, size_t bytes) -> int (0: made)
// and free(void *); a copy policy names its stream type and has copy(dst, src, bytes, to_device, stream) -> int.  Holders are
// move-only and free in their destructor.  None of them synchronises a stream: whoever remakes or grows a buffer that a copy or
// a launch in flight may still touch synchronises first, and says why there.
#pragma once
#include <cstddef>
#include <utility>

namespace wafer_eng __attribute__((visibility("hidden"))) {

// n elements of T, made once (make again: the first block goes back)
template <typename T, typename Mem>
class Array {
    T *p_ = nullptr;
    size_t n_ = 0;

public:
    Array() = default;
    Array(Array &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}   // (so no copies: move-only)
    Array &operator=(Array &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~Array() { reset(); }
    int make(size_t n)
    {
        reset();
        void *q = nullptr;
        const int rc = Mem::alloc(&q, sizeof(T) * n);
        if (rc != 0) return rc;
        p_ = static_cast<T *>(q);
        n_ = n;
        return 0;
    }
    void reset()
    {
        if (p_) Mem::free(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }   // where a kernel argument or a copy takes the pointer
    size_t size() const { return n_; }
    size_t bytes() const { return sizeof(T) * n_; }
};

// Grow-only: size() is at least the largest n reserved so far; contents are not carried over.  The new block is made first and
// the old one goes back only once it exists: a failed reserve leaves the old block and its size in place.
template <typename T, typename Mem>
struct GrowArray : Array<T, Mem> {
    int reserve(size_t n)
    {
        if (n <= this->size()) return 0;
        Array<T, Mem> wider;
        const int rc = wider.make(n);
        if (rc == 0) Array<T, Mem>::operator=(std::move(wider));
        return rc;
    }
};

// a device array and its pinned host mirror, n elements each; operator[] is the host side
template <typename T, typename Dev, typename Pin, typename Copy>
struct HostDev {
    Array<T, Dev> dev;
    Array<T, Pin> host;
    int make(size_t n)   // both or neither
    {
        int rc = dev.make(n);
        if (rc == 0 && (rc = host.make(n)) != 0) dev.reset();
        return rc;
    }
    T &operator[](size_t i) const { return host[i]; }
    // `count` elements from element `first` on, in stream order
    int upload(size_t count, typename Copy::stream s, size_t first = 0) const { return Copy::copy(dev + first, host + first, sizeof(T) * count, true, s); }
    int download(size_t count, typename Copy::stream s, size_t first = 0) const { return Copy::copy(host + first, dev + first, sizeof(T) * count, false, s); }
};

} // namespace wafer_eng
