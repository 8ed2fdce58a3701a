// dev_buf.h -- memory a context's state owns: DevBuf<T> (hipMalloc) and PinnedBuf<T> (hipHostMalloc with the flags it was constructed
// with).  Move-only; the destructor frees.  ensure(count) grows only: a larger request frees the old block first and allocates the new
// one (contents are not kept), and a failed allocation leaves the buffer empty (capacity 0), so that the next call tries again.  Both
// convert to T*, so a kernel launch names the buffer as it named the raw pointer; a reinterpret_cast needs get().  No pool, no registry.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

template <class T, bool kPinned>
class OwnedBuf {
   public:
    explicit OwnedBuf(unsigned host_flags = 0) : flags_(host_flags) {}
    OwnedBuf(OwnedBuf&& o) noexcept : flags_(o.flags_) { swap(o); }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {      // (what this buffer held goes with `o`)
        swap(o);
        return *this;
    }
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    ~OwnedBuf() { release(); }
    hipError_t ensure(size_t count) {        // room for `count` elements
        if (count <= cap_) return hipSuccess;
        release();
        const hipError_t e = kPinned ? hipHostMalloc((void**)&p_, count * sizeof(T), flags_) : hipMalloc((void**)&p_, count * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = count;
        return e;
    }
    void release() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }

   private:
    void swap(OwnedBuf& o) {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        std::swap(flags_, o.flags_);
    }
    T* p_ = nullptr;
    size_t cap_ = 0;      // elements
    unsigned flags_;
};
template <class T>
using DevBuf = OwnedBuf<T, false>;
template <class T>
using PinnedBuf = OwnedBuf<T, true>;
