// Move-only owners of the HIP resources the entry layer holds (se_engine in engine_impl.h, StreamResampler in k_resample.hip, the
// parked objects of parked.h): a member is released by its destructor, so the objects' teardown lists nothing.  Releases ignore their
// status - they run in destructors.
#pragma once
#include "common.h"
#include <utility>

namespace se {

template <typename T, hipError_t (*Free)(void*)>
class OwnedBuf {
  public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        std::swap(p_, o.p_);
        return *this;
    }
    ~OwnedBuf() { reset(); }
    void reset() {
        if (p_) (void)Free(p_);
        p_ = nullptr;
    }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

  protected:
    T* p_ = nullptr;
};

// n elements of device memory; alloc() on a buffer that holds memory releases it first
template <typename T>
struct DevBuf : OwnedBuf<T, hipFree> {
    void alloc(size_t n) {
        this->reset();
        SE_HIP(hipMalloc(reinterpret_cast<void**>(&this->p_), n * sizeof(T)));
    }
};

// ... of pinned host memory
template <typename T>
struct PinnedBuf : OwnedBuf<T, hipHostFree> {
    void alloc(size_t n) {
        this->reset();
        SE_HIP(hipHostMalloc(reinterpret_cast<void**>(&this->p_), n * sizeof(T), hipHostMallocDefault));
    }
};

// a handle that the first get() creates: an event without timing, a non-blocking stream
template <typename H, hipError_t (*Create)(H*, unsigned), unsigned Flags, hipError_t (*Destroy)(H)>
class LazyHandle {
  public:
    LazyHandle() = default;
    LazyHandle(const LazyHandle&) = delete;
    LazyHandle& operator=(const LazyHandle&) = delete;
    ~LazyHandle() {
        if (h_) (void)Destroy(h_);
    }
    H get() {
        if (!h_) SE_HIP(Create(&h_, Flags));
        return h_;
    }

  private:
    H h_ = nullptr;
};
using Event = LazyHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDisableTiming, hipEventDestroy>;
using OwnedStream = LazyHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamNonBlocking, hipStreamDestroy>;

}  // namespace se
