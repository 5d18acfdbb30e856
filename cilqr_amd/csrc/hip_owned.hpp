// Private to cilqr_amd/csrc: move-only owners of the HIP resources a handle holds -- device memory, pinned host memory,
// events, streams.  Each is empty until made and releases what it holds in reset() or its destructor, with whatever
// device is current (cilqr_destroy makes it the handle's).  A creation that fails leaves its owner empty, so the next
// call that needs the resource tries again.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace cilqr {

// Device memory (hipMalloc / hipFree) or, Pinned, pinned host memory (hipHostMalloc / hipHostFree).
template <bool Pinned>
class hip_mem {
 public:
  hip_mem() = default;
  hip_mem(hip_mem&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  hip_mem& operator=(hip_mem o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }
  ~hip_mem() { reset(); }

  void* get() const { return p_; }
  template <typename T>
  T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
  void reset() {
    if (p_ == nullptr) return;
    if constexpr (Pinned) (void)hipHostFree(p_);
    else (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  // exactly `bytes` in place of what is held (`flags`: pinned memory only)
  hipError_t alloc(size_t bytes, unsigned flags = hipHostMallocDefault) {
    reset();
    void* p = nullptr;
    hipError_t e;
    if constexpr (Pinned) e = hipHostMalloc(&p, bytes, flags);
    else e = hipMalloc(&p, bytes);
    if (e == hipSuccess) p_ = p, bytes_ = bytes;
    return e;
  }
  // at least `need` bytes: a smaller block is freed first, then exactly `need` allocated (its contents are not kept).
  // `account` keeps the sum of such sizes for other threads to read; bytes() belongs to the thread that grows the block.
  hipError_t grow(size_t need, std::atomic<int64_t>* account = nullptr) {
    if (need <= bytes_) return hipSuccess;
    if (account) account->fetch_sub((int64_t)bytes_, std::memory_order_relaxed);
    const hipError_t e = alloc(need);
    if (e == hipSuccess && account) account->fetch_add((int64_t)need, std::memory_order_relaxed);
    return e;
  }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};
using dev_mem = hip_mem<false>;
using pinned_mem = hip_mem<true>;

// The blocks of ONE entry point that takes HOST or DEVICE arrays (staging.hpp: staged_call): the tables it builds on the
// host on their way to the device, with the landing place of its count; their device twin, with the count and any scratch
// behind them; the staging of HOST inputs and of HOST outputs.  All grow to the largest call and never shrink.
struct call_blocks {
  pinned_mem tab_host;
  dev_mem tab, in, out;
};

// A hipEvent_t or hipStream_t.
template <typename H, hipError_t (*Destroy)(H)>
class hip_handle {
 public:
  hip_handle() = default;
  hip_handle(hip_handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  hip_handle& operator=(hip_handle o) noexcept { std::swap(h_, o.h_); return *this; }
  ~hip_handle() { reset(); }

  H get() const { return h_; }
  void reset() {
    if (h_ != nullptr) (void)Destroy(h_);
    h_ = nullptr;
  }

 protected:
  template <typename Create>
  hipError_t make(Create create) {   // in place of what is held
    reset();
    H h = nullptr;
    const hipError_t e = create(&h);
    if (e == hipSuccess) h_ = h;
    return e;
  }

 private:
  H h_ = nullptr;
};

struct hip_event : hip_handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDisableTiming) {
    return make([flags](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); });
  }
  hipError_t create_timed() { return make([](hipEvent_t* e) { return hipEventCreate(e); }); }   // profiling
};

struct hip_stream : hip_handle<hipStream_t, hipStreamDestroy> {
  hipError_t create(unsigned flags) {
    return make([flags](hipStream_t* s) { return hipStreamCreateWithFlags(s, flags); });
  }
  hipError_t create(unsigned flags, int priority) {
    return make([=](hipStream_t* s) { return hipStreamCreateWithPriority(s, flags, priority); });
  }
};

}  // namespace cilqr
