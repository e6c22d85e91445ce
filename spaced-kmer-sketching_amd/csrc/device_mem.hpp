// Device and pinned memory shared by the kernels' launchers and the C-ABI
// layer: pinned staging copies, the device block cache and grow-only scratch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace sks {

// Small host<->device copies through a per-thread pinned staging buffer,
// synchronous on `s` only. A pageable hipMemcpyAsync goes through the
// runtime's shared staging path: with two contexts building on two streams, one
// context's 1 KB count read-back waited for the other stream's scan
// (--hip-trace), serialising the concurrent builds.
hipError_t pinned_d2h(void* dst, const void* src, size_t bytes, hipStream_t s);
hipError_t pinned_h2d(void* dst, const void* src, size_t bytes, hipStream_t s);
// Staging buffers parked by exited threads, ready for reuse (diagnostics).
size_t pinned_pool_size();

// The process's device block cache (host_mem.cpp).  cache_alloc: a parked block
// of the current device of at least `bytes` (and at most 2x + 1 MB, so a small
// request does not pin a large block), or a fresh hipMalloc; *real is the
// block's true size, which every release reports back so the cache's limits
// are checked against what it holds.  cache_release parks a
// block the device is known to be done with (no event: the hot path, after a
// stream synchronisation); cache_release_after parks it to be handed out again
// only once `s` has passed the point of the call.  None waits for the device,
// except that blocks evicted beyond the cache limits are freed (hipFree waits).
hipError_t cache_alloc(void** p, size_t bytes, size_t* real);
void cache_release(void* p, size_t bytes);
void cache_release_after(void* p, size_t bytes, hipStream_t s);
void trim_device_cache(int device);

// The one owner of a cached device block.  Move-only.  A block still owned at
// destruction — an early error return, where work queued on it may not have
// run yet — goes back ordered after the current end of the stream it was bound
// to at allocation, so it is safe for any other context that is handed it.
// Allocation and release run with the block's device current.
class DevBlock {
 public:
  void* ptr = nullptr;
  size_t bytes = 0;  // the block's real size (at least what was asked for)

  DevBlock() = default;
  DevBlock(DevBlock&& o) noexcept { *this = std::move(o); }
  DevBlock& operator=(DevBlock&& o) noexcept {  // what this held leaves with `o`
    std::swap(ptr, o.ptr), std::swap(bytes, o.bytes), std::swap(stream_, o.stream_);
    return *this;
  }
  ~DevBlock() { release_after(stream_); }

  // every use of the block until it is released or handed to another owner
  // is expected on `bound`
  hipError_t alloc(size_t want, hipStream_t bound) {
    release_after(stream_);
    const hipError_t e = cache_alloc(&ptr, want, &bytes);
    if (e != hipSuccess) ptr = nullptr, bytes = 0;
    stream_ = bound;
    return e;
  }
  // the device is done with the block (the caller guarantees it)
  void release() {
    if (ptr) cache_release(ptr, bytes);
    ptr = nullptr, bytes = 0;
  }
  void release_after(hipStream_t s) {
    if (ptr) cache_release_after(ptr, bytes, s);
    ptr = nullptr, bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
  explicit operator bool() const { return ptr != nullptr; }

 private:
  hipStream_t stream_ = nullptr;
};

// Grow-only device scratch owned by a context.  With `owner` set (the
// context's stream; every use of the buffer is ordered on it) a grown buffer's
// old block goes back to the block cache after the stream's queued work, with
// no device-wide wait; without it, growth waits for the whole device.
// `bytes` is the real size of the block held.
struct Scratch {
  void* ptr = nullptr;
  size_t bytes = 0;
  const hipStream_t* owner = nullptr;
  hipError_t reserve(size_t n);
  void release();
};

}  // namespace sks
