// Memory the C-ABI layer manages for itself: the per-thread pinned staging
// (pinned_d2h / pinned_h2d) and the process-wide device block cache.
#include <cstring>
#include <mutex>

#include "sks_ctx.hpp"

namespace sks {

namespace {
struct PinnedStage {
  void* p = nullptr;
  size_t bytes = 0;
};

// Host -> device copies of small metadata go through a pinned ring and do not
// wait: the bytes are copied into the ring at once (the caller's buffer may go
// away), the DMA is queued on `s`, and an event marks when that part of the
// ring may be rewritten.  A build used to synchronise its stream after every
// metadata upload (a dozen round trips for one 5 Mb genome).
struct RingUse {
  size_t off, len;
  int device;
  hipEvent_t ev;
};
struct PinnedRing {
  char* p = nullptr;
  size_t bytes = 0, head = 0;
  std::vector<RingUse> pending;
  std::vector<std::pair<int, hipEvent_t>> spare;  // (device, event) ready for reuse
};

// A thread's pinned staging (the d2h stage and the h2d ring).  Threads borrow
// one from a process-wide pool on first use and give it back when they exit,
// so the pinned memory is bounded by the largest number of threads staging at
// once, not by how many threads a long-running caller has started (the
// facade's parallel_* entry points start fresh threads on every call).  Pool
// entries are never freed: nothing touches HIP at thread or process exit
// (thread_local destructors of the main thread run before static ones, and
// could otherwise run after the HIP runtime is gone).
struct PinnedSlots {
  PinnedStage stage;
  PinnedRing ring;
};
std::mutex g_slots_mu;
std::vector<PinnedSlots*>* g_slots_pool = new std::vector<PinnedSlots*>();  // never freed

struct SlotsHandle {
  PinnedSlots* s = nullptr;
  PinnedSlots& get() {
    if (!s) {
      std::lock_guard<std::mutex> lk(g_slots_mu);
      if (!g_slots_pool->empty()) {
        s = g_slots_pool->back();
        g_slots_pool->pop_back();
      } else {
        s = new PinnedSlots();
      }
    }
    return *s;
  }
  ~SlotsHandle() {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_slots_mu);
    g_slots_pool->push_back(s);  // pending ring copies stay tracked by their events
  }
};
thread_local SlotsHandle t_slots;

hipError_t stage_reserve(PinnedStage& st, size_t bytes) {
  if (bytes <= st.bytes) return hipSuccess;
  if (st.p) (void)hipHostFree(st.p);
  st.p = nullptr;
  st.bytes = 0;
  size_t nb = std::max<size_t>(bytes, size_t(1) << 16);
  nb = (nb + 4095) & ~size_t(4095);
  hipError_t e = hipHostMalloc(&st.p, nb, hipHostMallocDefault);
  if (e == hipSuccess) st.bytes = nb;
  return e;
}

void ring_retire(PinnedRing& R, size_t i) {
  R.spare.emplace_back(R.pending[i].device, R.pending[i].ev);
  R.pending.erase(R.pending.begin() + (std::ptrdiff_t)i);
}
}  // namespace

size_t pinned_pool_size() {
  std::lock_guard<std::mutex> lk(g_slots_mu);
  return g_slots_pool->size();
}

hipError_t pinned_d2h(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return hipSuccess;
  PinnedStage& st = t_slots.get().stage;
  hipError_t e;
  if ((e = stage_reserve(st, bytes)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(st.p, src, bytes, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  std::memcpy(dst, st.p, bytes);
  return hipSuccess;
}

hipError_t pinned_h2d(void* dst, const void* src, size_t bytes, hipStream_t s) {
  if (!bytes) return hipSuccess;
  PinnedRing& R = t_slots.get().ring;
  hipError_t e;
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
  const size_t need = (bytes + 255) & ~size_t(255);
  // completed copies free their part of the ring
  for (size_t i = 0; i < R.pending.size();) {
    if (hipEventQuery(R.pending[i].ev) == hipSuccess) {
      ring_retire(R, i);
    } else {
      (void)hipGetLastError();  // hipErrorNotReady is not an error here
      ++i;
    }
  }
  if (need > R.bytes) {  // grow: drain, then reallocate
    for (const RingUse& u : R.pending)
      if ((e = hipEventSynchronize(u.ev)) != hipSuccess) return e;
    while (!R.pending.empty()) ring_retire(R, R.pending.size() - 1);
    if (R.p) (void)hipHostFree(R.p);
    R.p = nullptr;
    R.bytes = R.head = 0;
    const size_t nb = std::max<size_t>(4 * need, size_t(1) << 20);
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&R.p), nb, hipHostMallocDefault)) != hipSuccess)
      return e;
    R.bytes = nb;
  }
  if (R.head + need > R.bytes) R.head = 0;
  const size_t off = R.head;
  for (size_t i = 0; i < R.pending.size();) {  // copies still reading [off, off + need)
    const RingUse& u = R.pending[i];
    if (u.off < off + need && off < u.off + u.len) {
      if ((e = hipEventSynchronize(u.ev)) != hipSuccess) return e;
      ring_retire(R, i);
    } else {
      ++i;
    }
  }
  std::memcpy(R.p + off, src, bytes);
  if ((e = hipMemcpyAsync(dst, R.p + off, bytes, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  hipEvent_t ev = nullptr;
  for (size_t i = 0; i < R.spare.size(); ++i)
    if (R.spare[i].first == dev) {
      ev = R.spare[i].second;
      R.spare.erase(R.spare.begin() + (std::ptrdiff_t)i);
      break;
    }
  if (!ev && (e = hipEventCreateWithFlags(&ev, hipEventDisableTiming)) != hipSuccess) return e;
  if ((e = hipEventRecord(ev, s)) != hipSuccess) return e;
  R.pending.push_back({off, need, dev, ev});
  R.head = off + need;
  return hipSuccess;
}

// ---- device block cache -----------------------------------------------------------------
namespace {

// Device block cache for sketch arrays. hipFree of a sketch-sized array unmaps
// it (≈160 us for config 3's 24 MB set, measured with --hip-trace), more than
// the build's whole host-side post-processing; released arrays are parked here
// and handed to later builds instead. Blocks are plain hipMalloc memory.
struct CachedBlock {
  int device;
  void* p;
  size_t bytes;
  hipEvent_t ready;  // null, or the stream point after which the block is free
};
std::mutex g_cache_mu;
std::vector<CachedBlock> g_cache;  // most recently released last
constexpr size_t kCacheMaxBlocks = 16;
constexpr size_t kCacheMaxBytes = size_t(4) << 30;

size_t cache_bytes_locked() {
  size_t t = 0;
  for (const auto& b : g_cache) t += b.bytes;
  return t;
}

int current_device() {
  int d = 0;
  (void)hipGetDevice(&d);
  return d;
}

// An event at the current end of `s`, or null after waiting for `s` when none
// could be made: either way a block released with it is free once it is reused.
hipEvent_t release_point(hipStream_t s) {
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, s) != hipSuccess) {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
  }
  return ev;
}

void free_blocks(const std::vector<CachedBlock>& blocks) {
  for (const CachedBlock& b : blocks) {
    if (b.ready) (void)hipEventDestroy(b.ready);
    (void)hipFree(b.p);
  }
}

// Parks a block whose last use has completed (ready == null) or completes at
// the event `ready`; evicts the oldest blocks beyond the cache limits.
void park(void* p, size_t bytes, hipEvent_t ready) {
  std::vector<CachedBlock> evict;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    g_cache.push_back({current_device(), p, bytes, ready});
    while (g_cache.size() > kCacheMaxBlocks ||
           (g_cache.size() > 1 && cache_bytes_locked() > kCacheMaxBytes)) {
      evict.push_back(g_cache.front());
      g_cache.erase(g_cache.begin());
    }
  }
  free_blocks(evict);
}

}  // namespace

hipError_t cache_alloc(void** p, size_t bytes, size_t* real) {
  bytes = std::max<size_t>(bytes, 8);
  const int dev = current_device();
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    size_t best = g_cache.size();
    for (size_t i = 0; i < g_cache.size(); ++i) {
      CachedBlock& b = g_cache[i];
      if (b.device != dev || b.bytes < bytes || b.bytes > 2 * bytes + (size_t(1) << 20)) continue;
      if (b.ready) {  // stream-ordered release: reusable once its event has completed
        if (hipEventQuery(b.ready) != hipSuccess) {
          (void)hipGetLastError();  // hipErrorNotReady is not an error here
          continue;
        }
        (void)hipEventDestroy(b.ready);
        b.ready = nullptr;
      }
      if (best == g_cache.size() || b.bytes < g_cache[best].bytes) best = i;
    }
    if (best != g_cache.size()) {
      *p = g_cache[best].p;
      *real = g_cache[best].bytes;
      g_cache.erase(g_cache.begin() + best);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory) {  // give the cache back and retry once
    (void)hipGetLastError();
    trim_device_cache(dev);
    e = hipMalloc(p, bytes);
  }
  *real = e == hipSuccess ? bytes : 0;
  return e;
}

void cache_release(void* p, size_t bytes) {
  if (p) park(p, bytes, nullptr);
}

void cache_release_after(void* p, size_t bytes, hipStream_t s) {
  if (p) park(p, bytes, release_point(s));
}

void trim_device_cache(int device) {
  std::vector<CachedBlock> drop;
  {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (size_t i = 0; i < g_cache.size();) {
      if (g_cache[i].device == device) {
        drop.push_back(g_cache[i]);
        g_cache.erase(g_cache.begin() + i);
      } else {
        ++i;
      }
    }
  }
  free_blocks(drop);
}

}  // namespace sks
