// The only device memory the library owns: the scratch of the conv kernels (scratch_get in conv_args.h: stream-K slots and flags
// of conv_tile.hip, partial tiles of conv_wgrad.hip and wgrad_halo.hip) and its release (u2_release_scratch).  Host code only.
#include <mutex>
#include <vector>

#include "common.h"
#include "conv_args.h"
#include "u2seg_hip.h"

namespace u2conv {

namespace {
struct ScratchEnt { int device; hipStream_t stream; int kind; void* buf; size_t cap; };
ScratchEnt g_scratch[128];
int g_scratch_used = 0;
std::mutex g_scratch_mu;
// blocks replaced by a larger one: another host thread (main / autograd) may hold the old pointer between scratch_get's return
// and its launch, which no stream synchronisation here can see - so an outgrown block is only FREED by u2_release_scratch().
// Growth is geometric (x 1.5) under a per-kind limit: the retired blocks of an entry sum to less than twice its final size.
struct RetiredEnt { int device; void* buf; };
std::vector<RetiredEnt> g_retired;
}  // namespace

void* scratch_get(int kind, hipStream_t s, size_t need_bytes, size_t limit_bytes, bool zero_on_alloc) {
  if (need_bytes == 0 || need_bytes > limit_bytes) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(g_scratch_mu);
  ScratchEnt* e = nullptr;
  for (int i = 0; i < g_scratch_used; ++i)
    if (g_scratch[i].device == dev && g_scratch[i].stream == s && g_scratch[i].kind == kind) { e = &g_scratch[i]; break; }
  if (e && e->cap >= need_bytes) return e->buf;
  if (!e) {
    if (g_scratch_used == 128) return nullptr;
    e = &g_scratch[g_scratch_used];
    *e = ScratchEnt{dev, s, kind, nullptr, 0};
  }
  // grow: 1.5 x the old block at least (a sequence of slowly growing launches must not reallocate every time), 2 MB granules
  size_t cap = need_bytes > e->cap + e->cap / 2 ? need_bytes : e->cap + e->cap / 2;
  cap = (cap + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
  if (cap > limit_bytes) cap = limit_bytes;
  if (e->buf) {
    g_retired.push_back(RetiredEnt{dev, e->buf});   // freed by u2_release_scratch (see g_retired)
    e->buf = nullptr; e->cap = 0;
  }
  void* p = nullptr;
  if (hipMalloc(&p, cap) != hipSuccess) return nullptr;
  if (zero_on_alloc && hipMemset(p, 0, cap) != hipSuccess) { (void)hipFree(p); return nullptr; }
  e->buf = p; e->cap = cap;
  if (e == &g_scratch[g_scratch_used]) ++g_scratch_used;
  return p;
}
}  // namespace u2conv

extern "C" int u2_release_scratch(void) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  std::lock_guard<std::mutex> lock(u2conv::g_scratch_mu);
  int freed = 0;
  for (int i = 0; i < u2conv::g_scratch_used; ++i) {
    u2conv::ScratchEnt& e = u2conv::g_scratch[i];
    if (!e.buf) continue;
    (void)hipSetDevice(e.device);
    (void)hipStreamSynchronize(e.stream);
    (void)hipFree(e.buf);
    ++freed;
  }
  u2conv::g_scratch_used = 0;
  for (const u2conv::RetiredEnt& r : u2conv::g_retired) {
    (void)hipSetDevice(r.device);
    (void)hipDeviceSynchronize();
    (void)hipFree(r.buf);
    ++freed;
  }
  u2conv::g_retired.clear();
  (void)hipSetDevice(cur);
  return freed;
}
