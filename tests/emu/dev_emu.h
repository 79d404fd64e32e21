// TEST INFRASTRUCTURE ONLY: host emulation of the device layer (see csrc/dev_hip.h) so that the
// CPU unit tests can run the engine's host logic and the generic kernels' index arithmetic
// without a GPU.  Never built into, or loaded by, the frb_baseband_amd package.
#ifndef FRBCH_DEV_EMU_H
#define FRBCH_DEV_EMU_H
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#define FRBCH_BACKEND_NAME "host-emulator(test-only)"
#define FRBCH_NO_FAST 1   /* the register-level gfx950 kernels are HIP only */
#define DEVFN static
#define KERNEL(name, PT) static void name(PT p, int bx, int by, int nthr, unsigned char* smem)
#define K_PROLOGUE ((void)0)
#define PHASE for (int tid = 0; tid < nthr; ++tid)
#define SYNC ((void)0)
#define FMUL_RN(a, b) ((a) * (b))   /* built with -ffp-contract=off */
#define FADD_RN(a, b) ((a) + (b))
#define LOAD_F4_STREAM(dst, ptr) ((dst) = *(const f4*)(ptr))
#define STORE_U32_STREAM(ptr, val) (*(uint32_t*)(ptr) = (uint32_t)(val))

static inline void emu_atomic_add_u64(unsigned long long* p, unsigned long long v) {
#pragma omp atomic
  *p += v;
}
static inline void emu_atomic_add_u32(unsigned int* p, unsigned int v) {
#pragma omp atomic
  *p += v;
}
static inline void emu_atomic_add_f64(double* p, double v) {
#pragma omp atomic
  *p += v;
}
#define ATOMIC_ADD_U64(ptr, v) emu_atomic_add_u64((unsigned long long*)(ptr), (unsigned long long)(v))
#define ATOMIC_ADD_U32(ptr, v) emu_atomic_add_u32((unsigned int*)(ptr), (unsigned int)(v))
#define ATOMIC_ADD_F64(ptr, v) emu_atomic_add_f64((double*)(ptr), (double)(v))
#define POST_NO_CONTRACT   /* built with -ffp-contract=off */

typedef void* dev_stream_t;
typedef int dev_event_t;

// ---- the scheduler ------------------------------------------------------------------------------------------------------------
// Mode 0 (the default): every call runs at once, in call order; streams and events are ignored.
// Modes 1 and 2 defer: every stream holds a queue of ops, nothing runs until the host asks (dev_sync, dev_event_sync, dev_free), and
// what then runs is a schedule a device may produce, chosen against the code under test:
//   1, lazy:         a host sync on `s` runs s's queue, and other streams only as far as s's waits demand (transitively); all else
//                    stays pending.  A consumer on the synced stream that lacks its wait runs before its producer.
//   2, others first: before s's queue runs, and again before each of its ops, every other stream runs as far as its own waits
//                    allow.  A side-lane op that lacks its wait on the caller's stream runs before the work it should follow.
// A wait depends on the event's most recent record at the time of the wait call, as hipStreamWaitEvent does; an event never recorded
// is satisfied.  One state for all translation units of the library (inline variable), behind one mutex (the host paths' threads).
struct EmuMarker {
  bool done = false;
  void* stream = nullptr;
};
struct EmuOp {
  std::function<void()> run;                 // empty: a wait
  std::shared_ptr<EmuMarker> wait;           // a wait: the record it depends on
  std::shared_ptr<EmuMarker> mark;           // a record: done once the op has run
  const char* lo = nullptr;                  // copies and memsets: the device bytes the op names (dev_free looks at them)
  const char* hi = nullptr;
  const char* lo2 = nullptr;
  const char* hi2 = nullptr;
};
struct EmuState {
  std::recursive_mutex m;
  std::atomic<int> mode{0};
  std::map<void*, std::deque<EmuOp>> q;      // by stream; the null stream is one of them
  std::map<int, std::shared_ptr<EmuMarker>> latest;   // event -> its most recent record
  std::map<const void*, size_t> sizes;       // allocations made while deferring
  std::map<void*, uint64_t> queued;          // ops ever queued, by stream
  uintptr_t next_stream = 0x1000;
  std::atomic<int> next_event{1};
  uint64_t violations = 0;
  std::atomic<long> fail_in{0};              // frbch_test_emu_fail_at: the fallible calls left before one fails; 0: disarmed
  std::atomic<long> live_blocks{0}, live_streams{0};   // dev_malloc blocks / streams not yet given back, in every mode
};
inline EmuState g_emu;
// a fallible call (dev_malloc, the copies, the memsets, dev_sync, dev_stream_create, dev_check_launch) asks first: true once, at
// the armed call, which then does nothing and returns failure
static inline bool emu_fail_now() {
  long n = g_emu.fail_in.load();
  while (n > 0 && !g_emu.fail_in.compare_exchange_weak(n, n - 1)) {}
  return n == 1;
}

static inline bool emu_deferred() { return g_emu.mode.load(std::memory_order_acquire) != 0; }
static inline void emu_run_until(void* s, const EmuMarker* target, int depth = 0);
// one op from the front of s's queue; a wait whose record has not run: demand it (run the recording stream up to it), or stop
static inline bool emu_step(void* s, bool demand, int depth) {
  std::deque<EmuOp>& q = g_emu.q[s];
  if (q.empty()) return false;
  if (q.front().wait && !q.front().wait->done) {
    if (!demand || depth > 64) return false;
    const std::shared_ptr<EmuMarker> w = q.front().wait;
    emu_run_until(w->stream, w.get(), depth + 1);
    if (!w->done) return false;
  }
  EmuOp op = std::move(g_emu.q[s].front());
  g_emu.q[s].pop_front();
  if (op.run) op.run();
  if (op.mark) op.mark->done = true;
  return true;
}
// s's queue as it stands now (target == nullptr), or up to and including the record `target`
static inline void emu_others_first(void* s);
static inline void emu_run_until(void* s, const EmuMarker* target, int depth) {
  size_t n = g_emu.q[s].size();
  const bool eager = depth == 0 && g_emu.mode.load() == 2;
  if (eager) emu_others_first(s);
  while ((target ? !target->done : n > 0) && emu_step(s, true, depth)) {
    if (eager) emu_others_first(s);      // (again behind every op of s: what it released runs at once)
    --n;
  }
}
// mode 2: every stream but `s` as far as its own waits allow
static inline void emu_others_first(void* s) {
  for (bool moved = true; moved;) {
    moved = false;
    std::vector<void*> ids;
    for (auto& kv : g_emu.q) ids.push_back(kv.first);
    for (void* o : ids)
      if (o != s)
        while (emu_step(o, false, 0)) moved = true;
  }
}
static inline void emu_drain_all() {
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  for (bool moved = true; moved;) {
    moved = false;
    std::vector<void*> ids;
    for (auto& kv : g_emu.q) ids.push_back(kv.first);
    for (void* o : ids)
      while (emu_step(o, true, 0)) moved = true;
  }
}
static inline uint64_t emu_pending() {
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  uint64_t n = 0;
  for (auto& kv : g_emu.q) n += kv.second.size();
  return n;
}
static inline void emu_set_mode(int mode) {
  emu_drain_all();
  g_emu.mode.store(mode, std::memory_order_release);
}
static inline void emu_push(void* s, EmuOp op) {
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  g_emu.q[s].push_back(std::move(op));
  g_emu.queued[s]++;
}
static inline void emu_push(void* s, std::function<void()> fn, const void* a = nullptr, size_t na = 0, const void* b = nullptr, size_t nb = 0) {
  EmuOp op;
  op.run = std::move(fn);
  op.lo = (const char*)a; op.hi = op.lo + na;
  op.lo2 = (const char*)b; op.hi2 = op.lo2 + nb;
  emu_push(s, std::move(op));
}

template <class PT>
static void emu_launch(void (*k)(PT, int, int, int, unsigned char*), long gx, long gy, int nthr, size_t lds, PT p) {
#pragma omp parallel
  {
    std::vector<unsigned char> smem(lds + 64);
#pragma omp for collapse(2) schedule(dynamic)
    for (long by = 0; by < gy; ++by)
      for (long bx = 0; bx < gx; ++bx) k(p, (int)bx, (int)by, nthr, smem.data());
  }
}
template <class PT>
static void emu_launch_on(void* s, void (*k)(PT, int, int, int, unsigned char*), long gx, long gy, int nthr, size_t lds, PT p) {
  if (!emu_deferred()) return emu_launch(k, gx, gy, nthr, lds, p);
  emu_push(s, [=]() { emu_launch(k, gx, gy, nthr, lds, p); });      // (the parameters by value, as a launch takes them)
}
#define DEV_LAUNCH(kern, gx, gy, nthr, lds, stream, params) \
  emu_launch_on((void*)(stream), kern, (long)(gx), (long)(gy), (int)(nthr), (size_t)(lds), params)

static inline const char* dev_last_error_string() { return "emulator"; }
static inline int dev_count() { return 1; }
static inline int dev_set(int) { return 0; }
static inline int dev_get() { return 0; }
static inline int dev_arch_ok(int, char* name, size_t cap, size_t* lds_limit) {
  snprintf(name, cap, "emu");
  *lds_limit = 160 * 1024;
  return 1;
}
template <class K>
static inline int dev_allow_lds(K, size_t) { return 0; }
static inline int dev_malloc(void** p, size_t n) {
  if (emu_fail_now()) return -1;
  *p = malloc(n ? n : 1);
  if (*p) g_emu.live_blocks++;
  if (*p && emu_deferred()) {
    std::lock_guard<std::recursive_mutex> lk(g_emu.m);
    g_emu.sizes[*p] = n ? n : 1;
  }
  return *p ? 0 : -1;
}
// (hipFree waits for the device: everything pending runs first; memory a pending copy or memset names counts as a violation)
static inline void dev_free(void* p) {
  if (p) g_emu.live_blocks--;
  if (p && emu_deferred()) {
    std::lock_guard<std::recursive_mutex> lk(g_emu.m);
    const auto it = g_emu.sizes.find(p);
    const char* lo = (const char*)p;
    const char* hi = lo + (it == g_emu.sizes.end() ? 1 : it->second);
    bool named = false;
    for (auto& kv : g_emu.q)
      for (auto& op : kv.second) named = named || (op.lo < hi && lo < op.hi) || (op.lo2 < hi && lo < op.hi2);
    if (named) g_emu.violations++;
    if (it != g_emu.sizes.end()) g_emu.sizes.erase(it);
    emu_drain_all();
  }
  free(p);
}
static inline int dev_h2d(void* d, const void* h, size_t n, dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) { memcpy(d, h, n); return 0; }
  auto src = std::make_shared<std::vector<unsigned char>>((const unsigned char*)h, (const unsigned char*)h + n);   // the host source as it is now
  emu_push(s, [=]() { memcpy(d, src->data(), n); }, d, n);
  return 0;
}
static inline int dev_d2h(void* h, const void* d, size_t n, dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) { memcpy(h, d, n); return 0; }
  emu_push(s, [=]() { memcpy(h, d, n); }, d, n);
  return 0;
}
static inline int dev_d2d(void* d, const void* s_, size_t n, dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) { memmove(d, s_, n); return 0; }
  emu_push(s, [=]() { memmove(d, s_, n); }, d, n, s_, n);
  return 0;
}
static inline void emu_copy2d(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height) {
  for (size_t r = 0; r < height; ++r) memmove((char*)d + r * dpitch, (const char*)s + r * spitch, width);
}
static inline int dev_copy2d(void* d, size_t dpitch, const void* s_, size_t spitch, size_t width, size_t height, dev_stream_t s) {
  if (!emu_deferred()) { emu_copy2d(d, dpitch, s_, spitch, width, height); return 0; }
  const size_t nd = height ? (height - 1) * dpitch + width : 0, ns = height ? (height - 1) * spitch + width : 0;
  emu_push(s, [=]() { emu_copy2d(d, dpitch, s_, spitch, width, height); }, d, nd, s_, ns);
  return 0;
}
static inline int dev_memset(void* d, int v, size_t n, dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) { memset(d, v, n); return 0; }
  emu_push(s, [=]() { memset(d, v, n); }, d, n);
  return 0;
}
static inline void emu_memset32(void* d, uint32_t v, size_t nwords) {
  for (size_t i = 0; i < nwords; ++i) ((uint32_t*)d)[i] = v;
}
static inline int dev_memset32(void* d, uint32_t v, size_t nwords, dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) { emu_memset32(d, v, nwords); return 0; }
  emu_push(s, [=]() { emu_memset32(d, v, nwords); }, d, nwords * 4);
  return 0;
}
static inline int dev_sync(dev_stream_t s) {
  if (emu_fail_now()) return -1;
  if (!emu_deferred()) return 0;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  emu_run_until(s, nullptr);
  return 0;
}
// Mode 0 hands out the one id it always did, the deferring modes distinct ones.  A stream outlives the mode that made it: the
// lanes of frbch_stream.cpp are kept for the life of the process, so the second stream of a chain is id 1 in every mode if a
// mode-0 run made it first (the stream-order tests always run mode 0 first) and a distinct id otherwise.  Either way it differs
// from every stream a deferring mode hands out (they start at 0x1010), which is all the scheduler needs: queues go by id.
static inline int dev_stream_create(dev_stream_t* s) {
  if (emu_fail_now()) return -1;
  g_emu.live_streams++;
  *s = (void*)1;
  if (emu_deferred()) {   // distinct streams
    std::lock_guard<std::recursive_mutex> lk(g_emu.m);
    *s = (void*)(g_emu.next_stream += 16);
  }
  return 0;
}
// (hipStreamDestroy lets the stream's work complete: so does this, and counts the caller's omission)
static inline void dev_stream_destroy(dev_stream_t s) {
  g_emu.live_streams--;
  if (!emu_deferred()) return;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  const auto it = g_emu.q.find(s);
  if (it == g_emu.q.end()) return;
  if (!it->second.empty()) {
    g_emu.violations++;
    emu_run_until(s, nullptr);
  }
  if (g_emu.q[s].empty()) g_emu.q.erase(s);
}
static inline int dev_cu_count(int) { return 256; }
// (events are distinct in every mode; mode 0 never looks at them)
static inline int dev_event_create_sync(int* e) { *e = g_emu.next_event.fetch_add(1); return 0; }
static inline void dev_event_record(dev_event_t e, dev_stream_t s) {
  if (!emu_deferred()) return;
  EmuOp op;
  op.run = []() {};
  op.mark = std::make_shared<EmuMarker>();
  op.mark->stream = s;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  g_emu.latest[e] = op.mark;
  emu_push(s, std::move(op));
}
static inline int dev_stream_wait(dev_stream_t s, int e) {
  if (!emu_deferred()) return 0;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  const auto it = g_emu.latest.find(e);
  if (it == g_emu.latest.end() || it->second->done) return 0;
  EmuOp op;
  op.wait = it->second;
  emu_push(s, std::move(op));
  return 0;
}
static inline int dev_event_sync(int e) {
  if (!emu_deferred()) return 0;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  const auto it = g_emu.latest.find(e);
  if (it == g_emu.latest.end() || it->second->done) return 0;
  const std::shared_ptr<EmuMarker> w = it->second;
  emu_run_until(w->stream, w.get());
  return w->done ? 0 : -1;
}
static inline int dev_check_launch() { return emu_fail_now() ? -1 : 0; }
static inline int dev_host_alloc(void** p, size_t n) { *p = malloc(n); return *p ? 0 : -1; }
static inline void dev_host_free(void* p) { free(p); }
static inline int dev_event_create(dev_event_t* e) { return dev_event_create_sync(e); }
static inline void dev_event_destroy(dev_event_t e) {
  if (!emu_deferred()) return;
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  g_emu.latest.erase(e);     // (a wait already queued keeps its record)
}
static inline float dev_event_ms(dev_event_t, dev_event_t b) { (void)dev_event_sync(b); return 0.f; }
#endif
