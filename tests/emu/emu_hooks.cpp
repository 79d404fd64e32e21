// TEST INFRASTRUCTURE ONLY: what tests/test_stream_order.py reaches of the emulator's scheduler (dev_emu.h) through ctypes.
// Part of libfrbch_emu.so alone; the product library has no such symbols (tests/test_abi.py).
#include "frbch_internal.h"

#ifdef FRBCH_TEST_HOOKS
extern "C" {
// 0: call order (the default); 1: lazy; 2: others first.  Everything pending runs before the mode changes.
void frbch_test_emu_set_mode(int mode) { emu_set_mode(mode); }
int frbch_test_emu_mode(void) { return g_emu.mode.load(); }
void* frbch_test_emu_stream_create(void) {
  dev_stream_t s = nullptr;
  (void)dev_stream_create(&s);
  return s;
}
void frbch_test_emu_stream_destroy(void* s) { dev_stream_destroy(s); }
// hipMemcpyAsync from pageable host memory: the source is read now, the destination written when the op runs
void frbch_test_emu_memcpy_async(void* dst, const void* src, size_t n, void* s) { (void)dev_h2d(dst, src, n, s); }
void frbch_test_emu_stream_sync(void* s) { (void)dev_sync(s); }
void frbch_test_emu_drain(void) { emu_drain_all(); }
uint64_t frbch_test_emu_pending(void) { return emu_pending(); }
uint64_t frbch_test_emu_violations(void) {
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  return g_emu.violations;
}
// the n-th fallible device-layer call from now on (dev_malloc, dev_h2d, dev_d2h, dev_d2d, dev_memset*, dev_sync, dev_stream_create,
// dev_check_launch) returns failure, once; 0 disarms.  tests/test_post_failures.py walks every failure return with it.
void frbch_test_emu_fail_at(long n) { g_emu.fail_in.store(n > 0 ? n : 0); }
// dev_malloc blocks not yet freed (low 32 bits) and streams not yet destroyed (high 32 bits), in every scheduler mode
uint64_t frbch_test_emu_live(void) {
  return ((uint64_t)g_emu.live_blocks.load() & 0xFFFFFFFFull) | ((uint64_t)g_emu.live_streams.load() << 32);
}
// ops queued, since the last call with reset != 0, on the second stream of the chain whose front lane has `ncu_front` CUs (the
// low 16 bits of frbch_config.overlap, rounded down to 8): the stream of frbchi::Lanes itself, so that nothing else is counted --
// not the handles' own streams (frbch_open queues the identity rescale there), not another caller stream.  0 without such lanes.
uint64_t frbch_test_emu_queued_on_lane(int ncu_front, int reset) {
  frbchi::Lanes* ln = frbchi::get_lanes(0, ncu_front / 8 * 8);
  std::lock_guard<std::recursive_mutex> lk(g_emu.m);
  const uint64_t n = ln ? g_emu.queued[ln->b] : 0;
  if (reset) g_emu.queued.clear();
  return n;
}
}
#endif
