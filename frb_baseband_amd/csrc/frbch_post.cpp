// libfrbch: behind and in front of the filterbank -- incoherent dedispersion, fold, corner turn; kernels in
// kernels_post.inc / kernels_post_fast.inc, which this translation unit alone sees (frbch_internal.h lists the units).
// C-ABI entry points behind the filterbank (include/frbch.h, "after the filterbank"): incoherent dedispersion of SIGPROC
// rows with PRESTO's prepdata / prepsubband options as the reference passes them (process_vdif.py:202-229) and the phase
// fold that base2fil.sh:474 delegates to dspsr.  A stage reads check, plan, launch; what it holds on the device belongs to a
// PostScope (_device) or a HostStage (_host), which give it back on every return.
#include "frbch_internal.h"

using namespace frbchi;

#include <chrono>
#include <limits>
#include <memory>
#include <new>
#include <system_error>
#include <thread>

#include "kernels_post.inc"
#ifndef FRBCH_NO_FAST
#include "kernels_post_fast.inc"
#endif

namespace {

struct PostErr {
  char* buf;
  size_t cap;
  int fail(int code, const std::string& msg) const {
    if (buf && cap) snprintf(buf, cap, "%s", msg.c_str());
    return code;
  }
};

// Device time of a stage for frbch_candidates_*: while `tl_stage_ms` points somewhere (this thread is inside such a call), a
// _device entry point adds the time between two events on its own stream -- its first and its last work -- to it.
thread_local double* tl_stage_ms = nullptr;
struct StageClock {
  dev_stream_t s = 0;
  dev_event_t a, b;
  bool on = false;
  StageClock() = default;
  explicit StageClock(dev_stream_t stream) { start(stream); }
  void start(dev_stream_t stream) {
    s = stream;
    if (!tl_stage_ms || dev_event_create(&a) != 0) return;
    if (dev_event_create(&b) != 0) { dev_event_destroy(a); return; }
    dev_event_record(a, s);
    on = true;
  }
  void finish() {                       // before the stream goes
    if (!on) return;
    on = false;
    dev_event_record(b, s);
    *tl_stage_ms += (double)dev_event_ms(a, b);
    dev_event_destroy(a);
    dev_event_destroy(b);
  }
};

// a device-layer call of a _device entry point that fails ends the call; its PostScope gives back what the call holds
#define POST_DEV(expr, what) do { if ((expr) != 0) return e.fail(FRBCH_E_DEVICE, std::string(what) + ": " + dev_last_error_string()); } while (0)

// What one _device call holds on the device: its non-blocking stream (s == 0: it could not be made), the clock of its stage
// (PostScope(false): none; it starts here, so a stage makes its scope where its device work begins) and what alloc() hands out.
struct PostScope {
  dev_stream_t s = 0;
  StageClock clk;
  std::vector<void*> held;
  explicit PostScope(bool clock = true) {
    if (dev_stream_create(&s) != 0) s = 0;
    else if (clock) clk.start(s);
  }
  PostScope(const PostScope&) = delete; PostScope& operator=(const PostScope&) = delete;
  template <class T> int alloc(T** p, size_t bytes) {
    held.push_back(nullptr);            // (a std::bad_alloc before the block exists, not with it in hand)
    if (dev_malloc(&held.back(), bytes) != 0) { held.pop_back(); return -1; }
    *p = (T*)held.back();
    return 0;
  }
  template <class T> void drop(T*& p) {   // a buffer that is done with before the call is: freed now, and forgotten
    held.erase(std::remove(held.begin(), held.end(), (void*)p), held.end());
    dev_free((void*)p);
    p = nullptr;
  }
  // On every return, or before it where the host has work left: the clock first, then the blocks in the order they were
  // allocated, then the stream.  The order is not cosmetic: StageClock::finish records its second event, frbch_candidates_* report
  // the difference as device time, and hipFree waits for the device -- a clock finished behind the frees would add them to it.
  void release() {                      // (a second call finds nothing left)
    clk.finish();
    for (void* q : held) dev_free(q);
    held.clear();
    if (s) dev_stream_destroy(s);
    s = 0;
  }
  ~PostScope() { release(); }
};

// The buffers of a _host twin: device copies of the caller's host arrays, allocated as they are named (after the first failure
// `failed` is set and nothing more is allocated).  upload() / download() put every `in` / `out` buffer on one stream -- the NULL
// stream, unless the caller has its own -- with one sync behind them.  The destructor frees, in that order, what drop() has not.
struct HostStage {
  enum { kIn = 1, kOut = 2, kCap = 20 };
  struct Buf { void* host; void* dev; size_t bytes; int dir; };
  Buf b[kCap];
  int n = 0;
  bool failed = false;
  HostStage() = default; HostStage(const HostStage&) = delete; HostStage& operator=(const HostStage&) = delete;
  void* add(int dir, const void* host, size_t bytes) {
    void* d = nullptr;
    if (failed || n == kCap || dev_malloc(&d, bytes) != 0) { failed = true; return nullptr; }
    b[n++] = Buf{(void*)host, d, bytes, host ? dir : 0};                       // (no host array: nothing to copy)
    return d;
  }
  template <class T> T* in(const T* host, size_t bytes) { return (T*)add(kIn, host, bytes); }
  template <class T> T* out(T* host, size_t bytes) { return (T*)add(kOut, host, bytes); }
  template <class T> T* inout(T* host, size_t bytes) { return (T*)add(kIn | kOut, host, bytes); }
  void* scratch(size_t bytes) { return add(0, nullptr, bytes); }                  // the caller copies by hand
  int upload(dev_stream_t s = 0) {
    for (int i = 0; i < n; ++i)
      if ((b[i].dir & kIn) && dev_h2d(b[i].dev, b[i].host, b[i].bytes, s) != 0) return -1;
    return dev_sync(s);
  }
  int download(dev_stream_t s = 0) {          // (no `out` buffer: no sync either)
    bool any = false;
    for (int i = 0; i < n; ++i)
      if (b[i].dir & kOut) { any = true; if (dev_d2h(b[i].host, b[i].dev, b[i].bytes, s) != 0) return -1; }
    return any ? dev_sync(s) : 0;
  }
  // the skeleton of a _host twin: the uploads, the _device twin, the downloads; the texts of the three failures
  template <class F> int run(const PostErr& e, const char* nomem, const char* up, const char* down, F device_twin) {
    if (failed) return e.fail(FRBCH_E_NOMEM, nomem);
    if (upload() != 0) return e.fail(FRBCH_E_DEVICE, up);
    const int rc = device_twin();
    return !rc && download() != 0 ? e.fail(FRBCH_E_DEVICE, down) : rc;
  }
  void drop(const void* p) {                  // a buffer that is done with before the call is
    for (int i = 0; i < n; ++i)
      if (b[i].dev == p) { dev_free(b[i].dev); b[i] = Buf{nullptr, nullptr, 0, 0}; }
  }
  ~HostStage() { for (int i = 0; i < n; ++i) dev_free(b[i].dev); }
};

int post_check_device(int device, const PostErr& e) {
  if (device < 0 || device >= dev_count()) return e.fail(FRBCH_E_DEVICE, "no such GPU (there is no CPU fallback)");
  return FRBCH_OK;
}

// the tests every entry point that takes rows begins with (rfi_check goes on from here with its own)
int post_check_layout(const frbch_fil_desc* f, const PostErr& e) {
  if (!f || f->size != sizeof(frbch_fil_desc)) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size");
  if (f->nchan < 1 || f->nifs < 1 || f->product >= f->nifs) return e.fail(FRBCH_E_ARG, "bad nchan / nifs / product");
  if (f->nbits != 8 && f->nbits != 16 && f->nbits != 32) return e.fail(FRBCH_E_ARG, "nbits must be 8, 16 or 32 (float)");
  return FRBCH_OK;
}

int post_check_fil(const frbch_fil_desc* f, uint64_t nrows, const PostErr& e) {
  const int rc = post_check_layout(f, e);
  if (rc) return rc;
  if (!(f->tsamp_s > 0) || f->foff_mhz == 0.0 || !(f->fch1_mhz > 0)) return e.fail(FRBCH_E_ARG, "bad tsamp / fch1 / foff");
  if (!nrows) return e.fail(FRBCH_E_ARG, "no rows");
  return FRBCH_OK;
}

size_t post_rows_bytes(const frbch_fil_desc* fil, uint64_t nrows) { return (size_t)nrows * fil->nifs * fil->nchan * (size_t)(fil->nbits / 8); }

// the fields PostParams, FoldpParams, CutParams and RfiParams share; everything else zero
template <class P> P post_params(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows) {
  P p;
  memset(&p, 0, sizeof p);
  p.rows = (decltype(p.rows))d_rows;
  p.nrows = nrows;
  p.nchan = (int)fil->nchan; p.nifs = (int)fil->nifs; p.nbits = fil->nbits;
  return p;
}

#ifndef FRBCH_NO_FAST
// a kernel with dynamic LDS: the permission for `lds` bytes, then the launch; != 0: the permission was refused
template <class K, class P> int launch_lds(K kern, dim3 grid, dim3 block, size_t lds, dev_stream_t s, const P& p) {
  if (dev_allow_lds(kern, lds) != 0) return -1;
  hipLaunchKernelGGL(kern, grid, block, lds, s, p);
  return 0;
}

template <int B> int launch_dedisp_tiled(bool flagged, bool zerodm, dim3 grid, size_t lds, dev_stream_t s, const PostParams& p) {
  if (flagged && zerodm) return launch_lds(fast::frbch_post_dedisp_tiled<B, true, true>, grid, dim3(256), lds, s, p);
  if (flagged) return launch_lds(fast::frbch_post_dedisp_tiled<B, true, false>, grid, dim3(256), lds, s, p);
  if (zerodm) return launch_lds(fast::frbch_post_dedisp_tiled<B, false, true>, grid, dim3(256), lds, s, p);
  return launch_lds(fast::frbch_post_dedisp_tiled<B, false, false>, grid, dim3(256), lds, s, p);
}
#endif

// delay of channel c relative to the highest channel frequency of the file, seconds (DSPSR / PRESTO constant 1/2.41e-4)
double post_delay_s(const frbch_fil_desc* f, double dm, uint32_t c) {
  const double fc = f->fch1_mhz + (double)c * f->foff_mhz;
  const double f_last = f->fch1_mhz + (double)(f->nchan - 1) * f->foff_mhz;
  const double fhi = f->foff_mhz < 0 ? f->fch1_mhz : f_last;
  return dm / kDmDispersion * (1.0 / (fc * fc) - 1.0 / (fhi * fhi));
}

std::vector<int32_t> post_delays(const frbch_fil_desc* f, const double* dms, uint32_t ndm, int64_t* maxd) {
  std::vector<int32_t> d((size_t)ndm * f->nchan);
  *maxd = 0;
  for (uint32_t i = 0; i < ndm; ++i)
    for (uint32_t c = 0; c < f->nchan; ++c) {
      const double s = post_delay_s(f, dms[i], c) / f->tsamp_s;
      const int64_t n = (int64_t)(s + 0.5);                 // PRESTO rounds the bin delay the same way
      d[(size_t)i * f->nchan + c] = (int32_t)n;
      *maxd = std::max<int64_t>(*maxd, n);
    }
  return d;
}

constexpr uint64_t kPostChunkRows = 4096;

// Which dedispersion kernel a call takes -- the one decision behind frbch_dedisperse_device's launch and
// frbch_dedisperse_kernel's answer.  true = the LDS-tiled kernel (kernels_post_fast.inc): whole 64-byte channel tiles,
// 16-byte pieces of every row (only the ADDRESS of d_rows is examined), and every (DM group, channel tile) fits its rows into
// the LDS; *range then holds [DM group][channel tile] (smallest delay, rows spanned beyond the time tile).  The emulator
// build has no such kernel: false.
bool post_dedisp_tiled(const frbch_fil_desc* fil, const void* d_rows, const std::vector<int32_t>& delays, uint32_t ndm,
                       std::vector<int32_t>* range) {
#ifndef FRBCH_NO_FAST
  const int bpv = fil->nbits / 8, ct = 64 / bpv;
  if (fil->nchan % ct != 0 || ((uintptr_t)d_rows % 16) != 0 || ((size_t)fil->nchan * bpv) % 16 != 0) return false;
  const int nct = (int)fil->nchan / ct, ngrp = (int)((ndm + fast::kDedND - 1) / fast::kDedND);
  range->assign((size_t)ngrp * nct * 2, 0);
  for (int g = 0; g < ngrp; ++g)
    for (int k = 0; k < nct; ++k) {
      int32_t lo = INT32_MAX, hi = 0;
      for (uint32_t d = (uint32_t)g * fast::kDedND; d < std::min<uint32_t>(ndm, (uint32_t)(g + 1) * fast::kDedND); ++d)
        for (int c = k * ct; c < (k + 1) * ct; ++c) {
          const int32_t v = delays[(size_t)d * fil->nchan + c];
          lo = std::min(lo, v);
          hi = std::max(hi, v);
        }
      (*range)[((size_t)g * nct + k) * 2] = lo;
      (*range)[((size_t)g * nct + k) * 2 + 1] = hi - lo;
      if (fast::kDedTT + (hi - lo) > fast::kDedRowsCap) return false;
    }
  return true;
#else
  (void)fil; (void)d_rows; (void)delays; (void)ndm; (void)range;
  return false;
#endif
}

// The clip and zero-DM pre-pass of frbch_dedisperse_* on the stream of `ps`: S[t] into p.rowsum (the caller's, [nrows]) where
// it is needed, then the clip -- flags, replacement values and S[t] of the clipped rows, in blocks `ps` holds; p.flagged and
// p.repl are set when a row clips.  It depends on the rows alone, not on the DMs: frbch_bandsearch_* run it once for all batches.
int post_dedisp_prepass(PostScope& ps, const PostErr& e, const frbch_fil_desc* fil, uint64_t nrows, uint32_t zerodm,
                        double clip_sigma, PostParams& p, uint64_t* nclip) {
  const dev_stream_t s = ps.s;
  const uint64_t nchunk = (nrows + kPostChunkRows - 1) / kPostChunkRows;
  double *d_colsum = nullptr, *d_repl = nullptr;
  uint8_t* d_flag = nullptr;
  uint64_t nflag = 0;
  if (clip_sigma > 0.0 || zerodm) {
    DEV_LAUNCH(frbch_post_rowsum, (nrows + 255) / 256, 1, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch rowsum");
  }
  if (clip_sigma > 0.0) {
    // time-domain clip on the zero-DM series S[t] (the sum over channels): two rounds of mean / sigma, the second without
    // the samples the first one flagged; a flagged time sample reads as the channel means of the unflagged ones
    std::vector<double> S(nrows);
    POST_DEV(dev_d2h(S.data(), p.rowsum, nrows * sizeof(double), s), "download row sums");
    POST_DEV(dev_sync(s), "sync");
    std::vector<uint8_t> flag(nrows, 0);
    for (int round = 0; round < 2; ++round) {
      double s1 = 0.0, s2 = 0.0;
      uint64_t n = 0;
      for (uint64_t t = 0; t < nrows; ++t)
        if (!flag[t]) { s1 += S[t]; s2 += S[t] * S[t]; ++n; }
      if (!n) break;
      const double mean = s1 / (double)n;
      const double var = s2 / (double)n - mean * mean;
      const double sig = var > 0.0 ? sqrt(var) : 0.0;
      const double lim = clip_sigma * sig;
      for (uint64_t t = 0; t < nrows; ++t) flag[t] = (uint8_t)(fabs(S[t] - mean) > lim ? 1 : 0);
    }
    for (uint64_t t = 0; t < nrows; ++t) nflag += flag[t];
    if (nflag && nflag < nrows) {
      POST_DEV(ps.alloc(&d_flag, nrows), "hipMalloc");
      POST_DEV(dev_h2d(d_flag, flag.data(), nrows, s), "upload flags");
      POST_DEV(ps.alloc(&d_colsum, nchunk * fil->nchan * sizeof(double)), "hipMalloc");
      POST_DEV(ps.alloc(&d_repl, fil->nchan * sizeof(double)), "hipMalloc");
      p.flagged = d_flag;
      p.colsum = d_colsum;
      DEV_LAUNCH(frbch_post_colsum, (fil->nchan + 255) / 256, nchunk, 256, 0, s, p);
      POST_DEV(dev_check_launch(), "launch colsum");
      std::vector<double> part(nchunk * fil->nchan), repl(fil->nchan);
      POST_DEV(dev_d2h(part.data(), d_colsum, part.size() * sizeof(double), s), "download column sums");
      POST_DEV(dev_sync(s), "sync");
      const double ngood = (double)(nrows - nflag);
      for (uint32_t c = 0; c < fil->nchan; ++c) {
        double m = 0.0;
        for (uint64_t k = 0; k < nchunk; ++k) m += part[k * fil->nchan + c];
        repl[c] = fil->nbits == 32 ? m / ngood : floor(m / ngood + 0.5);     // integer rows stay integer
      }
      POST_DEV(dev_h2d(d_repl, repl.data(), repl.size() * sizeof(double), s), "upload replacements");
      p.repl = d_repl;
      if (zerodm) {
        DEV_LAUNCH(frbch_post_rowsum, (nrows + 255) / 256, 1, 256, 0, s, p);   // S[t] of the clipped rows
        POST_DEV(dev_check_launch(), "launch rowsum");
      }
    } else {
      nflag = 0;
    }
  }
  *nclip = nflag;
  return FRBCH_OK;
}

}  // namespace

extern "C" long frbch_dedisperse_nout(const frbch_fil_desc* fil, uint64_t nrows, const double* dms, uint32_t ndm) {
  PostErr e{nullptr, 0};
  if (post_check_fil(fil, nrows, e) || !dms || !ndm) return FRBCH_E_ARG;
  for (uint32_t i = 0; i < ndm; ++i)
    if (!(dms[i] >= 0.0) || !(dms[i] < 1.0e5)) return FRBCH_E_ARG;
  int64_t maxd = 0;
  (void)post_delays(fil, dms, ndm, &maxd);
  return (int64_t)nrows > maxd ? (long)((int64_t)nrows - maxd) : 0;
}

extern "C" int frbch_dedisperse_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms,
                                       uint32_t ndm) {
  if (!d_rows || frbch_dedisperse_nout(fil, nrows, dms, ndm) <= 0) return FRBCH_E_ARG;   // what frbch_dedisperse_device refuses
  int64_t maxd = 0;
  const std::vector<int32_t> delays = post_delays(fil, dms, ndm, &maxd);
  std::vector<int32_t> range;
  return post_dedisp_tiled(fil, d_rows, delays, ndm, &range) ? 1 : 0;
}

extern "C" int frbch_dedisperse_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms,
                                       uint32_t ndm, uint32_t zerodm, double clip_sigma, int device, float* d_out,
                                       uint64_t nout, uint64_t* nclipped, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!d_rows || !d_out || !dms || !ndm) return e.fail(FRBCH_E_ARG, "null argument");
  const long want = frbch_dedisperse_nout(fil, nrows, dms, ndm);
  if (want <= 0) return e.fail(FRBCH_E_ARG, "the largest dispersion delay exceeds the data");
  if ((uint64_t)want != nout) return e.fail(FRBCH_E_CAPACITY, "nout must be frbch_dedisperse_nout()");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  int64_t maxd = 0;
  const std::vector<int32_t> delays = post_delays(fil, dms, ndm, &maxd);
  double* d_rowsum = nullptr;
  int32_t* d_delays = nullptr;
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  POST_DEV(ps.alloc(&d_rowsum, nrows * sizeof(double)), "hipMalloc");
  POST_DEV(ps.alloc(&d_delays, delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_delays, delays.data(), delays.size() * sizeof(int32_t), s), "upload delays");
  PostParams p = post_params<PostParams>(fil, d_rows, nrows);
  p.prod = (int)fil->product;
  p.rowsum = d_rowsum;
  p.delays = d_delays;
  p.out = d_out;
  p.nout = nout;
  p.ndm = (int)ndm;
  p.zerodm = zerodm ? 1 : 0;
  p.rows_per_chunk = kPostChunkRows;
  uint64_t nflag = 0;
  if ((rc = post_dedisp_prepass(ps, e, fil, nrows, zerodm, clip_sigma, p, &nflag)) != 0) return rc;
  std::vector<int32_t> range;
  const bool tiled = post_dedisp_tiled(fil, d_rows, delays, ndm, &range);
#ifndef FRBCH_NO_FAST
  if (tiled) {
    const int bpv = fil->nbits / 8, ngrp = (int)((ndm + fast::kDedND - 1) / fast::kDedND);
    int32_t* d_range = nullptr;
    POST_DEV(ps.alloc(&d_range, range.size() * sizeof(int32_t)), "hipMalloc");
    POST_DEV(dev_h2d(d_range, range.data(), range.size() * sizeof(int32_t), s), "upload tile ranges");
    POST_DEV(dev_sync(s), "sync");
    p.tile_range = d_range;
    const size_t lds = (size_t)fast::kDedRowsCap * fast::kDedRowB + 16 + (size_t)fast::kDedRowsCap * 9;
    const dim3 grid((unsigned)((nout + fast::kDedTT - 1) / fast::kDedTT), (unsigned)ngrp);
    const bool fl = p.flagged != nullptr, zd = p.zerodm != 0;
    int refused;
    if (bpv == 1) refused = launch_dedisp_tiled<1>(fl, zd, grid, lds, s, p);
    else if (bpv == 2) refused = launch_dedisp_tiled<2>(fl, zd, grid, lds, s, p);
    else refused = launch_dedisp_tiled<4>(fl, zd, grid, lds, s, p);
    POST_DEV(refused, "LDS size");
  }
#endif
  if (!tiled) DEV_LAUNCH(frbch_post_dedisp, (nout + 255) / 256, ndm, 256, 0, s, p);
  POST_DEV(dev_check_launch(), "launch dedisp");
  POST_DEV(dev_sync(s), "sync");
  if (nclipped) *nclipped = nflag;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dedisperse_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms,
                                     uint32_t ndm, uint32_t zerodm, double clip_sigma, int device, float* out,
                                     uint64_t nout, uint64_t* nclipped, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!rows || !out) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_out = hs.out(out, (size_t)ndm * nout * sizeof(float));
  return hs.run(e, "device memory for the rows", "upload rows", "download series",
                [&]() { return frbch_dedisperse_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, device, d_out, nout, nclipped, err, err_cap); });
}

extern "C" long frbch_fold_nsub(const frbch_fil_desc* fil, uint64_t nrows, double subint_s) {
  PostErr e{nullptr, 0};
  if (post_check_fil(fil, nrows, e) || !(subint_s > 0)) return FRBCH_E_ARG;
  const uint64_t rps = std::max<uint64_t>(1, (uint64_t)llround(subint_s / fil->tsamp_s));
  return (long)((nrows + rps - 1) / rps);       // the last sub-integration may be short (dspsr -L keeps it too)
}

extern "C" int frbch_fold_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, double f0_hz, double f1,
                                 double pepoch_mjd, double dm, uint32_t apply_delays, uint32_t nbin, double subint_s,
                                 int device, double* d_profile, uint32_t* d_hits, uint32_t nsub, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!d_rows || !d_profile || !d_hits) return e.fail(FRBCH_E_ARG, "null argument");
  if (!(f0_hz > 0) || nbin < 2 || nbin > 65536) return e.fail(FRBCH_E_ARG, "F0 must be positive, nbin in [2, 65536]");
  const long want = frbch_fold_nsub(fil, nrows, subint_s);
  if (want <= 0 || (uint32_t)want != nsub) return e.fail(FRBCH_E_CAPACITY, "nsub must be frbch_fold_nsub()");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps(false);                                     // (no stage of frbch_candidates_*: no clock)
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  const size_t nslot = (size_t)nsub * nbin * fil->nchan;
  unsigned long long* d_sum_i = nullptr;
  double* d_dly = nullptr;
  PostParams p = post_params<PostParams>(fil, d_rows, nrows);
  p.prod = (int)fil->product;
  p.hits = d_hits;
  POST_DEV(dev_memset(d_hits, 0, nslot * sizeof(uint32_t), s), "clear hits");
  POST_DEV(dev_memset(d_profile, 0, nslot * sizeof(double), s), "clear profile");
  const bool integer_rows = fil->nbits != 32;
  if (integer_rows) {      // exact uint64 sums, converted to double at the end
    POST_DEV(ps.alloc(&d_sum_i, nslot * sizeof(unsigned long long)), "hipMalloc");
    POST_DEV(dev_memset(d_sum_i, 0, nslot * sizeof(unsigned long long), s), "clear sums");
    p.prof_i = d_sum_i;
  } else {
    p.prof_f = d_profile;
  }
  if (apply_delays && dm != 0.0) {
    std::vector<double> dly(fil->nchan);
    for (uint32_t c = 0; c < fil->nchan; ++c) dly[c] = post_delay_s(fil, dm, c);
    POST_DEV(ps.alloc(&d_dly, dly.size() * sizeof(double)), "hipMalloc");
    POST_DEV(dev_h2d(d_dly, dly.data(), dly.size() * sizeof(double), s), "upload delays");
    POST_DEV(dev_sync(s), "sync");
    p.chan_delay_s = d_dly;
  }
  p.t0_s = (fil->tstart_mjd - pepoch_mjd) * 86400.0;
  p.tsamp_s = fil->tsamp_s;
  p.f0 = f0_hz;
  p.half_f1 = 0.5 * f1;
  p.nbin = (int)nbin;
  p.rows_per_sub = std::max<uint64_t>(1, (uint64_t)llround(subint_s / fil->tsamp_s));
  p.nsub = nsub;
  p.rows_per_chunk = 512;
  DEV_LAUNCH(frbch_post_fold, (fil->nchan + 255) / 256, (nrows + p.rows_per_chunk - 1) / p.rows_per_chunk, 256, 0, s, p);
  POST_DEV(dev_check_launch(), "launch fold");
  if (integer_rows) {
    // exact integer sums -> double (every value < 2^53)
    std::vector<unsigned long long> tmp(nslot);
    POST_DEV(dev_d2h(tmp.data(), d_sum_i, nslot * sizeof(unsigned long long), s), "download sums");
    POST_DEV(dev_sync(s), "sync");
    std::vector<double> dbl(nslot);
    for (size_t i = 0; i < nslot; ++i) dbl[i] = (double)tmp[i];
    POST_DEV(dev_h2d(d_profile, dbl.data(), nslot * sizeof(double), s), "upload profile");
  }
  POST_DEV(dev_sync(s), "sync");
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_fold_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, double f0_hz, double f1,
                               double pepoch_mjd, double dm, uint32_t apply_delays, uint32_t nbin, double subint_s,
                               int device, double* profile, uint32_t* hits, uint32_t nsub, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!rows || !profile || !hits) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t nslot = (size_t)nsub * nbin * fil->nchan;
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  double* d_prof = hs.out(profile, nslot * sizeof(double));
  uint32_t* d_hits = hs.out(hits, nslot * sizeof(uint32_t));
  return hs.run(e, "device memory for the rows", "upload rows", "download profile", [&]() {
    return frbch_fold_device(fil, d_rows, nrows, f0_hz, f1, pepoch_mjd, dm, apply_delays, nbin, subint_s, device, d_prof, d_hits, nsub, err, err_cap);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// fold of every product with a phase model (polynomial + Doppler factor, or TEMPO polyco blocks)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// the model as the kernels read it: blocks relative to the start of the file, first row of every block
int foldp_model(const frbch_fil_desc* fil, uint64_t nrows, const frbch_fold_model* m, std::vector<FoldSeg>* seg,
                std::vector<uint64_t>* seg_row, const PostErr& e) {
  if (!m || m->size != sizeof(frbch_fold_model)) return e.fail(FRBCH_E_ARG, "frbch_fold_model: wrong size");
  if (m->nbin < 2 || m->nbin > 65536) return e.fail(FRBCH_E_ARG, "nbin must be in [2, 65536]");
  if (!m->nseg) {
    if (!(m->f0_hz > 0)) return e.fail(FRBCH_E_ARG, "F0 must be positive");
    if (!(m->doppler > -1.0) || !(m->doppler < 1.0)) return e.fail(FRBCH_E_ARG, "doppler must lie in (-1, 1)");
    return FRBCH_OK;
  }
  if (!m->seg) return e.fail(FRBCH_E_ARG, "nseg > 0 without blocks");
  if (m->doppler != 0.0) return e.fail(FRBCH_E_ARG, "doppler together with a polyco: a polyco is topocentric already");
  const double last_s = (double)(nrows - 1) * fil->tsamp_s;
  bool first_in = false, last_in = false;
  for (uint32_t i = 0; i < m->nseg; ++i) {
    const frbch_polyco_seg& g = m->seg[i];
    if (g.ncoeff < 1 || g.ncoeff > 15) return e.fail(FRBCH_E_ARG, "polyco block " + std::to_string(i) + ": ncoeff must be 1..15");
    if (!(g.span_min > 0) || !(g.f0_hz > 0)) return e.fail(FRBCH_E_ARG, "polyco block " + std::to_string(i) + ": span and F0 must be positive");
    if (i && !(g.tmid_mjd > m->seg[i - 1].tmid_mjd)) return e.fail(FRBCH_E_ARG, "polyco blocks must be in ascending TMID order");
    FoldSeg f;
    memset(&f, 0, sizeof f);
    f.dt0_min = (fil->tstart_mjd - g.tmid_mjd) * 1440.0;
    f.rphase = g.rphase_frac;
    f.f0 = g.f0_hz;
    f.ncoeff = (int)g.ncoeff;
    for (uint32_t k = 0; k < g.ncoeff; ++k) f.coeff[k] = g.coeff[k];
    seg->push_back(f);
    uint64_t first = 0;
    if (i) {
      const double x = ((0.5 * (m->seg[i - 1].tmid_mjd + g.tmid_mjd) - fil->tstart_mjd) * 86400.0) / fil->tsamp_s;
      first = x <= 0.0 ? 0 : (x >= (double)nrows ? nrows : (uint64_t)ceil(x));
    }
    seg_row->push_back(first);
    if (fabs(f.dt0_min) <= 0.5 * g.span_min) first_in = true;
    if (fabs(f.dt0_min + last_s / 60.0) <= 0.5 * g.span_min) last_in = true;
  }
  if (!first_in || !last_in)
    return e.fail(FRBCH_E_ARG, std::string(first_in ? "the last" : "the first") + " row lies outside the span of every polyco block");
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_foldp_device(const frbch_fil_desc* fil_in, const void* d_rows, uint64_t nrows, const frbch_fold_model* m,
                                  int device, double* d_profile, uint32_t* d_hits, uint32_t nsub, uint32_t* kernel_used,
                                  char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!fil_in || fil_in->size != sizeof(frbch_fil_desc)) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size");
  frbch_fil_desc fd = *fil_in;
  fd.product = 0;                                          // every product is folded
  const frbch_fil_desc* fil = &fd;
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (fil->nifs > 4) return e.fail(FRBCH_E_ARG, "nifs must be 1..4");
  if (!d_rows || !d_profile || !d_hits) return e.fail(FRBCH_E_ARG, "null argument");
  std::vector<FoldSeg> seg;
  std::vector<uint64_t> seg_row;
  rc = foldp_model(fil, nrows, m, &seg, &seg_row, e);
  if (rc) return rc;
  const long want = frbch_fold_nsub(fil, nrows, m->subint_s);
  if (want <= 0 || (uint32_t)want != nsub) return e.fail(FRBCH_E_CAPACITY, "nsub must be frbch_fold_nsub()");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps(false);
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  const uint32_t nbin = m->nbin;
  const size_t nslot = (size_t)nsub * nbin * fil->nchan, nsum = nslot * fil->nifs;
  unsigned long long* d_sum_i = nullptr;
  double* d_dly = nullptr;
  FoldSeg* d_seg = nullptr;
  uint64_t* d_seg_row = nullptr;
  FoldpParams p = post_params<FoldpParams>(fil, d_rows, nrows);
  p.nbin = (int)nbin;
  p.hits = d_hits;
  const bool integer_rows = fil->nbits != 32;
  if (integer_rows) {      // exact uint64 sums, converted to double at the end
    POST_DEV(ps.alloc(&d_sum_i, nsum * sizeof(unsigned long long)), "hipMalloc");
    POST_DEV(dev_memset(d_sum_i, 0, nsum * sizeof(unsigned long long), s), "clear sums");
    p.prof_i = d_sum_i;
  } else {
    POST_DEV(dev_memset(d_profile, 0, nsum * sizeof(double), s), "clear profile");
  }
  p.prof_f = d_profile;
  std::vector<double> dly;
  if (m->apply_delays && m->dm != 0.0) {
    dly.resize(fil->nchan);
    for (uint32_t c = 0; c < fil->nchan; ++c) dly[c] = post_delay_s(fil, m->dm, c);
    POST_DEV(ps.alloc(&d_dly, dly.size() * sizeof(double)), "hipMalloc");
    POST_DEV(dev_h2d(d_dly, dly.data(), dly.size() * sizeof(double), s), "upload delays");
    p.chan_delay_s = d_dly;
  }
  if (!seg.empty()) {
    POST_DEV(ps.alloc(&d_seg, seg.size() * sizeof(FoldSeg)), "hipMalloc");
    POST_DEV(ps.alloc(&d_seg_row, seg_row.size() * sizeof(uint64_t)), "hipMalloc");
    POST_DEV(dev_h2d(d_seg, seg.data(), seg.size() * sizeof(FoldSeg), s), "upload polyco blocks");
    POST_DEV(dev_h2d(d_seg_row, seg_row.data(), seg_row.size() * sizeof(uint64_t), s), "upload block rows");
    p.seg = d_seg;
    p.seg_row = d_seg_row;
    p.nseg = (int)seg.size();
  }
  p.t0_s = (fil->tstart_mjd - m->pepoch_mjd) * 86400.0;
  p.tsamp_s = fil->tsamp_s;
  p.f0 = m->f0_hz;
  p.half_f1 = 0.5 * m->f1;
  p.doppler = m->doppler;
  p.rows_per_sub = std::max<uint64_t>(1, (uint64_t)llround(m->subint_s / fil->tsamp_s));
  p.nsub = nsub;
  uint32_t used = 0;
#ifndef FRBCH_NO_FAST
  {   // the LDS kernel: integer rows, the bin a function of the row only, a tile of >= 16 channels x nbin in the LDS
    const int bpv = fil->nbits / 8;
    int ct = 0, ct_log2 = 0;
    for (int k = 8; k >= 4; --k)
      if (fil->nchan % (1u << k) == 0 && (size_t)nbin * (1u << k) * sizeof(uint32_t) <= fast::kFoldLdsBudget) { ct = 1 << k; ct_log2 = k; break; }
    const uint64_t row_cap = bpv == 1 ? (1ull << 24) : (1ull << 16);      // a uint32 sum of a run cannot overflow
    if (integer_rows && !p.chan_delay_s && ct && ((uintptr_t)d_rows % 4) == 0 && (uint64_t)nsub * nbin < 0xFFFFFFFFull &&
        (uint64_t)(fil->nchan / ct) * fil->nifs <= 65535) {
      p.ct = ct;
      p.ct_log2 = ct_log2;
      p.ntile = (int)fil->nchan / ct;
      const uint64_t nbase = (uint64_t)p.ntile * fil->nifs * nsub;          // workgroups with one row run per sub-integration
      const uint64_t wg_goal = (uint64_t)fast::kFoldWgPerCu * std::max(1, dev_cu_count(device));
      const uint64_t per_sub = std::max<uint64_t>(1, (wg_goal + nbase - 1) / nbase);
      p.rows_per_chunk = std::min(row_cap, std::max<uint64_t>(fast::kFoldThreads, (p.rows_per_sub + per_sub - 1) / per_sub));
      p.chunks_per_sub = (uint32_t)((p.rows_per_sub + p.rows_per_chunk - 1) / p.rows_per_chunk);
      if ((uint64_t)nsub * p.chunks_per_sub <= 0x7FFFFFFFull) {
        uint32_t *d_slot = nullptr, *d_slot_hits = nullptr;
        POST_DEV(ps.alloc(&d_slot, nrows * sizeof(uint32_t)), "hipMalloc");
        POST_DEV(ps.alloc(&d_slot_hits, (size_t)nsub * nbin * sizeof(uint32_t)), "hipMalloc");
        POST_DEV(dev_memset(d_slot_hits, 0, (size_t)nsub * nbin * sizeof(uint32_t), s), "clear slot counts");
        p.slot = d_slot;
        p.slot_hits = d_slot_hits;
        p.nconv = nslot;
        hipLaunchKernelGGL(fast::frbch_post_foldp_slots, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, p);
        POST_DEV(dev_check_launch(), "launch fold slots");
        hipLaunchKernelGGL(fast::frbch_post_foldp_hits, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, s, p);
        POST_DEV(dev_check_launch(), "launch fold hits");
        const size_t lds = (size_t)nbin * ct * sizeof(uint32_t);
        const dim3 grid((unsigned)((uint64_t)nsub * p.chunks_per_sub), (unsigned)(p.ntile * fil->nifs));
        if (bpv == 1) POST_DEV(launch_lds(fast::frbch_post_foldp_lds<1>, grid, dim3(fast::kFoldThreads), lds, s, p), "LDS size");
        else POST_DEV(launch_lds(fast::frbch_post_foldp_lds<2>, grid, dim3(fast::kFoldThreads), lds, s, p), "LDS size");
        POST_DEV(dev_check_launch(), "launch fold");
        used = 1;
      }
    }
  }
#endif
  if (!used) {
    POST_DEV(dev_memset(d_hits, 0, nslot * sizeof(uint32_t), s), "clear hits");
    p.rows_per_chunk = 512;
    DEV_LAUNCH(frbch_post_foldp, (fil->nchan + 255) / 256, (nrows + p.rows_per_chunk - 1) / p.rows_per_chunk, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch fold");
  }
  if (integer_rows) {
    p.prof_f = d_profile;
    p.nconv = nsum;
    DEV_LAUNCH(frbch_post_u64_to_f64, (nsum + 255) / 256, 1, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch convert");
  }
  POST_DEV(dev_sync(s), "sync");       // (also: the host vectors the uploads read stay alive until here)
  if (kernel_used) *kernel_used = used;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_foldp_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_fold_model* m, int device,
                                double* profile, uint32_t* hits, uint32_t nsub, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  if (!fil || fil->size != sizeof(frbch_fil_desc)) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size");
  frbch_fil_desc fd = *fil;
  fd.product = 0;
  int rc = post_check_fil(&fd, nrows, e);
  if (rc) return rc;
  if (!rows || !profile || !hits) return e.fail(FRBCH_E_ARG, "null argument");
  if (!m || m->size != sizeof(frbch_fold_model)) return e.fail(FRBCH_E_ARG, "frbch_fold_model: wrong size");
  if (m->nbin < 2 || m->nbin > 65536) return e.fail(FRBCH_E_ARG, "nbin must be in [2, 65536]");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t nslot = (size_t)nsub * m->nbin * fil->nchan, nsum = nslot * fil->nifs;
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  double* d_prof = hs.out(profile, nsum * sizeof(double));
  uint32_t* d_hits = hs.out(hits, nslot * sizeof(uint32_t));
  return hs.run(e, "device memory for the rows", "upload rows", "download profile",
                [&]() { return frbch_foldp_device(fil, d_rows, nrows, m, device, d_prof, d_hits, nsub, kernel_used, err, err_cap); });
}

// ---------------------------------------------------------------------------------------------------------------------
// single-pulse search of the dedispersed series
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kSpRawCap = 1u << 20;     // raw peaks the device list holds (24 MiB); more: FRBCH_E_CAPACITY, never a cut list

int sp_check(const frbch_sp_params* sp, uint64_t* blk_len, const PostErr& e) {
  if (!sp || sp->size != sizeof(frbch_sp_params)) return e.fail(FRBCH_E_ARG, "frbch_sp_params: wrong size");
  if (!(sp->threshold > 0.0) || !(sp->threshold <= 1.0e6)) return e.fail(FRBCH_E_ARG, "threshold must lie in (0, 1e6]");
  if (sp->nwidth < 1 || sp->nwidth > 16) return e.fail(FRBCH_E_ARG, "1..16 widths");
  for (uint32_t k = 0; k < sp->nwidth; ++k)
    if (sp->widths[k] < 1 || sp->widths[k] > 1024 || (k && sp->widths[k] <= sp->widths[k - 1]))
      return e.fail(FRBCH_E_ARG, "widths must be strictly ascending, each 1..1024");
  *blk_len = sp->detrend_len ? sp->detrend_len : 1000;
  if (*blk_len < 64 || *blk_len > 65536) return e.fail(FRBCH_E_ARG, "detrend_len must be 0 (= 1000) or 64..65536");
  return FRBCH_OK;
}

// Which search kernel a call takes -- the one decision behind frbch_spsearch_device's launch and *kernel_used.  true = the
// LDS kernel (kernels_post_fast.inc): the tile and the halo of the largest LISTED width (one that exceeds nout included)
// fit its prefix array, kSpTile + 2 wmax <= kSpLdsN, and sample indices fit 32 bits.  The emulator build has no such
// kernel: false.
bool sp_search_lds(const frbch_sp_params* sp, uint64_t nout) {
#ifndef FRBCH_NO_FAST
  return (int)sp->widths[sp->nwidth - 1] <= fast::kSpMaxWidth && nout < (1ull << 31);
#else
  (void)sp; (void)nout;
  return false;
#endif
}

struct SpRaw {
  uint32_t width;
  uint64_t centre;
  long long sum;
  double sigma;
};
// frbch_spsearch_device; with `all` every candidate goes there instead (cands and cap are then not looked at, and no
// number of candidates is a capacity error): frbch_candidates_* own their list
int sp_search_run(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_sp_params* sp, int device, frbch_sp_cand* cands,
                  uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, std::vector<frbch_sp_cand>* all, char* err, size_t err_cap);
}  // namespace

extern "C" int frbch_spsearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_sp_params* sp, int device,
                                     frbch_sp_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err,
                                     size_t err_cap) try {
  return sp_search_run(d_series, ndm, nout, sp, device, cands, cap, ncand, kernel_used, nullptr, err, err_cap);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

namespace {
int sp_search_run(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_sp_params* sp, int device, frbch_sp_cand* cands,
                  uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, std::vector<frbch_sp_cand>* all, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint64_t blk_len = 0;
  int rc = sp_check(sp, &blk_len, e);
  if (rc) return rc;
  if (!d_series || !ncand || (!all && cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if (!ndm || !nout || ndm > 65535) return e.fail(FRBCH_E_ARG, "ndm must be 1..65535, nout positive");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  SpParams p;
  memset(&p, 0, sizeof p);
  p.series = d_series;
  p.nout = nout;
  p.ndm = (int)ndm;
  p.blk_len = blk_len;
  p.nblk = (uint32_t)std::max<uint64_t>(1, nout / blk_len);
  p.nwidth = (int)sp->nwidth;
  for (uint32_t k = 0; k < sp->nwidth; ++k) {
    p.width[k] = (int)sp->widths[k];
    const double scaled = sp->threshold * 1024.0;
    const double t = ceil(scaled * sqrt((double)sp->widths[k]));
    p.thr[k] = t < 9.0e18 ? (long long)t : INT64_MAX;             // (no sum reaches 2^37)
  }
  p.peak_cap = kSpRawCap;
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  POST_DEV(ps.alloc(&p.stats, (size_t)ndm * p.nblk * 2 * sizeof(double)), "hipMalloc");
  POST_DEV(ps.alloc(&p.peaks, (size_t)kSpRawCap * sizeof(SpPeak)), "hipMalloc");
  POST_DEV(ps.alloc(&p.npeak, sizeof(uint32_t)), "hipMalloc");
  POST_DEV(dev_memset(p.npeak, 0, sizeof(uint32_t), s), "clear peak count");
  DEV_LAUNCH(frbch_post_sp_stats, p.nblk, ndm, kSpPartials, (3 * kSpPartials + 2) * sizeof(double), s, p);
  POST_DEV(dev_check_launch(), "launch block statistics");
  const bool lds = sp_search_lds(sp, nout);
#ifndef FRBCH_NO_FAST
  if (lds)
    hipLaunchKernelGGL(fast::frbch_post_sp_search_lds, dim3((unsigned)((nout + fast::kSpTile - 1) / fast::kSpTile), ndm),
                       dim3(fast::kSpThreads), 0, s, p);
#endif
  if (!lds) {
    POST_DEV(ps.alloc(&p.q, (size_t)ndm * nout * sizeof(int32_t)), "hipMalloc");
    DEV_LAUNCH(frbch_post_sp_quant, (nout + 255) / 256, ndm, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch quantise");
    DEV_LAUNCH(frbch_post_sp_search, (nout + 255) / 256, ndm, 256, 0, s, p);
  }
  POST_DEV(dev_check_launch(), "launch search");
  uint32_t nraw = 0;
  POST_DEV(dev_d2h(&nraw, p.npeak, sizeof nraw, s), "download peak count");
  POST_DEV(dev_sync(s), "sync");
  if (nraw > kSpRawCap)
    return e.fail(FRBCH_E_CAPACITY, "threshold too low: " + std::to_string(nraw) + " raw peaks, the device list holds " +
                                        std::to_string(kSpRawCap));
  std::vector<SpPeak> raw(nraw);
  if (nraw) {
    POST_DEV(dev_d2h(raw.data(), p.peaks, (size_t)nraw * sizeof(SpPeak), s), "download peaks");
    POST_DEV(dev_sync(s), "sync");
  }
  ps.release();                           // the device is done with; the host goes on with the raw list
  if (kernel_used) *kernel_used = lds ? 1 : 0;
  // across widths, DM by DM, on the raw list (one pass, not iterated): a raw peak falls to a stronger one whose centre
  // lies within half the larger of the two widths; equal sigma: the narrower wins, then the earlier
  std::sort(raw.begin(), raw.end(), [](const SpPeak& a, const SpPeak& b) {
    return a.dm != b.dm ? a.dm < b.dm : a.t + a.width / 2 != b.t + b.width / 2 ? a.t + a.width / 2 < b.t + b.width / 2 : a.width < b.width;
  });
  uint64_t total = 0;
  std::vector<SpRaw> one;
  const uint64_t reach = sp->widths[sp->nwidth - 1] / 2;
  for (size_t i0 = 0; i0 < raw.size();) {
    size_t i1 = i0;
    one.clear();
    for (; i1 < raw.size() && raw[i1].dm == raw[i0].dm; ++i1) {
      SpRaw r;
      r.width = raw[i1].width;
      r.centre = raw[i1].t + raw[i1].width / 2;
      r.sum = raw[i1].sum;
      r.sigma = (double)raw[i1].sum / (1024.0 * sqrt((double)raw[i1].width));
      one.push_back(r);
    }
    size_t first = 0;                                             // one[first ..) may still lie within `reach` of one[i]
    for (size_t i = 0; i < one.size(); ++i) {
      const SpRaw& a = one[i];
      while (one[first].centre + reach < a.centre) ++first;
      bool dropped = false;
      for (size_t j = first; j < one.size() && one[j].centre <= a.centre + reach && !dropped; ++j) {
        if (j == i) continue;
        const SpRaw& b = one[j];
        const uint64_t dist = a.centre > b.centre ? a.centre - b.centre : b.centre - a.centre;
        if (dist > std::max(a.width, b.width) / 2) continue;
        dropped = b.sigma > a.sigma || (b.sigma == a.sigma && (b.width < a.width || (b.width == a.width && b.centre < a.centre)));
      }
      if (dropped) continue;
      if (all || total < cap) {                                   // (centre, width) ascending already: the output order
        frbch_sp_cand c;
        c.dm_index = raw[i0].dm;
        c.width = a.width;
        c.sample = a.centre;
        c.sigma = (float)a.sigma;
        c.reserved = 0;
        if (all) all->push_back(c);
        else cands[total] = c;
      }
      ++total;
    }
    i0 = i1;
  }
  *ncand = total;
  if (!all && total > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(total) + " candidates, room for " + std::to_string(cap));
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_spsearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_sp_params* sp, int device,
                                   frbch_sp_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err,
                                   size_t err_cap) {
  PostErr e{err, err_cap};
  uint64_t blk_len = 0;
  int rc = sp_check(sp, &blk_len, e);
  if (rc) return rc;
  if (!series || !ndm || !nout) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  float* d_series = hs.in(series, (size_t)ndm * nout * sizeof(float));
  return hs.run(e, "device memory for the series", "upload series", "download",
                [&]() { return frbch_spsearch_device(d_series, ndm, nout, sp, device, cands, cap, ncand, kernel_used, err, err_cap); });
}

extern "C" int frbch_dedisperse_search_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms,
                                            uint32_t ndm, uint32_t zerodm, double clip_sigma, const frbch_sp_params* sp,
                                            int device, float* series_out, uint64_t nout, uint64_t* nclipped,
                                            frbch_sp_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used,
                                            char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  uint64_t blk_len = 0;
  rc = sp_check(sp, &blk_len, e);
  if (rc) return rc;
  if (!rows || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_out = hs.out(series_out, (size_t)ndm * nout * sizeof(float));          // (series_out may be null: no download then)
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the rows");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload rows");
  rc = frbch_dedisperse_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, device, d_out, nout, nclipped, err, err_cap);
  hs.drop(d_rows);                                                 // the plane stays in HBM; the rows are done with
  if (!rc && series_out && hs.download() != 0) rc = e.fail(FRBCH_E_DEVICE, "download series");
  if (!rc) rc = frbch_spsearch_device(d_out, ndm, nout, sp, device, cands, cap, ncand, kernel_used, err, err_cap);
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// periodicity search of the dedispersed series
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kPsRawCap = 1u << 20;     // raw peaks the device list holds (16 MiB); more: FRBCH_E_CAPACITY, never a cut list
constexpr int kPsMinLog = 12, kPsMaxLog = 22;
constexpr double kPsSigmaMax = 30.0;

struct PsPlan {
  uint32_t n = 0, wblock = 0, nblk = 0, kmin = 0, nfold = 0;
  int log2n = 0;
  double tsamp = 0.0;
};

bool ps_fold_ok(uint32_t h) { return h == 1 || h == 2 || h == 4 || h == 8 || h == 16; }

int ps_check(const frbch_ps_params* par, uint64_t nout, double tsamp_default, PsPlan* pl, const PostErr& e) {
  if (!par || par->size != sizeof(frbch_ps_params)) return e.fail(FRBCH_E_ARG, "frbch_ps_params: wrong size");
  if (!(par->sigma > 0.0) || !(par->sigma <= kPsSigmaMax)) return e.fail(FRBCH_E_ARG, "sigma must lie in (0, 30]");
  if (par->nharm != 0 && !ps_fold_ok(par->nharm)) return e.fail(FRBCH_E_ARG, "nharm must be 1, 2, 4, 8 or 16 (0 = 16)");
  const uint32_t B = par->wblock ? par->wblock : 128;
  if (B < 32 || B > 1024 || (B & (B - 1))) return e.fail(FRBCH_E_ARG, "wblock must be a power of two in 32..1024 (0 = 128)");
  if (!(par->flo_hz >= 0.0) || !(par->flo_hz < 1.0e300)) return e.fail(FRBCH_E_ARG, "flo_hz must be finite and not negative");
  const double tsamp = par->tsamp_s != 0.0 ? par->tsamp_s : tsamp_default;
  if (!(tsamp > 0.0) || !(tsamp < 1.0e300)) return e.fail(FRBCH_E_ARG, "tsamp_s must be positive");
  uint64_t n = par->nfft;
  if (!n) {
    n = 1;
    while (n * 2 <= nout && n < (1ull << kPsMaxLog)) n *= 2;
  }
  if ((n & (n - 1)) || n < (1ull << kPsMinLog) || n > (1ull << kPsMaxLog) || n > nout)
    return e.fail(FRBCH_E_ARG, "the transform length must be a power of two in 2^12..2^22 and at most nout");
  pl->n = (uint32_t)n;
  pl->log2n = 0;
  while ((1ull << pl->log2n) < n) ++pl->log2n;
  pl->wblock = B;
  const uint32_t nb = pl->n / 2 - 1, rest = nb % B;
  pl->nblk = nb / B + (rest != 0 && rest >= B / 2 ? 1u : 0u);
  const double flo = par->flo_hz != 0.0 ? par->flo_hz : 0.5;
  const double kf = ceil(flo * (double)pl->n * tsamp);
  pl->kmin = kf < 1.0 ? 1u : kf < (double)(pl->n / 2) ? (uint32_t)kf : pl->n / 2;      // n / 2: nothing is searched
  const uint32_t nharm = par->nharm ? par->nharm : 16;
  pl->nfold = 0;
  while ((1u << pl->nfold) <= nharm) ++pl->nfold;
  pl->tsamp = tsamp;
  return FRBCH_OK;
}

// how the fast form cuts the log2 n stages into LDS-resident passes: one up to 2^13, two up to 2^18 (9 stages a pass with 16
// columns in a tile of 2^13 values), three above
int ps_passes(int L, int r[3]) {
  r[0] = r[1] = r[2] = 0;
  if (L <= 13) { r[0] = L; return 1; }
  if (L <= 18) { r[0] = (L + 1) / 2; r[1] = L - r[0]; return 2; }
  r[0] = (L + 2) / 3;
  r[1] = (L - r[0] + 1) / 2;
  r[2] = L - r[0] - r[1];
  return 3;
}

// the one decision behind frbch_psearch_device's launches and frbch_psearch_kernel's answer; the emulator build has no fast form
bool ps_fast(const float* d_series) {
#ifndef FRBCH_NO_FAST
  return ((uintptr_t)d_series % 16) == 0;
#else
  (void)d_series;
  return false;
#endif
}

// W[k] = ((float)cos(a), (float)(-sin(a))), a = 2.0 pi k / n, k < n / 2.  A million sines take the host longer than the device
// takes for the transforms, so the table of the last length asked for is kept (at most 16 MiB).
std::shared_ptr<const std::vector<float>> ps_table(uint32_t n) {
  static std::mutex m;
  static std::shared_ptr<const std::vector<float>> kept;
  std::lock_guard<std::mutex> lk(m);
  if (kept && kept->size() == (size_t)n) return kept;
  auto tw = std::make_shared<std::vector<float>>((size_t)n);
  for (uint32_t k = 0; k < n / 2; ++k) {
    const double a = 2.0 * M_PI * (double)k / (double)n;
    (*tw)[2 * (size_t)k] = (float)cos(a);
    (*tw)[2 * (size_t)k + 1] = (float)(-sin(a));
  }
  kept = tw;
  return kept;
}

// Q(h, x) = exp(-x) sum_{i<h} x^i / i!
double ps_q(uint32_t h, double x) {
  double term = 1.0, sum = 1.0;
  for (uint32_t i = 1; i < h; ++i) { term = term * x / (double)i; sum = sum + term; }
  return exp(-x) * sum;
}

// log Q(h, x) without overflow: below 1 the sum as it stands, from 1 on with its largest term x^(h-1) / (h-1)! taken out
double ps_logq(uint32_t h, double x) {
  if (x < 1.0) {
    double s = 1.0;
    for (uint32_t i = h - 1; i >= 1; --i) s = s * x / (double)i + 1.0;
    return -x + log(s);
  }
  double r = 1.0, lf = 0.0;
  for (uint32_t i = 1; i < h; ++i) r = r * (double)i / x + 1.0;          // 1 + (h-1)/x (1 + (h-2)/x (... (1 + 1/x)))
  for (uint32_t i = 2; i < h; ++i) lf = lf + log((double)i);
  return -x + ((double)(h - 1) * log(x) - lf + log(r));
}

double ps_logtail(double s) {
  if (s < 30.0) return log(0.5 * erfc(s / sqrt(2.0)));
  const double s2 = s * s;
  return -0.5 * s2 - log(s) - 0.5 * log(2.0 * M_PI) + log1p(-1.0 / s2 + 3.0 / (s2 * s2));
}

double ps_sigma(uint32_t h, float H) {
  double x = (double)H;
  if (!(x <= (double)std::numeric_limits<float>::max())) x = (double)std::numeric_limits<float>::max();
  const double lq = ps_logq(h, x);
  if (!(lq < 0.0)) return 0.0;
  double lo = 0.0, hi = sqrt(-2.0 * lq) + 2.0;
  for (int it = 0; it < 64; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (ps_logtail(mid) > lq) lo = mid; else hi = mid;
  }
  return 0.5 * (lo + hi);
}

// a's fundamental lies below b's: k_a / h_a < k_b / h_b
bool ps_f_less(const frbch_ps_cand& a, const frbch_ps_cand& b) { return (uint64_t)a.k * b.h < (uint64_t)b.k * a.h; }
// |k_a h_b - k_b h_a|
uint64_t ps_f_dist(const frbch_ps_cand& a, const frbch_ps_cand& b) {
  const uint64_t x = (uint64_t)a.k * b.h, y = (uint64_t)b.k * a.h;
  return x > y ? x - y : y - x;
}

// step 8 on the raw records of all series (any order); fills sigma and freq_hz; the survivors in output order
void ps_sift(std::vector<frbch_ps_cand>& raw, uint32_t n, double tsamp, std::vector<frbch_ps_cand>* out) {
  for (frbch_ps_cand& c : raw) {
    c.sigma = ps_sigma(c.h, c.power);
    c.freq_hz = (double)c.k / ((double)c.h * ((double)n * tsamp));
  }
  std::sort(raw.begin(), raw.end(), [](const frbch_ps_cand& a, const frbch_ps_cand& b) {
    if (a.dm_index != b.dm_index) return a.dm_index < b.dm_index;
    if (ps_f_less(a, b)) return true;
    if (ps_f_less(b, a)) return false;
    return a.h != b.h ? a.h < b.h : a.k < b.k;
  });
  for (size_t i0 = 0; i0 < raw.size();) {
    size_t i1 = i0;
    while (i1 < raw.size() && raw[i1].dm_index == raw[i0].dm_index) ++i1;
    size_t first = i0;                                            // raw[first ..) may still lie within one bin below raw[i]
    for (size_t i = i0; i < i1; ++i) {
      const frbch_ps_cand& a = raw[i];
      while (ps_f_dist(raw[first], a) > (uint64_t)raw[first].h * a.h) ++first;       // (stops at i at the latest: distance 0)
      bool dropped = false;
      for (size_t j = first; j < i1 && !dropped; ++j) {
        if (j == i) continue;
        const frbch_ps_cand& b = raw[j];
        if (ps_f_dist(a, b) > (uint64_t)a.h * b.h) {
          if (j > i) break;                                       // sorted by f: every later one lies further
          continue;
        }
        dropped = b.sigma > a.sigma || (b.sigma == a.sigma && (b.h < a.h || (b.h == a.h && b.k < a.k)));
      }
      if (!dropped) out->push_back(a);
    }
    i0 = i1;
  }
  std::sort(out->begin(), out->end(), [](const frbch_ps_cand& a, const frbch_ps_cand& b) {
    return a.dm_index != b.dm_index ? a.dm_index < b.dm_index : a.h != b.h ? a.h < b.h : a.k < b.k;
  });
}

int ps_deliver(const std::vector<frbch_ps_cand>& out, frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, const PostErr& e) {
  *ncand = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) cands[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " candidates, room for " + std::to_string(cap));
  return FRBCH_OK;
}
}  // namespace

extern "C" long frbch_psearch_nfft(uint64_t nout, const frbch_ps_params* par) {
  PsPlan pl;
  if (ps_check(par, nout, 1.0, &pl, PostErr{nullptr, 0})) return FRBCH_E_ARG;
  return (long)pl.n;
}

extern "C" int frbch_psearch_thresholds(double sigma, float* thr) {
  if (!thr || !(sigma > 0.0) || !(sigma <= kPsSigmaMax)) return FRBCH_E_ARG;
  const double tail = 0.5 * erfc(sigma / sqrt(2.0));
  for (int f = 0; f < 5; ++f) {
    const uint32_t h = 1u << f;
    double lo = 0.0, hi = 1000.0;                                  // Q(lo) > tail >= Q(hi) throughout
    for (;;) {
      const double mid = 0.5 * (lo + hi);
      if (!(mid > lo) || !(mid < hi)) break;                       // one step of double wide
      if (ps_q(h, mid) > tail) lo = mid; else hi = mid;
    }
    float t = (float)hi;
    if ((double)t < hi) t = nextafterf(t, std::numeric_limits<float>::infinity());
    thr[f] = t;
  }
  return FRBCH_OK;
}

extern "C" int frbch_psearch_kernel(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, uint32_t* npass) {
  PsPlan pl;
  if (!d_series || !ndm || ndm > 65535 || ps_check(par, nout, 1.0, &pl, PostErr{nullptr, 0})) return FRBCH_E_ARG;
  int r[3];
  const bool fast = ps_fast(d_series);
  if (npass) *npass = fast ? (uint32_t)ps_passes(pl.log2n, r) : 0u;
  return fast ? 1 : 0;
}

extern "C" int frbch_psearch_sift(const frbch_ps_cand* raw, uint64_t nraw, uint32_t n, double tsamp_s, frbch_ps_cand* cands,
                                  uint64_t cap, uint64_t* ncand, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!ncand || (nraw && !raw) || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if ((n & (n - 1)) || n < (1u << kPsMinLog) || n > (1u << kPsMaxLog)) return e.fail(FRBCH_E_ARG, "n must be a power of two in 2^12..2^22");
  if (!(tsamp_s > 0.0) || !(tsamp_s < 1.0e300)) return e.fail(FRBCH_E_ARG, "tsamp_s must be positive");
  for (uint64_t i = 0; i < nraw; ++i)
    if (!ps_fold_ok(raw[i].h) || raw[i].k < 1 || raw[i].k >= n / 2)
      return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": h must be 1, 2, 4, 8 or 16 and k lie in 1 .. n/2 - 1");
  std::vector<frbch_ps_cand> all(raw, raw + nraw), out;
  ps_sift(all, n, tsamp_s, &out);
  return ps_deliver(out, cands, cap, ncand, e);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

namespace {
// steps 1 to 7 for the p.ndm series p describes, on stream s: the table, the scratch and a cleared p.npeak are in place
int ps_launches(const PsParams& p, const PsPlan& pl, bool fast, int npass, const int r[3], dev_stream_t s, const PostErr& e) {
  const uint32_t ndm = (uint32_t)p.ndm, n = p.n, nh = n / 2;
  DEV_LAUNCH(frbch_post_ps_mean, ndm, 1, kPsPartials, kPsPartials * sizeof(double), s, p);
  POST_DEV(dev_check_launch(), "launch mean");
#ifndef FRBCH_NO_FAST
  if (fast) {
    PsParams q = p;
    q.rcur = r[0];
    q.logc = npass == 1 ? 0 : 4;
    q.s0 = 0;
    if (launch_lds(fast::frbch_post_ps_fft_first, dim3(1u << (pl.log2n - q.rcur - q.logc), (unsigned)p.npair), dim3(fast::kPsThreads),
                   fast::ps_lds_bytes(q.rcur + q.logc), s, q) != 0)
      return e.fail(FRBCH_E_DEVICE, "LDS permission for the first pass");
    POST_DEV(dev_check_launch(), "launch first pass");
    for (int i = 1; i < npass; ++i) {
      q.s0 += q.rcur;
      q.rcur = r[i];
      q.logc = 4;
      if (launch_lds(fast::frbch_post_ps_fft_later, dim3(1u << (pl.log2n - q.rcur - 4), (unsigned)p.npair), dim3(fast::kPsThreads),
                     fast::ps_lds_bytes(q.rcur + 4), s, q) != 0)
        return e.fail(FRBCH_E_DEVICE, "LDS permission for a later pass");
      POST_DEV(dev_check_launch(), "launch later pass");
    }
  }
#endif
  if (!fast) {
    DEV_LAUNCH(frbch_post_ps_load, n / 256, p.npair, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch load");
    for (int st = 1; st <= pl.log2n; ++st) {
      PsParams q = p;
      q.stage = st;
      DEV_LAUNCH(frbch_post_ps_stage, nh / 256, p.npair, 256, 0, s, q);
    }
    POST_DEV(dev_check_launch(), "launch stages");
  }
  DEV_LAUNCH(frbch_post_ps_power, nh / 256, p.npair, 256, 0, s, p);
#ifndef FRBCH_NO_FAST
  if (fast) {
    const uint32_t per = (uint32_t)fast::kPsNormTile / pl.wblock;
    hipLaunchKernelGGL(fast::frbch_post_ps_norm_lds, dim3((pl.nblk + per - 1) / per, ndm), dim3(fast::kPsThreads), 0, s, p);
  }
#endif
  if (!fast) DEV_LAUNCH(frbch_post_ps_norm, (pl.nblk + 63) / 64, ndm, 64, 0, s, p);
  POST_DEV(dev_check_launch(), "launch powers and levels");
  if (pl.kmin < nh) {
    DEV_LAUNCH(frbch_post_ps_harm, nh / 256, ndm, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch harmonic sums");
  }
  return FRBCH_OK;
}

int ps_search_run(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, double tsamp_default, int device,
                  frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  PsPlan pl;
  int rc = ps_check(par, nout, tsamp_default, &pl, e);
  if (rc) return rc;
  if (!d_series || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if (!ndm || ndm > 65535) return e.fail(FRBCH_E_ARG, "ndm must be 1..65535");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const uint32_t n = pl.n, nh = n / 2;
  PsParams p;
  memset(&p, 0, sizeof p);
  p.series = d_series;
  p.nout = nout;
  p.ndm = (int)ndm;
  p.npair = (int)((ndm + 1) / 2);
  p.log2n = pl.log2n;
  p.n = n;
  p.wblock = pl.wblock; p.nblk = pl.nblk; p.kmin = pl.kmin; p.nfold = pl.nfold;
  while ((1u << p.logb) < pl.wblock) ++p.logb;
  frbch_psearch_thresholds(par->sigma, p.thr);
  p.peak_cap = kPsRawCap;
  const std::shared_ptr<const std::vector<float>> tw = ps_table(n);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  float* d_tw = nullptr;
  const size_t work_bytes = (size_t)p.npair * n * 2 * sizeof(float), pw_bytes = (size_t)ndm * nh * sizeof(float);
  if (ps.alloc(&d_tw, (size_t)n * sizeof(float)) || ps.alloc(&p.mean, (size_t)ndm * sizeof(double)) ||
      ps.alloc(&p.live, (size_t)ndm * sizeof(uint32_t)) || ps.alloc(&p.work, work_bytes) || ps.alloc(&p.pw, pw_bytes) ||
      ps.alloc(&p.peaks, (size_t)kPsRawCap * sizeof(PsPeak)) || ps.alloc(&p.npeak, sizeof(uint32_t)))
    return e.fail(FRBCH_E_NOMEM, "device memory for the periodicity search: work array " + std::to_string(work_bytes) + " bytes, powers " +
                                     std::to_string(pw_bytes) + " bytes, table " + std::to_string((size_t)n * sizeof(float)) +
                                     " bytes, raw peaks " + std::to_string((size_t)kPsRawCap * sizeof(PsPeak)) + " bytes");
  p.tw = d_tw;
  POST_DEV(dev_h2d(d_tw, tw->data(), (size_t)n * sizeof(float), s), "upload table");
  POST_DEV(dev_memset(p.npeak, 0, sizeof(uint32_t), s), "clear peak count");
  int r[3];
  const bool fast = ps_fast(d_series);
  const int npass = fast ? ps_passes(pl.log2n, r) : 0;
  if ((rc = ps_launches(p, pl, fast, npass, r, s, e)) != 0) return rc;
  uint32_t nraw = 0;
  POST_DEV(dev_d2h(&nraw, p.npeak, sizeof nraw, s), "download peak count");
  POST_DEV(dev_sync(s), "sync");
  if (nraw > kPsRawCap)
    return e.fail(FRBCH_E_CAPACITY, "threshold too low: " + std::to_string(nraw) + " raw peaks, the device list holds " +
                                        std::to_string(kPsRawCap));
  std::vector<PsPeak> raw(nraw);
  if (nraw) {
    POST_DEV(dev_d2h(raw.data(), p.peaks, (size_t)nraw * sizeof(PsPeak), s), "download peaks");
    POST_DEV(dev_sync(s), "sync");
  }
  ps.release();                           // the device is done with; the host goes on with the raw list
  if (kernel_used) { kernel_used[0] = fast ? 1u : 0u; kernel_used[1] = (uint32_t)npass; }
  std::vector<frbch_ps_cand> all(nraw), out;
  for (uint32_t i = 0; i < nraw; ++i) {
    frbch_ps_cand c;
    memset(&c, 0, sizeof c);
    c.dm_index = raw[i].dm; c.h = raw[i].h; c.k = raw[i].k; c.power = raw[i].H;
    all[i] = c;
  }
  ps_sift(all, n, pl.tsamp, &out);
  return ps_deliver(out, cands, cap, ncand, e);
}
}  // namespace

extern "C" int frbch_psearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, int device,
                                    frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err,
                                    size_t err_cap) try {
  return ps_search_run(d_series, ndm, nout, par, 0.0, device, cands, cap, ncand, kernel_used, err, err_cap);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_psearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, int device,
                                  frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err,
                                  size_t err_cap) {
  PostErr e{err, err_cap};
  PsPlan pl;
  int rc = ps_check(par, nout, 0.0, &pl, e);
  if (rc) return rc;
  if (!series || !ndm || ndm > 65535) return e.fail(FRBCH_E_ARG, "null argument, or ndm outside 1..65535");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  float* d_series = hs.in(series, (size_t)ndm * nout * sizeof(float));
  return hs.run(e, "device memory for the series", "upload series", "download",
                [&]() { return frbch_psearch_device(d_series, ndm, nout, par, device, cands, cap, ncand, kernel_used, err, err_cap); });
}

extern "C" int frbch_dedisperse_psearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms,
                                             uint32_t ndm, uint32_t zerodm, double clip_sigma, const frbch_ps_params* par,
                                             int device, float* series_out, uint64_t nout, uint64_t* nclipped,
                                             frbch_ps_cand* cands, uint64_t cap, uint64_t* ncand, uint32_t* kernel_used,
                                             char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  PsPlan pl;
  if ((rc = ps_check(par, nout, fil->tsamp_s, &pl, e)) != 0) return rc;
  if (!rows || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if (!ndm || ndm > 65535) return e.fail(FRBCH_E_ARG, "ndm must be 1..65535");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_out = hs.out(series_out, (size_t)ndm * nout * sizeof(float));          // (series_out may be null: no download then)
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the rows");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload rows");
  rc = frbch_dedisperse_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, device, d_out, nout, nclipped, err, err_cap);
  hs.drop(d_rows);                                                 // the plane stays in HBM; the rows are done with
  if (!rc && series_out && hs.download() != 0) rc = e.fail(FRBCH_E_DEVICE, "download series");
  if (!rc) rc = ps_search_run(d_out, ndm, nout, par, fil->tsamp_s, device, cands, cap, ncand, kernel_used, err, err_cap);
  return rc;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_ps_group_cands(const frbch_ps_cand* cands, uint64_t ncand, uint32_t dm_gap, frbch_ps_group* groups,
                                    uint64_t cap, uint64_t* ngroup, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!ngroup || (ncand && !cands) || (cap && !groups)) return e.fail(FRBCH_E_ARG, "null argument");
  if (dm_gap < 1 || dm_gap > 16) return e.fail(FRBCH_E_ARG, "dm_gap must be 1..16");
  for (uint64_t i = 0; i < ncand; ++i)
    if (!ps_fold_ok(cands[i].h) || !cands[i].k) return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": h must be 1, 2, 4, 8 or 16 and k positive");
  *ngroup = 0;
  if (!ncand) return FRBCH_OK;
  // sweep in order of the fundamental: record i meets the later ones within 1.5 bins; union-find joins the linked pairs
  std::vector<uint64_t> order(ncand), parent(ncand);
  for (uint64_t i = 0; i < ncand; ++i) order[i] = parent[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    if (ps_f_less(cands[a], cands[b])) return true;
    if (ps_f_less(cands[b], cands[a])) return false;
    return a < b;
  });
  auto find = [&](uint64_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  for (uint64_t i = 0; i < ncand; ++i) {
    const frbch_ps_cand& a = cands[order[i]];
    for (uint64_t j = i + 1; j < ncand; ++j) {
      const frbch_ps_cand& b = cands[order[j]];
      if (2 * ps_f_dist(a, b) > 3 * (uint64_t)a.h * b.h) break;
      const uint32_t ddm = a.dm_index > b.dm_index ? a.dm_index - b.dm_index : b.dm_index - a.dm_index;
      if (ddm > dm_gap) continue;
      const uint64_t ra = find(order[i]), rb = find(order[j]);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    }
  }
  auto better = [](const frbch_ps_cand& a, const frbch_ps_cand& b) {     // a represents a group rather than b
    if (a.sigma != b.sigma) return a.sigma > b.sigma;
    if (a.h != b.h) return a.h < b.h;
    if (a.dm_index != b.dm_index) return a.dm_index < b.dm_index;
    return a.k < b.k;
  };
  std::vector<int64_t> slot(ncand, -1);                                  // root -> index in `out`
  std::vector<frbch_ps_group> out;
  for (uint64_t i = 0; i < ncand; ++i) {
    const uint64_t r = find(i);
    const frbch_ps_cand& c = cands[i];
    if (slot[r] < 0) {
      slot[r] = (int64_t)out.size();
      frbch_ps_group g;
      memset(&g, 0, sizeof g);
      g.best = c;
      g.nmember = 1;
      g.dm_index_lo = g.dm_index_hi = c.dm_index;
      out.push_back(g);
      continue;
    }
    frbch_ps_group& g = out[(size_t)slot[r]];
    if (better(c, g.best)) g.best = c;
    ++g.nmember;
    g.dm_index_lo = std::min(g.dm_index_lo, c.dm_index);
    g.dm_index_hi = std::max(g.dm_index_hi, c.dm_index);
  }
  std::stable_sort(out.begin(), out.end(), [](const frbch_ps_group& a, const frbch_ps_group& b) {
    if (a.best.sigma != b.best.sigma) return a.best.sigma > b.best.sigma;
    if (ps_f_less(a.best, b.best)) return true;
    if (ps_f_less(b.best, a.best)) return false;
    if (a.best.dm_index != b.best.dm_index) return a.best.dm_index < b.best.dm_index;
    return a.best.h < b.best.h;
  });
  *ngroup = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) groups[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " groups, room for " + std::to_string(cap));
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// ---------------------------------------------------------------------------------------------------------------------
// acceleration search: the resampler, the periodicity search of every trial's resampled plane, grouping across DMs and trials
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr double kPaLight = 299792458.0;
constexpr uint32_t kPaMaxAcc = 1024;
constexpr uint32_t kPaMaxRows = 65534;             // series rows of a batch: the second grid dimension, kept even
constexpr uint64_t kPaBudget = 2ull << 30;         // bytes of per-row scratch a batch may take when the caller leaves the choice

// q of every trial; FRBCH_E_ARG for a list that is not strictly ascending, a trial that is not finite or out of range
int pa_check_accs(const double* accs, uint32_t nacc, uint32_t n, double tsamp, std::vector<double>* q, const PostErr& e) {
  if (!accs) return e.fail(FRBCH_E_ARG, "null argument");
  if (nacc < 1 || nacc > kPaMaxAcc) return e.fail(FRBCH_E_ARG, "nacc must be 1..1024");
  q->resize(nacc);
  for (uint32_t i = 0; i < nacc; ++i) {
    const double a = accs[i];
    if (!(fabs(a) <= std::numeric_limits<double>::max())) return e.fail(FRBCH_E_ARG, "trial " + std::to_string(i) + ": the acceleration is not finite");
    if (i && !(a > accs[i - 1])) return e.fail(FRBCH_E_ARG, "the trial accelerations must be strictly ascending (trial " + std::to_string(i) + ")");
    const double qi = (a * tsamp) / (2.0 * 299792458.0);
    if (!(fabs(qi) * (double)n <= 0.5)) {
      char buf[160];
      snprintf(buf, sizeof buf, "trial %u: |a| = %.9g m/s^2 is too large for n = %u samples of %.9g s: the largest is %.9g m/s^2", i,
               fabs(a), n, tsamp, kPaLight / ((double)n * tsamp));
      return e.fail(FRBCH_E_ARG, buf);
    }
    (*q)[i] = qi;
  }
  return FRBCH_OK;
}

int pa_check_n(uint32_t n, uint64_t nout, const PostErr& e) {
  if ((n & (n - 1)) || n < (1u << kPsMinLog) || n > (1u << kPsMaxLog) || n > nout)
    return e.fail(FRBCH_E_ARG, "n must be a power of two in 2^12..2^22 and at most nout");
  return FRBCH_OK;
}

// the one decision behind the resampler's launch and frbch_resample_kernel's answer; the emulator build has no fast form
bool res_fast(const float* d_series, uint64_t nout, const float* d_out) {
#ifndef FRBCH_NO_FAST
  return ((uintptr_t)d_series % 16) == 0 && ((uintptr_t)d_out % 16) == 0 && nout % 4 == 0;
#else
  (void)d_series; (void)nout; (void)d_out;
  return false;
#endif
}

// `trials` trials of rp.rows_per_trial rows each (at most 65535 rows), rp.q and rp.out at the first of them
int res_launch(bool fast, const ResParams& rp, uint32_t trials, dev_stream_t s, const PostErr& e) {
  const uint32_t rows = trials * (uint32_t)rp.rows_per_trial;
#ifndef FRBCH_NO_FAST
  if (fast) hipLaunchKernelGGL(fast::frbch_post_resample_lds, dim3(rp.n / fast::kResTile, rows), dim3(fast::kResThreads), 0, s, rp);
#endif
  if (!fast) DEV_LAUNCH(frbch_post_resample, rp.n / 256, rows, 256, 0, s, rp);
  POST_DEV(dev_check_launch(), "launch resampler");
  return FRBCH_OK;
}

struct PaPlan {
  uint32_t rpt = 0, tpb = 0, nbatch = 0;           // rows of a trial (even), trials of a batch, batches
  uint64_t row_bytes = 0, scratch = 0;
};

void pa_plan(uint32_t ndm, uint32_t n, uint32_t nacc, uint32_t batch_rows, PaPlan* a) {
  a->rpt = ndm + (ndm & 1u);
  // a row of a batch: its resampled samples, its half of a pair's work array, its powers, its mean and its live word
  a->row_bytes = (uint64_t)n * 4 + (uint64_t)n * 4 + (uint64_t)(n / 2) * 4 + sizeof(double) + sizeof(uint32_t);
  uint64_t rows = batch_rows ? batch_rows : kPaBudget / a->row_bytes;
  rows = std::min<uint64_t>(rows, kPaMaxRows);
  a->tpb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nacc, rows / a->rpt));
  a->nbatch = (nacc + a->tpb - 1) / a->tpb;
  a->scratch = (uint64_t)a->tpb * a->rpt * a->row_bytes + (uint64_t)n * sizeof(float) + (uint64_t)nacc * sizeof(double) +
               (uint64_t)kPsRawCap * sizeof(PsPeak) + sizeof(uint32_t);
}

int pa_check(const frbch_ps_params* par, uint32_t ndm, uint64_t nout, double tsamp_default, const double* accs, uint32_t nacc,
             PsPlan* pl, std::vector<double>* q, const PostErr& e) {
  int rc = ps_check(par, nout, tsamp_default, pl, e);
  if (rc) return rc;
  if (!ndm || ndm > kPaMaxRows) return e.fail(FRBCH_E_ARG, "ndm must be 1..65534");
  return pa_check_accs(accs, nacc, pl->n, pl->tsamp, q, e);
}

int pa_search_run(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, double tsamp_default,
                  const double* accs, uint32_t nacc, uint32_t batch_rows, int device, frbch_pa_cand* cands, uint64_t cap,
                  uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  PsPlan pl;
  std::vector<double> q;
  int rc = pa_check(par, ndm, nout, tsamp_default, accs, nacc, &pl, &q, e);
  if (rc) return rc;
  if (!d_series || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const uint32_t n = pl.n, nh = n / 2;
  PaPlan ap;
  pa_plan(ndm, n, nacc, batch_rows, &ap);
  const uint32_t rows_max = ap.tpb * ap.rpt;
  PsParams p;
  memset(&p, 0, sizeof p);
  p.nout = n;                                      // the resampled plane: rows of n samples
  p.log2n = pl.log2n;
  p.n = n;
  p.wblock = pl.wblock; p.nblk = pl.nblk; p.kmin = pl.kmin; p.nfold = pl.nfold;
  while ((1u << p.logb) < pl.wblock) ++p.logb;
  frbch_psearch_thresholds(par->sigma, p.thr);
  p.peak_cap = kPsRawCap;
  const std::shared_ptr<const std::vector<float>> tw = ps_table(n);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  float *d_tw = nullptr, *d_res = nullptr;
  double* d_q = nullptr;
  if (ps.alloc(&d_tw, (size_t)n * sizeof(float)) || ps.alloc(&d_q, (size_t)nacc * sizeof(double)) ||
      ps.alloc(&d_res, (size_t)rows_max * n * sizeof(float)) || ps.alloc(&p.mean, (size_t)rows_max * sizeof(double)) ||
      ps.alloc(&p.live, (size_t)rows_max * sizeof(uint32_t)) || ps.alloc(&p.work, (size_t)(rows_max / 2) * n * 2 * sizeof(float)) ||
      ps.alloc(&p.pw, (size_t)rows_max * nh * sizeof(float)) || ps.alloc(&p.peaks, (size_t)kPsRawCap * sizeof(PsPeak)) ||
      ps.alloc(&p.npeak, sizeof(uint32_t)))
    return e.fail(FRBCH_E_NOMEM, "device memory for the acceleration search: " + std::to_string(ap.scratch) + " bytes for batches of " +
                                     std::to_string(rows_max) + " rows (a smaller batch_rows takes less)");
  p.tw = d_tw;
  p.series = d_res;
  POST_DEV(dev_h2d(d_tw, tw->data(), (size_t)n * sizeof(float), s), "upload table");
  POST_DEV(dev_h2d(d_q, q.data(), (size_t)nacc * sizeof(double), s), "upload trials");
  ResParams rp;
  memset(&rp, 0, sizeof rp);
  rp.series = d_series;
  rp.nout = nout;
  rp.n = n;
  rp.ndm = (int)ndm;
  rp.rows_per_trial = (int)ap.rpt;
  rp.out = d_res;
  const bool rfast = res_fast(d_series, nout, d_res), fast = ps_fast(d_res);
  int r[3];
  const int npass = fast ? ps_passes(pl.log2n, r) : 0;
  std::vector<std::vector<frbch_ps_cand>> per(nacc);
  std::vector<PsPeak> raw;
  for (uint32_t first = 0; first < nacc; first += ap.tpb) {
    const uint32_t trials = std::min(ap.tpb, nacc - first), rows = trials * ap.rpt;
    rp.q = d_q + first;
    p.ndm = (int)rows;
    p.npair = (int)(rows / 2);
    POST_DEV(dev_memset(p.npeak, 0, sizeof(uint32_t), s), "clear peak count");
    if ((rc = res_launch(rfast, rp, trials, s, e)) != 0) return rc;
    if ((rc = ps_launches(p, pl, fast, npass, r, s, e)) != 0) return rc;
    uint32_t nraw = 0;
    POST_DEV(dev_d2h(&nraw, p.npeak, sizeof nraw, s), "download peak count");
    POST_DEV(dev_sync(s), "sync");
    if (nraw > kPsRawCap)
      return e.fail(FRBCH_E_CAPACITY, "threshold too low: " + std::to_string(nraw) + " raw peaks in the batch of trials " +
                                          std::to_string(first) + " .. " + std::to_string(first + trials - 1) +
                                          ", the device list holds " + std::to_string(kPsRawCap) + " per batch");
    raw.resize(nraw);
    if (nraw) {
      POST_DEV(dev_d2h(raw.data(), p.peaks, (size_t)nraw * sizeof(PsPeak), s), "download peaks");
      POST_DEV(dev_sync(s), "sync");
    }
    for (uint32_t i = 0; i < nraw; ++i) {
      frbch_ps_cand c;
      memset(&c, 0, sizeof c);
      c.dm_index = raw[i].dm % ap.rpt; c.h = raw[i].h; c.k = raw[i].k; c.power = raw[i].H;
      per[first + raw[i].dm / ap.rpt].push_back(c);
    }
  }
  ps.release();                           // the device is done with; the host goes on with the raw lists
  if (kernel_used) { kernel_used[0] = rfast ? 1u : 0u; kernel_used[1] = fast ? 1u : 0u; kernel_used[2] = (uint32_t)npass; }
  std::vector<frbch_pa_cand> out;
  for (uint32_t i = 0; i < nacc; ++i) {   // step 8 of every trial on its own
    std::vector<frbch_ps_cand> kept;
    ps_sift(per[i], n, pl.tsamp, &kept);
    for (const frbch_ps_cand& c : kept) {
      frbch_pa_cand o;
      memset(&o, 0, sizeof o);
      o.dm_index = c.dm_index; o.acc_index = i; o.h = c.h; o.k = c.k; o.power = c.power;
      o.sigma = c.sigma; o.freq_hz = c.freq_hz; o.acc_ms2 = accs[i];
      out.push_back(o);
    }
  }
  *ncand = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) cands[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " candidates, room for " + std::to_string(cap));
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_resample_kernel(const float* d_series, uint64_t nout, const float* d_out) {
  if (!d_series || !d_out || !nout) return FRBCH_E_ARG;
  return res_fast(d_series, nout, d_out) ? 1 : 0;
}

extern "C" int frbch_resample_device(const float* d_series, uint32_t ndm, uint64_t nout, uint32_t n, double tsamp_s,
                                     const double* accs, uint32_t nacc, int device, float* d_out, uint32_t* kernel_used,
                                     char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = pa_check_n(n, nout, e);
  if (rc) return rc;
  if (!(tsamp_s > 0.0) || !(tsamp_s < 1.0e300)) return e.fail(FRBCH_E_ARG, "tsamp_s must be positive");
  if (!d_series || !d_out) return e.fail(FRBCH_E_ARG, "null argument");
  if (!ndm || ndm > 65535) return e.fail(FRBCH_E_ARG, "ndm must be 1..65535");
  std::vector<double> q;
  if ((rc = pa_check_accs(accs, nacc, n, tsamp_s, &q, e)) != 0) return rc;
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  double* d_q = nullptr;
  if (ps.alloc(&d_q, (size_t)nacc * sizeof(double))) return e.fail(FRBCH_E_NOMEM, "device memory for the trials");
  POST_DEV(dev_h2d(d_q, q.data(), (size_t)nacc * sizeof(double), ps.s), "upload trials");
  ResParams rp;
  memset(&rp, 0, sizeof rp);
  rp.series = d_series;
  rp.nout = nout;
  rp.n = n;
  rp.ndm = (int)ndm;
  rp.rows_per_trial = (int)ndm;
  const bool fast = res_fast(d_series, nout, d_out);
  const uint32_t step = std::max<uint32_t>(1, 65535u / ndm);           // trials of a launch: at most 65535 rows
  for (uint32_t first = 0; first < nacc; first += step) {
    rp.q = d_q + first;
    rp.out = d_out + (size_t)first * ndm * n;
    if ((rc = res_launch(fast, rp, std::min(step, nacc - first), ps.s, e)) != 0) return rc;
  }
  POST_DEV(dev_sync(ps.s), "sync");
  if (kernel_used) kernel_used[0] = fast ? 1u : 0u;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_resample_host(const float* series, uint32_t ndm, uint64_t nout, uint32_t n, double tsamp_s, const double* accs,
                                   uint32_t nacc, int device, float* out, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = pa_check_n(n, nout, e);
  if (rc) return rc;
  if (!(tsamp_s > 0.0) || !(tsamp_s < 1.0e300)) return e.fail(FRBCH_E_ARG, "tsamp_s must be positive");
  if (!series || !out || !ndm || ndm > 65535) return e.fail(FRBCH_E_ARG, "null argument, or ndm outside 1..65535");
  std::vector<double> q;
  if ((rc = pa_check_accs(accs, nacc, n, tsamp_s, &q, e)) != 0) return rc;
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  float* d_series = hs.in(series, (size_t)ndm * nout * sizeof(float));
  float* d_out = hs.out(out, (size_t)nacc * ndm * n * sizeof(float));
  return hs.run(e, "device memory for the series and the resampled planes", "upload series", "download resampled planes", [&]() {
    return frbch_resample_device(d_series, ndm, nout, n, tsamp_s, accs, nacc, device, d_out, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_pasearch_plan(uint32_t ndm, uint64_t nout, const frbch_ps_params* par, uint32_t nacc, uint32_t batch_rows,
                                   uint32_t* n, uint32_t* rows_per_batch, uint32_t* nbatch, uint64_t* scratch_bytes, char* err,
                                   size_t err_cap) {
  PostErr e{err, err_cap};
  PsPlan pl;
  const int rc = ps_check(par, nout, 1.0, &pl, e);
  if (rc) return rc;
  if (!ndm || ndm > kPaMaxRows) return e.fail(FRBCH_E_ARG, "ndm must be 1..65534");
  if (nacc < 1 || nacc > kPaMaxAcc) return e.fail(FRBCH_E_ARG, "nacc must be 1..1024");
  PaPlan ap;
  pa_plan(ndm, pl.n, nacc, batch_rows, &ap);
  if (n) *n = pl.n;
  if (rows_per_batch) *rows_per_batch = ap.tpb * ap.rpt;
  if (nbatch) *nbatch = ap.nbatch;
  if (scratch_bytes) *scratch_bytes = ap.scratch;
  return FRBCH_OK;
}

extern "C" int frbch_pasearch_device(const float* d_series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par,
                                     const double* accs, uint32_t nacc, uint32_t batch_rows, int device, frbch_pa_cand* cands,
                                     uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap) try {
  return pa_search_run(d_series, ndm, nout, par, 0.0, accs, nacc, batch_rows, device, cands, cap, ncand, kernel_used, err, err_cap);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_pasearch_host(const float* series, uint32_t ndm, uint64_t nout, const frbch_ps_params* par, const double* accs,
                                   uint32_t nacc, uint32_t batch_rows, int device, frbch_pa_cand* cands, uint64_t cap,
                                   uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  PsPlan pl;
  std::vector<double> q;
  int rc = pa_check(par, ndm, nout, 0.0, accs, nacc, &pl, &q, e);
  if (rc) return rc;
  if (!series) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  float* d_series = hs.in(series, (size_t)ndm * nout * sizeof(float));
  return hs.run(e, "device memory for the series", "upload series", "download", [&]() {
    return frbch_pasearch_device(d_series, ndm, nout, par, accs, nacc, batch_rows, device, cands, cap, ncand, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dedisperse_pasearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms,
                                              uint32_t ndm, uint32_t zerodm, double clip_sigma, const frbch_ps_params* par,
                                              const double* accs, uint32_t nacc, uint32_t batch_rows, int device,
                                              float* series_out, uint64_t nout, uint64_t* nclipped, frbch_pa_cand* cands,
                                              uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  PsPlan pl;
  std::vector<double> q;
  if ((rc = pa_check(par, ndm, nout, fil->tsamp_s, accs, nacc, &pl, &q, e)) != 0) return rc;
  if (!rows || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_out = hs.out(series_out, (size_t)ndm * nout * sizeof(float));          // (series_out may be null: no download then)
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the rows");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload rows");
  rc = frbch_dedisperse_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, device, d_out, nout, nclipped, err, err_cap);
  hs.drop(d_rows);                                                 // the plane stays in HBM; the rows are done with
  if (!rc && series_out && hs.download() != 0) rc = e.fail(FRBCH_E_DEVICE, "download series");
  if (!rc) rc = pa_search_run(d_out, ndm, nout, par, fil->tsamp_s, accs, nacc, batch_rows, device, cands, cap, ncand, kernel_used, err, err_cap);
  return rc;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_pa_group_cands(const frbch_pa_cand* cands, uint64_t ncand, uint32_t dm_gap, uint32_t acc_gap,
                                    frbch_pa_group* groups, uint64_t cap, uint64_t* ngroup, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!ngroup || (ncand && !cands) || (cap && !groups)) return e.fail(FRBCH_E_ARG, "null argument");
  if (dm_gap < 1 || dm_gap > 16) return e.fail(FRBCH_E_ARG, "dm_gap must be 1..16");
  if (acc_gap < 1 || acc_gap > 16) return e.fail(FRBCH_E_ARG, "acc_gap must be 1..16");
  for (uint64_t i = 0; i < ncand; ++i)
    if (!ps_fold_ok(cands[i].h) || !cands[i].k) return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": h must be 1, 2, 4, 8 or 16 and k positive");
  *ngroup = 0;
  if (!ncand) return FRBCH_OK;
  auto f_less = [](const frbch_pa_cand& a, const frbch_pa_cand& b) { return (uint64_t)a.k * b.h < (uint64_t)b.k * a.h; };
  auto f_dist = [](const frbch_pa_cand& a, const frbch_pa_cand& b) {
    const uint64_t x = (uint64_t)a.k * b.h, y = (uint64_t)b.k * a.h;
    return x > y ? x - y : y - x;
  };
  // the sweep of frbch_ps_group_cands, with the distance in trials as a third condition
  std::vector<uint64_t> order(ncand), parent(ncand);
  for (uint64_t i = 0; i < ncand; ++i) order[i] = parent[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    if (f_less(cands[a], cands[b])) return true;
    if (f_less(cands[b], cands[a])) return false;
    return a < b;
  });
  auto find = [&](uint64_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  for (uint64_t i = 0; i < ncand; ++i) {
    const frbch_pa_cand& a = cands[order[i]];
    for (uint64_t j = i + 1; j < ncand; ++j) {
      const frbch_pa_cand& b = cands[order[j]];
      if (2 * f_dist(a, b) > 3 * (uint64_t)a.h * b.h) break;
      const uint32_t ddm = a.dm_index > b.dm_index ? a.dm_index - b.dm_index : b.dm_index - a.dm_index;
      const uint32_t dacc = a.acc_index > b.acc_index ? a.acc_index - b.acc_index : b.acc_index - a.acc_index;
      if (ddm > dm_gap || dacc > acc_gap) continue;
      const uint64_t ra = find(order[i]), rb = find(order[j]);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    }
  }
  auto better = [](const frbch_pa_cand& a, const frbch_pa_cand& b) {     // a represents a group rather than b
    if (a.sigma != b.sigma) return a.sigma > b.sigma;
    if (a.h != b.h) return a.h < b.h;
    if (a.dm_index != b.dm_index) return a.dm_index < b.dm_index;
    if (a.acc_index != b.acc_index) return a.acc_index < b.acc_index;
    return a.k < b.k;
  };
  std::vector<int64_t> slot(ncand, -1);                                  // root -> index in `out`
  std::vector<frbch_pa_group> out;
  for (uint64_t i = 0; i < ncand; ++i) {
    const uint64_t r = find(i);
    const frbch_pa_cand& c = cands[i];
    if (slot[r] < 0) {
      slot[r] = (int64_t)out.size();
      frbch_pa_group g;
      memset(&g, 0, sizeof g);
      g.best = c;
      g.nmember = 1;
      g.dm_index_lo = g.dm_index_hi = c.dm_index;
      g.acc_index_lo = g.acc_index_hi = c.acc_index;
      out.push_back(g);
      continue;
    }
    frbch_pa_group& g = out[(size_t)slot[r]];
    if (better(c, g.best)) g.best = c;
    ++g.nmember;
    g.dm_index_lo = std::min(g.dm_index_lo, c.dm_index);
    g.dm_index_hi = std::max(g.dm_index_hi, c.dm_index);
    g.acc_index_lo = std::min(g.acc_index_lo, c.acc_index);
    g.acc_index_hi = std::max(g.acc_index_hi, c.acc_index);
  }
  std::stable_sort(out.begin(), out.end(), [&](const frbch_pa_group& a, const frbch_pa_group& b) {
    if (a.best.sigma != b.best.sigma) return a.best.sigma > b.best.sigma;
    if (f_less(a.best, b.best)) return true;
    if (f_less(b.best, a.best)) return false;
    if (a.best.dm_index != b.best.dm_index) return a.best.dm_index < b.best.dm_index;
    if (a.best.acc_index != b.best.acc_index) return a.best.acc_index < b.best.acc_index;
    return a.best.h < b.best.h;
  });
  *ngroup = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) groups[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " groups, room for " + std::to_string(cap));
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// ---------------------------------------------------------------------------------------------------------------------
// candidates: grouping across DMs (host only) and the two cut-out planes
// ---------------------------------------------------------------------------------------------------------------------
namespace {
bool sp_better(const frbch_sp_cand& a, const frbch_sp_cand& b) {        // a represents a group rather than b
  if (a.sigma != b.sigma) return a.sigma > b.sigma;
  if (a.width != b.width) return a.width < b.width;
  if (a.dm_index != b.dm_index) return a.dm_index < b.dm_index;
  return a.sample < b.sample;
}
// The link rule of frbch_sp_group_cands on records with dm_index, sample and width (frbch_sp_cand, frbch_spb_cand):
// -> for every record the smallest index of its group, the connected component of the link graph.
template <class Rec> std::vector<uint64_t> sp_link(const frbch_fil_desc* fil, const double* dms, uint32_t ndm, const Rec* cands,
                                                   uint64_t ncand, uint32_t dm_gap) {
  // D_i: the largest delay of DM i, and the largest |D_a - D_b| two linked records can have
  int64_t maxd = 0;
  const std::vector<int32_t> delays = post_delays(fil, dms, ndm, &maxd);
  std::vector<int64_t> D(ndm, 0);
  for (uint32_t i = 0; i < ndm; ++i)
    for (uint32_t c = 0; c < fil->nchan; ++c) D[i] = std::max<int64_t>(D[i], delays[(size_t)i * fil->nchan + c]);
  int64_t smear = 0;
  for (uint32_t i = 0; i < ndm; ++i)
    for (uint32_t j = i + 1; j < ndm && j - i <= dm_gap; ++j) smear = std::max<int64_t>(smear, std::llabs(D[i] - D[j]));
  uint32_t wmax = 0;
  for (uint64_t i = 0; i < ncand; ++i) wmax = std::max(wmax, cands[i].width);
  const uint64_t reach = (uint64_t)(wmax / 2) + (uint64_t)smear;       // no two linked records lie further apart
  // sweep in sample order: record i meets the later ones within `reach`; union-find joins the linked pairs
  std::vector<uint64_t> order(ncand), parent(ncand);
  for (uint64_t i = 0; i < ncand; ++i) order[i] = parent[i] = i;
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    return cands[a].sample != cands[b].sample ? cands[a].sample < cands[b].sample : a < b;
  });
  auto find = [&](uint64_t x) {
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
  };
  for (uint64_t i = 0; i < ncand; ++i) {
    const Rec& a = cands[order[i]];
    for (uint64_t j = i + 1; j < ncand && cands[order[j]].sample - a.sample <= reach; ++j) {
      const Rec& b = cands[order[j]];
      const uint32_t ddm = a.dm_index > b.dm_index ? a.dm_index - b.dm_index : b.dm_index - a.dm_index;
      if (ddm > dm_gap) continue;
      const uint64_t tol = (uint64_t)(std::max(a.width, b.width) / 2) + (uint64_t)std::llabs(D[a.dm_index] - D[b.dm_index]);
      if (b.sample - a.sample > tol) continue;
      const uint64_t ra = find(order[i]), rb = find(order[j]);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    }
  }
  std::vector<uint64_t> root(ncand);
  for (uint64_t i = 0; i < ncand; ++i) root[i] = find(i);
  return root;
}
}  // namespace

extern "C" int frbch_sp_group_cands(const frbch_fil_desc* fil, const double* dms, uint32_t ndm, const frbch_sp_cand* cands,
                                    uint64_t ncand, uint32_t dm_gap, frbch_sp_group* groups, uint64_t cap, uint64_t* ngroup,
                                    char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, 1, e);
  if (rc) return rc;
  if (!dms || !ndm || !ngroup || (ncand && !cands) || (cap && !groups)) return e.fail(FRBCH_E_ARG, "null argument");
  if (dm_gap < 1 || dm_gap > 16) return e.fail(FRBCH_E_ARG, "dm_gap must be 1..16");
  for (uint32_t i = 0; i < ndm; ++i)
    if (!(dms[i] >= 0.0) || !(dms[i] < 1.0e5)) return e.fail(FRBCH_E_ARG, "a DM outside [0, 1e5)");
  for (uint64_t i = 0; i < ncand; ++i)
    if (cands[i].dm_index >= ndm) return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": dm_index >= ndm");
  *ngroup = 0;
  if (!ncand) return FRBCH_OK;
  const std::vector<uint64_t> root = sp_link(fil, dms, ndm, cands, ncand, dm_gap);
  std::vector<int64_t> slot(ncand, -1);                                  // root -> index in `out`
  std::vector<frbch_sp_group> out;
  for (uint64_t i = 0; i < ncand; ++i) {
    const uint64_t r = root[i];
    const frbch_sp_cand& c = cands[i];
    if (slot[r] < 0) {
      slot[r] = (int64_t)out.size();
      frbch_sp_group g;
      memset(&g, 0, sizeof g);
      g.best = c;
      g.best.reserved = 0;
      g.nmember = 1;
      g.dm_index_lo = g.dm_index_hi = c.dm_index;
      g.sample_lo = g.sample_hi = c.sample;
      out.push_back(g);
      continue;
    }
    frbch_sp_group& g = out[(size_t)slot[r]];
    if (sp_better(c, g.best)) { g.best = c; g.best.reserved = 0; }
    ++g.nmember;
    g.dm_index_lo = std::min(g.dm_index_lo, c.dm_index);
    g.dm_index_hi = std::max(g.dm_index_hi, c.dm_index);
    g.sample_lo = std::min(g.sample_lo, c.sample);
    g.sample_hi = std::max(g.sample_hi, c.sample);
  }
  std::sort(out.begin(), out.end(), [](const frbch_sp_group& a, const frbch_sp_group& b) {
    if (a.best.dm_index != b.best.dm_index) return a.best.dm_index < b.best.dm_index;
    if (a.best.sample != b.best.sample) return a.best.sample < b.best.sample;
    if (a.best.width != b.best.width) return a.best.width < b.best.width;
    return a.sample_lo < b.sample_lo;                                    // (two groups with the same best key: duplicate records apart)
  });
  *ngroup = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) groups[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " groups, room for " + std::to_string(cap));
  return FRBCH_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// band-limited single-pulse search: the series of every range of sub-bands, their search in batches of DMs, the grouping
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct BandPlan {
  uint32_t nsub = 0, cps = 0, wmin = 0, wmax = 0;
  std::vector<uint16_t> ab;              // [nband][2] (a, b), ascending a, then b
  uint32_t nband() const { return (uint32_t)(ab.size() / 2); }
};

int band_check(uint32_t nchan, const frbch_band_params* bp, BandPlan* plan, const PostErr& e) {
  if (!bp || bp->size != sizeof(frbch_band_params)) return e.fail(FRBCH_E_ARG, "frbch_band_params: wrong size");
  if (bp->nsub < 1 || bp->nsub > 16) return e.fail(FRBCH_E_ARG, "nsub must be 1..16");
  if (!nchan || nchan % bp->nsub != 0) return e.fail(FRBCH_E_ARG, "nsub must divide nchan");
  plan->nsub = bp->nsub;
  plan->cps = nchan / bp->nsub;
  plan->wmin = bp->min_sub ? bp->min_sub : 1;
  plan->wmax = bp->max_sub ? bp->max_sub : bp->nsub;
  if (plan->wmax > bp->nsub) return e.fail(FRBCH_E_ARG, "max_sub exceeds nsub");
  if (plan->wmin > plan->wmax) return e.fail(FRBCH_E_ARG, "min_sub exceeds max_sub");
  plan->ab.clear();
  for (uint32_t a = 0; a < bp->nsub; ++a)
    for (uint32_t b = a + plan->wmin; b <= bp->nsub && b - a <= plan->wmax; ++b) {
      plan->ab.push_back((uint16_t)a);
      plan->ab.push_back((uint16_t)b);
    }
  return FRBCH_OK;
}

// everything frbch_dedisperse_bands_* and frbch_bandsearch_* refuse before the device is looked at; fills *plan
int bands_check(const frbch_fil_desc* fil, uint64_t nrows, const double* dms, uint32_t ndm, const frbch_band_params* bp,
                BandPlan* plan, uint64_t nout, const PostErr& e) {
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!dms || !ndm) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = band_check(fil->nchan, bp, plan, e)) != 0) return rc;
  if ((uint64_t)ndm * plan->nband() > 65535)
    return e.fail(FRBCH_E_ARG, "ndm * nband = " + std::to_string((uint64_t)ndm * plan->nband()) + " series, the search takes 65535");
  const long want = frbch_dedisperse_nout(fil, nrows, dms, ndm);
  if (want < 0) return e.fail(FRBCH_E_ARG, "a DM outside [0, 1e5)");
  if (want == 0) return e.fail(FRBCH_E_ARG, "the largest dispersion delay exceeds the data");
  if ((uint64_t)want != nout) return e.fail(FRBCH_E_CAPACITY, "nout must be frbch_dedisperse_nout()");
  return FRBCH_OK;
}

// Which form a run of DMs takes -- the one decision behind the launch, *kernel_used and frbch_dedisperse_bands_kernel's
// answer.  true = the tiled prefix kernel + the range kernel: integer rows, a running sum that fits uint32, a sub-band of whole
// channel tiles, and the tiled dedispersion's own conditions (post_dedisp_tiled; *range is its table).
bool bands_tiled(const frbch_fil_desc* fil, const void* d_rows, const std::vector<int32_t>& delays, uint32_t ndm, const BandPlan& plan,
                 std::vector<int32_t>* range) {
  if (fil->nbits != 8 && fil->nbits != 16) return false;
  if (fil->nchan > 65536 || plan.cps % (64 / (fil->nbits / 8)) != 0) return false;
  return post_dedisp_tiled(fil, d_rows, delays, ndm, range);
}

#ifndef FRBCH_NO_FAST
template <int B> int launch_bands_tiled(bool flagged, bool zerodm, dim3 grid, size_t lds, dev_stream_t s, const PostParams& p) {
  if (flagged && zerodm) return launch_lds(fast::frbch_post_dedisp_bands_tiled<B, true, true>, grid, dim3(256), lds, s, p);
  if (flagged) return launch_lds(fast::frbch_post_dedisp_bands_tiled<B, true, false>, grid, dim3(256), lds, s, p);
  if (zerodm) return launch_lds(fast::frbch_post_dedisp_bands_tiled<B, false, true>, grid, dim3(256), lds, s, p);
  return launch_lds(fast::frbch_post_dedisp_bands_tiled<B, false, false>, grid, dim3(256), lds, s, p);
}
#endif

// What a bands dedispersion holds on the device next to the pre-pass: the band list, and per run of at most `ndm_cap` DMs the
// delays, the tile table and the prefix planes of the tiled form (allocated when a run first takes it).
struct BandsDev {
  uint16_t* d_ab = nullptr;
  int32_t *d_delays = nullptr, *d_range = nullptr;
  uint32_t* d_pre = nullptr;
  double* d_prez = nullptr;
  uint32_t ndm_cap = 0;
};

int bands_dev_init(PostScope& ps, const PostErr& e, const frbch_fil_desc* fil, const BandPlan& plan, uint32_t ndm_cap, BandsDev* bd) {
  bd->ndm_cap = ndm_cap;
  POST_DEV(ps.alloc(&bd->d_ab, plan.ab.size() * sizeof(uint16_t)), "hipMalloc");
  POST_DEV(dev_h2d(bd->d_ab, plan.ab.data(), plan.ab.size() * sizeof(uint16_t), ps.s), "upload bands");
  POST_DEV(ps.alloc(&bd->d_delays, (size_t)ndm_cap * fil->nchan * sizeof(int32_t)), "hipMalloc");
  return FRBCH_OK;
}

// One run of consecutive DMs on the stream of `ps`, behind the pre-pass (p holds its results): d_out [ndm * nband][nout].
// Synchronous: the stream is idle when it returns.  *tiled_out: the form taken.
int bands_run(PostScope& ps, const PostErr& e, const frbch_fil_desc* fil, const void* d_rows, PostParams p, const BandPlan& plan,
              BandsDev& bd, const double* dms, uint32_t ndm, float* d_out, bool* tiled_out) {
  const dev_stream_t s = ps.s;
  int64_t maxd = 0;
  const std::vector<int32_t> delays = post_delays(fil, dms, ndm, &maxd);
  POST_DEV(dev_h2d(bd.d_delays, delays.data(), delays.size() * sizeof(int32_t), s), "upload delays");
  p.delays = bd.d_delays;
  p.out = d_out;
  p.ndm = (int)ndm;
  p.band_ab = bd.d_ab;
  p.nband = (int)plan.nband();
  p.bsub = (int)plan.nsub;
  p.cps = (int)plan.cps;
  p.bw_min = (int)plan.wmin;
  p.bw_max = (int)plan.wmax;
  std::vector<int32_t> range;
  const bool tiled = bands_tiled(fil, d_rows, delays, ndm, plan, &range);
#ifndef FRBCH_NO_FAST
  if (tiled) {
    const int bpv = fil->nbits / 8, ngrp = (int)((ndm + fast::kDedND - 1) / fast::kDedND);
    const size_t ngrp_cap = (bd.ndm_cap + fast::kDedND - 1) / fast::kDedND, nct = fil->nchan / (64 / bpv);
    const size_t npre = (size_t)bd.ndm_cap * plan.nsub * p.nout;
    if (!bd.d_range) POST_DEV(ps.alloc(&bd.d_range, ngrp_cap * nct * 2 * sizeof(int32_t)), "hipMalloc");
    if (!bd.d_pre) POST_DEV(ps.alloc(&bd.d_pre, npre * sizeof(uint32_t)), "hipMalloc");
    if (p.zerodm && !bd.d_prez) POST_DEV(ps.alloc(&bd.d_prez, npre * sizeof(double)), "hipMalloc");
    POST_DEV(dev_h2d(bd.d_range, range.data(), range.size() * sizeof(int32_t), s), "upload tile ranges");
    POST_DEV(dev_sync(s), "sync");
    p.tile_range = bd.d_range;
    p.pre = bd.d_pre;
    p.prez = bd.d_prez;
    const size_t lds = (size_t)fast::kDedRowsCap * fast::kDedRowB + 16 + (size_t)fast::kDedRowsCap * 9;
    const unsigned gx = (unsigned)((p.nout + fast::kDedTT - 1) / fast::kDedTT);
    const bool fl = p.flagged != nullptr, zd = p.zerodm != 0;
    const int refused = bpv == 1 ? launch_bands_tiled<1>(fl, zd, dim3(gx, (unsigned)ngrp), lds, s, p)
                                 : launch_bands_tiled<2>(fl, zd, dim3(gx, (unsigned)ngrp), lds, s, p);
    POST_DEV(refused, "LDS size");
    POST_DEV(dev_check_launch(), "launch band prefixes");
    const dim3 grid(gx, (unsigned)plan.nband(), ndm);
    if (zd) hipLaunchKernelGGL(fast::frbch_post_bands_ranges<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(fast::frbch_post_bands_ranges<false>, grid, dim3(256), 0, s, p);
  }
#endif
  if (!tiled) DEV_LAUNCH(frbch_post_dedisp_bands, (p.nout + 255) / 256, ndm, 256, 0, s, p);
  POST_DEV(dev_check_launch(), "launch band series");
  POST_DEV(dev_sync(s), "sync");                                   // (the host's delays and tile table were read)
  *tiled_out = tiled;
  return FRBCH_OK;
}

// the parameters of the pre-pass and of every run behind it
PostParams bands_params(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, double* d_rowsum, uint64_t nout, uint32_t zerodm) {
  PostParams p = post_params<PostParams>(fil, d_rows, nrows);
  p.prod = (int)fil->product;
  p.rowsum = d_rowsum;
  p.nout = nout;
  p.zerodm = zerodm ? 1 : 0;
  p.rows_per_chunk = kPostChunkRows;
  return p;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" int frbch_band_list(uint32_t nchan, const frbch_band_params* bands, uint16_t* sub_lo, uint16_t* sub_hi, uint32_t cap,
                               uint32_t* nband, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  BandPlan plan;
  const int rc = band_check(nchan, bands, &plan, e);
  if (rc) return rc;
  if (!nband || (cap && (!sub_lo || !sub_hi))) return e.fail(FRBCH_E_ARG, "null argument");
  *nband = plan.nband();
  for (uint32_t j = 0; j < std::min(cap, plan.nband()); ++j) {
    sub_lo[j] = plan.ab[2 * j];
    sub_hi[j] = plan.ab[2 * j + 1];
  }
  if (plan.nband() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(plan.nband()) + " bands, room for " + std::to_string(cap));
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dedisperse_bands_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms,
                                             uint32_t ndm, const frbch_band_params* bands) try {
  PostErr e{nullptr, 0};
  BandPlan plan;
  const long nout = frbch_dedisperse_nout(fil, nrows, dms, ndm);
  if (!d_rows || nout <= 0 || bands_check(fil, nrows, dms, ndm, bands, &plan, (uint64_t)nout, e)) return FRBCH_E_ARG;
  int64_t maxd = 0;
  const std::vector<int32_t> delays = post_delays(fil, dms, ndm, &maxd);
  std::vector<int32_t> range;
  return bands_tiled(fil, d_rows, delays, ndm, plan, &range) ? 1 : 0;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_dedisperse_bands_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms,
                                             uint32_t ndm, uint32_t zerodm, double clip_sigma, const frbch_band_params* bands,
                                             int device, float* d_out, uint64_t nout, uint64_t* nclipped, uint32_t* kernel_used,
                                             char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  BandPlan plan;
  int rc = bands_check(fil, nrows, dms, ndm, bands, &plan, nout, e);
  if (rc) return rc;
  if (!d_rows || !d_out) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  double* d_rowsum = nullptr;
  POST_DEV(ps.alloc(&d_rowsum, nrows * sizeof(double)), "hipMalloc");
  PostParams p = bands_params(fil, d_rows, nrows, d_rowsum, nout, zerodm);
  uint64_t nflag = 0;
  if ((rc = post_dedisp_prepass(ps, e, fil, nrows, zerodm, clip_sigma, p, &nflag)) != 0) return rc;
  BandsDev bd;
  if ((rc = bands_dev_init(ps, e, fil, plan, ndm, &bd)) != 0) return rc;
  bool tiled = false;
  if ((rc = bands_run(ps, e, fil, d_rows, p, plan, bd, dms, ndm, d_out, &tiled)) != 0) return rc;
  if (nclipped) *nclipped = nflag;
  if (kernel_used) *kernel_used = tiled ? 1 : 0;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dedisperse_bands_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms,
                                           uint32_t ndm, uint32_t zerodm, double clip_sigma, const frbch_band_params* bands,
                                           int device, float* out, uint64_t nout, uint64_t* nclipped, uint32_t* kernel_used,
                                           char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  BandPlan plan;
  int rc = bands_check(fil, nrows, dms, ndm, bands, &plan, nout, e);
  if (rc) return rc;
  if (!rows || !out) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_out = hs.out(out, (size_t)ndm * plan.nband() * nout * sizeof(float));
  return hs.run(e, "device memory for the rows", "upload rows", "download series", [&]() {
    return frbch_dedisperse_bands_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, bands, device, d_out, nout, nclipped,
                                         kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_bandsearch_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                       uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, const frbch_sp_params* sp,
                                       uint64_t plane_bytes, int device, uint64_t nout, uint64_t* nclipped, frbch_spb_cand* cands,
                                       uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, uint32_t* nbatch, double* stage_ms,
                                       char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  BandPlan plan;
  int rc = bands_check(fil, nrows, dms, ndm, bands, &plan, nout, e);
  if (rc) return rc;
  uint64_t blk_len = 0;
  if ((rc = sp_check(sp, &blk_len, e)) != 0) return rc;
  if (!d_rows || !ncand || (cap && !cands)) return e.fail(FRBCH_E_ARG, "null argument");
  const uint64_t one = (uint64_t)plan.nband() * nout * sizeof(float), budget = plane_bytes ? plane_bytes : 1ull << 30;
  if (budget < one)
    return e.fail(FRBCH_E_ARG, "plane_bytes = " + std::to_string(budget) + " holds no DM: one DM's plane takes " + std::to_string(one));
  const uint32_t per = (uint32_t)std::min<uint64_t>(ndm, budget / one);
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps(false);
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  auto t0 = std::chrono::steady_clock::now();
  double ms[3] = {0.0, 0.0, 0.0};
  double* d_rowsum = nullptr;
  float* d_plane = nullptr;
  POST_DEV(ps.alloc(&d_rowsum, nrows * sizeof(double)), "hipMalloc");
  PostParams p = bands_params(fil, d_rows, nrows, d_rowsum, nout, zerodm);
  uint64_t nflag = 0;
  if ((rc = post_dedisp_prepass(ps, e, fil, nrows, zerodm, clip_sigma, p, &nflag)) != 0) return rc;
  BandsDev bd;
  if ((rc = bands_dev_init(ps, e, fil, plan, per, &bd)) != 0) return rc;
  POST_DEV(ps.alloc(&d_plane, (size_t)per * one), "hipMalloc");
  POST_DEV(dev_sync(ps.s), "sync");
  ms[0] = ms_since(t0);
  std::vector<frbch_sp_cand> part;
  uint64_t total = 0;
  uint32_t nb = 0, search_kernel = 0;
  bool all_tiled = true;
  for (uint32_t d0 = 0; d0 < ndm; d0 += per, ++nb) {
    const uint32_t n = std::min(per, ndm - d0);
    bool tiled = false;
    t0 = std::chrono::steady_clock::now();
    if ((rc = bands_run(ps, e, fil, d_rows, p, plan, bd, dms + d0, n, d_plane, &tiled)) != 0) return rc;
    ms[1] += ms_since(t0);
    all_tiled = all_tiled && tiled;
    t0 = std::chrono::steady_clock::now();
    part.clear();
    uint64_t npart = 0;
    if ((rc = sp_search_run(d_plane, n * plan.nband(), nout, sp, device, nullptr, 0, &npart, &search_kernel, &part, err, err_cap)) != 0)
      return rc;
    ms[2] += ms_since(t0);
    for (const frbch_sp_cand& c : part) {               // series = dm * nband + j, sorted by (series, sample, width) already
      if (total < cap) {
        const uint32_t j = c.dm_index % plan.nband();
        frbch_spb_cand r;
        r.dm_index = d0 + c.dm_index / plan.nband();
        r.width = c.width;
        r.sample = c.sample;
        r.sigma = c.sigma;
        r.sub_lo = plan.ab[2 * j];
        r.sub_hi = plan.ab[2 * j + 1];
        cands[total] = r;
      }
      ++total;
    }
  }
  *ncand = total;
  if (nclipped) *nclipped = nflag;
  if (kernel_used) { kernel_used[0] = all_tiled ? 1 : 0; kernel_used[1] = search_kernel; }
  if (nbatch) *nbatch = nb;
  if (stage_ms) for (int i = 0; i < 3; ++i) stage_ms[i] = ms[i];
  if (total > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(total) + " candidates, room for " + std::to_string(cap));
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_bandsearch_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                     uint32_t zerodm, double clip_sigma, const frbch_band_params* bands, const frbch_sp_params* sp,
                                     uint64_t plane_bytes, int device, uint64_t nout, uint64_t* nclipped, frbch_spb_cand* cands,
                                     uint64_t cap, uint64_t* ncand, uint32_t* kernel_used, uint32_t* nbatch, double* stage_ms,
                                     char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  BandPlan plan;
  int rc = bands_check(fil, nrows, dms, ndm, bands, &plan, nout, e);
  if (rc) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  return hs.run(e, "device memory for the rows", "upload rows", "download", [&]() {
    return frbch_bandsearch_device(fil, d_rows, nrows, dms, ndm, zerodm, clip_sigma, bands, sp, plane_bytes, device, nout, nclipped,
                                   cands, cap, ncand, kernel_used, nbatch, stage_ms, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

namespace {
bool spb_better(const frbch_spb_cand& a, const frbch_spb_cand& b) {     // a represents a group rather than b
  if (a.sigma != b.sigma) return a.sigma > b.sigma;
  const int wa = a.sub_hi - a.sub_lo, wb = b.sub_hi - b.sub_lo;
  if (wa != wb) return wa < wb;
  if (a.width != b.width) return a.width < b.width;
  if (a.dm_index != b.dm_index) return a.dm_index < b.dm_index;
  if (a.sample != b.sample) return a.sample < b.sample;
  return a.sub_lo < b.sub_lo;
}
}  // namespace

extern "C" int frbch_spb_group_cands(const frbch_fil_desc* fil, const double* dms, uint32_t ndm, uint32_t nsub,
                                     const frbch_spb_cand* cands, uint64_t ncand, uint32_t dm_gap, frbch_spb_group* groups,
                                     uint64_t cap, uint64_t* ngroup, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = post_check_fil(fil, 1, e);
  if (rc) return rc;
  if (!dms || !ndm || !ngroup || (ncand && !cands) || (cap && !groups)) return e.fail(FRBCH_E_ARG, "null argument");
  if (dm_gap < 1 || dm_gap > 16) return e.fail(FRBCH_E_ARG, "dm_gap must be 1..16");
  if (nsub < 1 || nsub > 16) return e.fail(FRBCH_E_ARG, "nsub must be 1..16");
  for (uint32_t i = 0; i < ndm; ++i)
    if (!(dms[i] >= 0.0) || !(dms[i] < 1.0e5)) return e.fail(FRBCH_E_ARG, "a DM outside [0, 1e5)");
  for (uint64_t i = 0; i < ncand; ++i) {
    if (cands[i].dm_index >= ndm) return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": dm_index >= ndm");
    if (cands[i].sub_lo >= cands[i].sub_hi || cands[i].sub_hi > nsub)
      return e.fail(FRBCH_E_ARG, "record " + std::to_string(i) + ": not a band of " + std::to_string(nsub) + " sub-bands");
  }
  *ngroup = 0;
  if (!ncand) return FRBCH_OK;
  const std::vector<uint64_t> root = sp_link(fil, dms, ndm, cands, ncand, dm_gap);
  std::vector<int64_t> slot(ncand, -1);                                  // root -> index in `out`
  std::vector<frbch_spb_group> out;
  for (uint64_t i = 0; i < ncand; ++i) {
    const frbch_spb_cand& c = cands[i];
    const bool full = c.sub_lo == 0 && c.sub_hi == nsub;
    if (slot[root[i]] < 0) {
      slot[root[i]] = (int64_t)out.size();
      frbch_spb_group g;
      memset(&g, 0, sizeof g);
      g.best = c;
      g.nmember = 1;
      g.dm_index_lo = g.dm_index_hi = c.dm_index;
      g.sub_lo_min = c.sub_lo;
      g.sub_hi_max = c.sub_hi;
      g.sample_lo = g.sample_hi = c.sample;
      g.full_sigma = full ? c.sigma : 0.0f;
      out.push_back(g);
      continue;
    }
    frbch_spb_group& g = out[(size_t)slot[root[i]]];
    if (spb_better(c, g.best)) g.best = c;
    ++g.nmember;
    g.dm_index_lo = std::min(g.dm_index_lo, c.dm_index);
    g.dm_index_hi = std::max(g.dm_index_hi, c.dm_index);
    g.sub_lo_min = std::min(g.sub_lo_min, c.sub_lo);
    g.sub_hi_max = std::max(g.sub_hi_max, c.sub_hi);
    g.sample_lo = std::min(g.sample_lo, c.sample);
    g.sample_hi = std::max(g.sample_hi, c.sample);
    if (full) g.full_sigma = std::max(g.full_sigma, c.sigma);
  }
  std::sort(out.begin(), out.end(), [](const frbch_spb_group& a, const frbch_spb_group& b) {
    if (a.best.dm_index != b.best.dm_index) return a.best.dm_index < b.best.dm_index;
    if (a.best.sample != b.best.sample) return a.best.sample < b.best.sample;
    if (a.best.width != b.best.width) return a.best.width < b.best.width;
    if (a.best.sub_lo != b.best.sub_lo) return a.best.sub_lo < b.best.sub_lo;
    if (a.best.sub_hi != b.best.sub_hi) return a.best.sub_hi < b.best.sub_hi;
    return a.sample_lo < b.sample_lo;
  });
  *ngroup = out.size();
  for (uint64_t i = 0; i < std::min<uint64_t>(cap, out.size()); ++i) groups[i] = out[i];
  if (out.size() > cap) return e.fail(FRBCH_E_CAPACITY, std::to_string(out.size()) + " groups, room for " + std::to_string(cap));
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

namespace {
constexpr uint64_t kCutTableCap = 1ull << 26;   // delay-table entries of one call (256 MiB); a longer batch is refused

// the part of cut_check that needs no candidate (frbch_candidates_* refuse a bad `cut` before they have any)
int cut_check_par(const frbch_fil_desc* fil, const frbch_cutout_params* par, const PostErr& e) {
  if (!par || par->size != sizeof(frbch_cutout_params)) return e.fail(FRBCH_E_ARG, "frbch_cutout_params: wrong size");
  if (par->nt < 2 || par->nt > 1024 || (par->nt & 1)) return e.fail(FRBCH_E_ARG, "nt must be even, 2..1024");
  if (par->nf < 1 || fil->nchan % par->nf != 0) return e.fail(FRBCH_E_ARG, "nf must divide nchan");
  if (par->ndm < 1 || par->ndm > 1024) return e.fail(FRBCH_E_ARG, "ndm must be 1..1024");
  return FRBCH_OK;
}

int cut_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_cutout_params* par, const frbch_cutout_cand* cands,
              uint32_t ncand, const PostErr& e) {
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  rc = cut_check_par(fil, par, e);
  if (rc) return rc;
  if (!cands || ncand < 1 || ncand > 65535) return e.fail(FRBCH_E_ARG, "1..65535 candidates");
  if ((uint64_t)ncand * par->nf * par->nt >= (1ull << 31) || (uint64_t)ncand * par->ndm * par->nt >= (1ull << 31))
    return e.fail(FRBCH_E_ARG, "a plane set of 2^31 elements or more");
  if ((uint64_t)ncand * par->ndm * fil->nchan > kCutTableCap)
    return e.fail(FRBCH_E_ARG, "ncand * ndm * nchan exceeds 2^26 delays: cut the batch into several calls");
  if (nrows >= (1ull << 62)) return e.fail(FRBCH_E_ARG, "too many rows");
  for (uint32_t i = 0; i < ncand; ++i) {
    const frbch_cutout_cand& c = cands[i];
    const std::string who = "candidate " + std::to_string(i) + ": ";
    if (c.tfactor < 1 || c.tfactor > 512) return e.fail(FRBCH_E_ARG, who + "tfactor must be 1..512");
    if (!(c.dm >= 0.0) || !(c.dm < 1.0e5) || !(c.dm_lo >= 0.0) || !(c.dm_lo < 1.0e5) || !(c.dm_hi >= 0.0) || !(c.dm_hi < 1.0e5))
      return e.fail(FRBCH_E_ARG, who + "a DM outside [0, 1e5)");
    if (c.dm_hi < c.dm_lo) return e.fail(FRBCH_E_ARG, who + "dm_hi < dm_lo");
    if (c.sample < -(1ll << 62) || c.sample > (1ll << 62)) return e.fail(FRBCH_E_ARG, who + "sample out of range");
  }
  return FRBCH_OK;
}

// what the kernels of a call read
struct CutPlan {
  std::vector<CutCand> cand;
  std::vector<int32_t> ft_delays, dt_delays;     // [count][nchan], [count][ndm][nchan]
  bool lds = false;                              // every tile of both planes fits the LDS kernel
  std::vector<int32_t> ft_range, dt_range;       // [count][row group][channel tile] (smallest delay, span; span < 0: not the group's)
  int ft_ngrp = 0, dt_ngrp = 0, nct = 0;
  int ft_rows = 0, dt_rows = 0;                  // rows of the largest tile
  unsigned ft_tiles = 1, dt_tiles = 1;           // time tiles of the candidate that needs most
};

// Which cut-out kernel a call takes -- the one decision behind frbch_cutout_device's launches, *kernel_used and
// frbch_cutout_kernel's answer.  true = the LDS kernel (kernels_post_fast.inc): 8- / 16-bit rows, whole 64-byte channel
// tiles, 16-byte pieces of every row (only the ADDRESS of d_rows is examined).  cut_build then still has to find room in
// the LDS for every (row group, channel tile, time tile).  The emulator build has no such kernel: false.
bool cut_lds_layout(const frbch_fil_desc* fil, const void* d_rows) {
#ifndef FRBCH_NO_FAST
  if (fil->nbits != 8 && fil->nbits != 16) return false;
  const int bpv = fil->nbits / 8, ct = 64 / bpv;
  return fil->nchan % ct == 0 && (int)fil->nchan <= fast::kCutMaxChan && ((uintptr_t)d_rows % 16) == 0 &&
         ((size_t)fil->nifs * fil->nchan * bpv) % 16 == 0;
#else
  (void)fil; (void)d_rows;
  return false;
#endif
}

// min / span of delays[r][c] over r in [0, nr) (rows `pitch` apart), c in [c0, c1) -> range[0..1]; false: does not fit
bool cut_tile_range(const int32_t* delays, int nr, size_t pitch, int c0, int c1, int32_t* range, int* rows_max) {
#ifndef FRBCH_NO_FAST
  int32_t lo = INT32_MAX, hi = INT32_MIN;
  for (int r = 0; r < nr; ++r)
    for (int c = c0; c < c1; ++c) {
      const int32_t v = delays[(size_t)r * pitch + c];
      lo = std::min(lo, v);
      hi = std::max(hi, v);
    }
  range[0] = lo;
  range[1] = hi - lo;
  if ((int64_t)hi - lo + fast::kCutTT > fast::kCutRowsCap) return false;
  *rows_max = std::max(*rows_max, fast::kCutTT + (hi - lo));
  return true;
#else
  (void)delays; (void)nr; (void)pitch; (void)c0; (void)c1; (void)range; (void)rows_max;
  return false;
#endif
}

int cut_build(const frbch_fil_desc* fil, const frbch_cutout_params* par, const frbch_cutout_cand* cands, uint32_t count,
              bool layout_ok, CutPlan* plan, const PostErr& e) {
  POST_NO_CONTRACT
  const uint32_t ndm = par->ndm;
  // the DMs of both planes, then their delays from post_delays: n_c(.) is what frbch_dedisperse_* computes because it is
  // computed by the same function
  std::vector<double> ft_dms(count), dt_dms((size_t)count * ndm);
  plan->cand.resize(count);
  for (uint32_t i = 0; i < count; ++i) {
    const frbch_cutout_cand& c = cands[i];
    plan->cand[i].t0 = c.sample - (long long)(par->nt / 2) * (long long)c.tfactor;
    plan->cand[i].tfactor = (int)c.tfactor;
    plan->cand[i].pad = 0;
    ft_dms[i] = c.dm;
    const double step = ndm > 1 ? (c.dm_hi - c.dm_lo) / (double)(ndm - 1) : 0.0;
    for (uint32_t k = 0; k < ndm; ++k) {
      const double off = (double)k * step;
      dt_dms[(size_t)i * ndm + k] = ndm > 1 ? c.dm_lo + off : c.dm_lo;
    }
  }
  int64_t ft_max = 0, dt_max = 0;
  plan->ft_delays = post_delays(fil, ft_dms.data(), count, &ft_max);
  plan->dt_delays = post_delays(fil, dt_dms.data(), count * ndm, &dt_max);
  if (std::max(ft_max, dt_max) > (int64_t)1 << 30) return e.fail(FRBCH_E_ARG, "a dispersion delay of more than 2^30 samples");
  plan->lds = false;
#ifndef FRBCH_NO_FAST
  if (layout_ok) {
    const uint32_t nchan = fil->nchan;
    const int ct = 64 / (fil->nbits / 8), nct = (int)nchan / ct, cpb = (int)(nchan / par->nf);
    const int NR = fast::kCutNR;
    plan->nct = nct;
    plan->ft_ngrp = ((int)par->nf + NR - 1) / NR;
    plan->dt_ngrp = ((int)ndm + NR - 1) / NR;
    plan->ft_range.assign((size_t)count * plan->ft_ngrp * nct * 2, -1);
    plan->dt_range.assign((size_t)count * plan->dt_ngrp * nct * 2, -1);
    plan->ft_rows = plan->dt_rows = fast::kCutTT;
    plan->ft_tiles = plan->dt_tiles = 1;
    bool fits = true;
    for (uint32_t i = 0; i < count && fits; ++i) {
      const int f = plan->cand[i].tfactor, bpt = f >= fast::kCutTT ? 1 : fast::kCutTT / f;
      const unsigned tiles = (unsigned)((par->nt + bpt - 1) / bpt);
      plan->ft_tiles = std::max(plan->ft_tiles, tiles);
      plan->dt_tiles = std::max(plan->dt_tiles, tiles);
      for (int g = 0; g < plan->dt_ngrp && fits; ++g) {
        const int nd = std::min(NR, (int)ndm - g * NR);
        for (int k = 0; k < nct && fits; ++k)
          fits = cut_tile_range(&plan->dt_delays[((size_t)i * ndm + (size_t)g * NR) * nchan], nd, nchan, k * ct, (k + 1) * ct,
                                &plan->dt_range[(((size_t)i * plan->dt_ngrp + g) * nct + k) * 2], &plan->dt_rows);
      }
      for (int g = 0; g < plan->ft_ngrp && fits; ++g) {
        const int c_lo = g * NR * cpb, c_hi = std::min((int)nchan, (g + 1) * NR * cpb);
        for (int k = c_lo / ct; k <= (c_hi - 1) / ct && fits; ++k)
          fits = cut_tile_range(&plan->ft_delays[(size_t)i * nchan], 1, nchan, std::max(c_lo, k * ct), std::min(c_hi, (k + 1) * ct),
                                &plan->ft_range[(((size_t)i * plan->ft_ngrp + g) * nct + k) * 2], &plan->ft_rows);
      }
    }
    plan->lds = fits;
  }
#else
  (void)layout_ok;
#endif
  return FRBCH_OK;
}

}  // namespace

extern "C" int frbch_cutout_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_cutout_params* par,
                                   const frbch_cutout_cand* cands, uint32_t ncand) {
  PostErr e{nullptr, 0};
  int rc = cut_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  CutPlan plan;
  rc = cut_build(fil, par, cands, ncand, cut_lds_layout(fil, d_rows), &plan, e);
  return rc ? rc : (plan.lds ? 1 : 0);
}

extern "C" int frbch_cutout_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_cutout_params* par,
                                   const frbch_cutout_cand* cands, uint32_t ncand, int device, float* d_ft, uint32_t* d_ft_hits,
                                   float* d_dt, uint32_t* d_dt_hits, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = cut_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!d_rows || !d_ft || !d_ft_hits || !d_dt || !d_dt_hits) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  CutPlan plan;
  rc = cut_build(fil, par, cands, ncand, cut_lds_layout(fil, d_rows), &plan, e);
  if (rc) return rc;
  const bool lds = plan.lds;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  CutCand* d_cand = nullptr;
  int32_t *d_ftd = nullptr, *d_dtd = nullptr;
  POST_DEV(ps.alloc(&d_cand, plan.cand.size() * sizeof(CutCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_ftd, plan.ft_delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dtd, plan.dt_delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_cand, plan.cand.data(), plan.cand.size() * sizeof(CutCand), s), "upload candidates");
  POST_DEV(dev_h2d(d_ftd, plan.ft_delays.data(), plan.ft_delays.size() * sizeof(int32_t), s), "upload delays");
  POST_DEV(dev_h2d(d_dtd, plan.dt_delays.data(), plan.dt_delays.size() * sizeof(int32_t), s), "upload delays");
  CutParams p = post_params<CutParams>(fil, d_rows, nrows);
  p.prod = (int)fil->product;
  p.nt = (int)par->nt; p.nf = (int)par->nf; p.ndm = (int)par->ndm; p.cpb = (int)(fil->nchan / par->nf);
  p.ncand = (int)ncand;
  p.cand = d_cand;
  p.ft_delays = d_ftd;
  p.dt_delays = d_dtd;
#ifndef FRBCH_NO_FAST
  if (lds) {
    int32_t *d_ftr = nullptr, *d_dtr = nullptr;
    POST_DEV(ps.alloc(&d_ftr, plan.ft_range.size() * sizeof(int32_t)), "hipMalloc");
    POST_DEV(ps.alloc(&d_dtr, plan.dt_range.size() * sizeof(int32_t)), "hipMalloc");
    POST_DEV(dev_h2d(d_ftr, plan.ft_range.data(), plan.ft_range.size() * sizeof(int32_t), s), "upload tile ranges");
    POST_DEV(dev_h2d(d_dtr, plan.dt_range.data(), plan.dt_range.size() * sizeof(int32_t), s), "upload tile ranges");
    p.nct = plan.nct;
    const int bpv = fil->nbits / 8;
    for (int kind = 0; kind < 2; ++kind) {
      p.kind = kind;
      p.out = kind ? d_dt : d_ft;
      p.hits = kind ? d_dt_hits : d_ft_hits;
      p.tile_range = kind ? d_dtr : d_ftr;
      p.ngrp = kind ? plan.dt_ngrp : plan.ft_ngrp;
      const size_t bytes = std::max((size_t)(kind ? plan.dt_rows : plan.ft_rows) * fast::kCutRowB, fast::kCutRedBytes) + 16;
      const dim3 grid(kind ? plan.dt_tiles : plan.ft_tiles, (unsigned)p.ngrp, ncand), block(fast::kCutTT);
      int refused;
      if (bpv == 1 && kind) refused = launch_lds(fast::frbch_post_cutout_lds<1, 1>, grid, block, bytes, s, p);
      else if (bpv == 1) refused = launch_lds(fast::frbch_post_cutout_lds<1, 0>, grid, block, bytes, s, p);
      else if (kind) refused = launch_lds(fast::frbch_post_cutout_lds<2, 1>, grid, block, bytes, s, p);
      else refused = launch_lds(fast::frbch_post_cutout_lds<2, 0>, grid, block, bytes, s, p);
      POST_DEV(refused, "LDS size");
      POST_DEV(dev_check_launch(), "launch cut-out");
    }
  }
#endif
  if (!lds)
    for (int kind = 0; kind < 2; ++kind) {
      p.kind = kind;
      p.out = kind ? d_dt : d_ft;
      p.hits = kind ? d_dt_hits : d_ft_hits;
      const uint64_t npix = (uint64_t)(kind ? par->ndm : par->nf) * par->nt;
      DEV_LAUNCH(frbch_post_cutout, (npix + 255) / 256, ncand, 256, 0, s, p);
      POST_DEV(dev_check_launch(), "launch cut-out");
    }
  POST_DEV(dev_sync(s), "sync");      // (the host vectors the uploads read stay alive until here)
  if (kernel_used) *kernel_used = lds ? 1 : 0;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_cutout_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_cutout_params* par,
                                 const frbch_cutout_cand* cands, uint32_t ncand, int device, float* ft, uint32_t* ft_hits,
                                 float* dt, uint32_t* dt_hits, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  int rc = cut_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!rows || !ft || !ft_hits || !dt || !dt_hits) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t nft = (size_t)ncand * par->nf * par->nt, ndt = (size_t)ncand * par->ndm * par->nt;
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  float* d_ft = hs.out(ft, nft * 4);
  uint32_t* d_fth = hs.out(ft_hits, nft * 4);
  float* d_dt = hs.out(dt, ndt * 4);
  uint32_t* d_dth = hs.out(dt_hits, ndt * 4);
  return hs.run(e, "device memory for the rows and the planes", "upload rows", "download planes",
                [&]() { return frbch_cutout_device(fil, d_rows, nrows, par, cands, ncand, device, d_ft, d_fth, d_dt, d_dth, kernel_used, err, err_cap); });
}

// ---------------------------------------------------------------------------------------------------------------------
// interference: block statistics, the mask, cleaned rows
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kRfiMaxBlockRows = 1u << 20;
constexpr uint32_t kRfiGridBlocks = 65535;        // blocks of one launch (grid.y)

int rfi_check(const frbch_fil_desc* f, uint64_t nrows, const frbch_rfi_params* par, uint32_t* nblk, const PostErr& e) {
  const int rc = post_check_layout(f, e);
  if (rc) return rc;
  if (!nrows) return e.fail(FRBCH_E_ARG, "no rows");
  if (!par || par->size != sizeof(frbch_rfi_params)) return e.fail(FRBCH_E_ARG, "frbch_rfi_params: wrong size");
  if (par->block_rows < 1 || par->block_rows > kRfiMaxBlockRows) return e.fail(FRBCH_E_ARG, "block_rows must be 1..2^20");
  if (!(par->t_cell >= 0) || !(par->t_chan >= 0) || std::isinf(par->t_cell) || std::isinf(par->t_chan))
    return e.fail(FRBCH_E_ARG, "t_cell and t_chan must be finite and not negative");
  if (!(par->chan_frac >= 0) || !(par->block_frac >= 0) || par->chan_frac > 1.0 || par->block_frac > 1.0)
    return e.fail(FRBCH_E_ARG, "chan_frac and block_frac must lie in 0..1");
  const uint64_t n = (nrows + par->block_rows - 1) / par->block_rows;
  if (n > 0x7FFFFFFFull || (uint64_t)f->nchan > 0x7FFFFFFFull / f->nifs) return e.fail(FRBCH_E_ARG, "too many blocks or channels");
  *nblk = (uint32_t)n;
  return FRBCH_OK;
}

// Which statistics kernel a call takes -- the one decision behind frbch_rfi_stats_device's launch, *kernel_used and
// frbch_rfi_stats_kernel's answer.  > 0 = the fast kernel (kernels_post_fast.inc) with that many bytes of the row per
// workgroup: 8- / 16-bit rows, whole 64-byte channel tiles, 16-byte pieces of every row (only the ADDRESS of d_rows is
// examined); the tile is the largest listed width that divides the row piece.  The emulator build has no such kernel: 0.
int rfi_fast_tile(const frbch_fil_desc* fil, const void* d_rows) {
#ifndef FRBCH_NO_FAST
  if (fil->nbits != 8 && fil->nbits != 16) return 0;
  const size_t bpv = (size_t)fil->nbits / 8, piece = (size_t)fil->nchan * bpv;
  if (piece % 64 != 0 || ((uintptr_t)d_rows % 16) != 0 || ((size_t)fil->nifs * piece) % 16 != 0) return 0;
  for (int w = 1024; w >= 64; w >>= 1)
    if (piece % (size_t)w == 0) return w;
  return 0;
#else
  (void)fil; (void)d_rows;
  return 0;
#endif
}

RfiParams rfi_params(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par, uint32_t nblk) {
  RfiParams p = post_params<RfiParams>(fil, d_rows, nrows);
  p.prod = (int)fil->product;
  p.block_rows = par->block_rows;
  p.nblk = nblk;
  return p;
}

// The k-th smallest of v[0 .. n) (no NaN among them); reorders v so that v[k] holds it and nothing before it is larger.
// Quickselect whose partition passes do not branch on the data: the table of a long file asks for thousands of medians.
double rfi_select(double* v, size_t n, size_t k) {
  size_t lo = 0, hi = n;
  while (hi - lo > 8) {
    const double a = v[lo], b = v[lo + (hi - lo) / 2], c = v[hi - 1];
    const double p = std::max(std::min(a, b), std::min(std::max(a, b), c));        // median of three: a value of the range
    size_t i = lo;
    for (size_t j = lo; j < hi; ++j) {                                             // [lo, i) < p <= [i, hi)
      const double x = v[j];
      v[j] = v[i];
      v[i] = x;
      i += x < p ? 1 : 0;
    }
    if (k < i) { hi = i; continue; }
    size_t m = i;
    for (size_t j = i; j < hi; ++j) {                                              // [i, m) == p < [m, hi)
      const double x = v[j];
      v[j] = v[m];
      v[m] = x;
      m += x <= p ? 1 : 0;
    }
    if (k < m) return p;
    lo = m;
  }
  for (size_t i = lo + 1; i < hi; ++i) {
    const double x = v[i];
    size_t j = i;
    for (; j > lo && v[j - 1] > x; --j) v[j] = v[j - 1];
    v[j] = x;
  }
  return v[k];
}

// 0.5 * (lower middle + upper middle) of v[0 .. n), n >= 1; reorders v
double rfi_median(double* v, size_t n) {
  const size_t k = n / 2;
  const double hi = rfi_select(v, n, k);
  double lo = hi;
  if (!(n & 1)) lo = *std::max_element(v, v + k);
  return 0.5 * (lo + hi);
}

// fn(first channel, one past the last) over all channels, on several threads when the table is large: every channel's
// result depends on that channel alone, so the split changes no bit.  (Measured on the 306 x 1024 table of a 10-s file: the
// four medians per channel are 20 ms of std::nth_element on one thread, more than the dedispersion the stage stands in
// front of; rfi_select and the split bring the decision to 2 ms.)  A thread that cannot be started runs in the caller.
template <class F>
void rfi_over_channels(uint32_t nchan, uint32_t nblk, F fn) {
  const uint64_t cells = (uint64_t)nchan * nblk;
  unsigned nt = cells >= (1u << 16) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
  nt = std::min<unsigned>(nt, nchan);
  if (nt <= 1) { fn(0u, nchan); return; }
  std::vector<std::thread> th;
  th.reserve(nt);
  const uint32_t per = (nchan + nt - 1) / nt;
  for (unsigned i = 1; i < nt; ++i) {
    if (i * per >= nchan) break;
    const uint32_t c0 = i * per, c1 = std::min(nchan, (i + 1) * per);
    try {
      th.emplace_back(fn, c0, c1);
    } catch (const std::system_error&) {
      fn(c0, c1);
    }
  }
  fn(0u, std::min(nchan, per));
  for (auto& t : th) t.join();
}
}  // namespace

extern "C" long frbch_rfi_nblk(uint64_t nrows, uint32_t block_rows) {
  if (!nrows || block_rows < 1 || block_rows > kRfiMaxBlockRows) return FRBCH_E_ARG;
  return (long)((nrows + block_rows - 1) / block_rows);
}

extern "C" int frbch_rfi_stats_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par) {
  PostErr e{nullptr, 0};
  uint32_t nblk = 0;
  const int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  return rfi_fast_tile(fil, d_rows) > 0 ? 1 : 0;
}

extern "C" int frbch_rfi_stats_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                      int device, void* d_stats, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!d_rows || !d_stats) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  RfiParams p = rfi_params(fil, d_rows, nrows, par, nblk);
  p.stats_i = (unsigned long long*)d_stats;
  p.stats_f = (double*)d_stats;
  const int tile = rfi_fast_tile(fil, d_rows);
  for (uint32_t b0 = 0; b0 < nblk; b0 += kRfiGridBlocks) {
    const uint32_t nb = std::min(kRfiGridBlocks, nblk - b0);
    p.blk0 = b0;
#ifndef FRBCH_NO_FAST
    if (tile > 0) {
      p.tile_bytes = tile;
      p.ntile = (int)((size_t)fil->nchan * (fil->nbits / 8) / (size_t)tile);
      const dim3 grid((unsigned)p.ntile, nb);
      if (fil->nbits == 8) hipLaunchKernelGGL(fast::frbch_post_rfi_stats_fast<1>, grid, dim3(fast::kRfiThreads), 0, s, p);
      else hipLaunchKernelGGL(fast::frbch_post_rfi_stats_fast<2>, grid, dim3(fast::kRfiThreads), 0, s, p);
    }
#endif
    if (tile <= 0) DEV_LAUNCH(frbch_post_rfi_stats, (fil->nchan + 255) / 256, nb, 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch statistics");
  }
  POST_DEV(dev_sync(s), "sync");
  if (kernel_used) *kernel_used = tile > 0 ? 1 : 0;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_stats_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                    int device, void* stats, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!rows || !stats) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  void* d_stats = hs.out(stats, (size_t)nblk * fil->nchan * 16);
  return hs.run(e, "device memory for the rows", "upload rows", "download statistics",
                [&]() { return frbch_rfi_stats_device(fil, d_rows, nrows, par, device, d_stats, kernel_used, err, err_cap); });
}

// The one decision (include/frbch.h, steps 1 to 8), host only: IEEE double, every operation rounded on its own.
extern "C" int frbch_rfi_mask(const frbch_fil_desc* fil, const void* stats, uint32_t nblk, uint64_t nrows, const frbch_rfi_params* par,
                              const uint8_t* zap, const uint8_t* prior, uint8_t* mask, double* repl, uint8_t* chan_flag,
                              uint8_t* blk_flag, char* err, size_t err_cap) {
  POST_NO_CONTRACT
  PostErr e{err, err_cap};
  uint32_t want = 0;
  const int rc = rfi_check(fil, nrows, par, &want, e);
  if (rc) return rc;
  if (nblk != want) return e.fail(FRBCH_E_ARG, "nblk must be frbch_rfi_nblk()");
  if (!stats || !mask || !repl || !chan_flag || !blk_flag) return e.fail(FRBCH_E_ARG, "null argument");
  const uint32_t nchan = fil->nchan;
  const bool integer_rows = fil->nbits != 32;
  const uint64_t n_last = nrows - (uint64_t)(nblk - 1) * par->block_rows;          // rows of the last block
  const double t_cell = par->t_cell;
  try {
  std::atomic<bool> oom(false);                     // (a worker's failed allocation must not leave its thread)
  // mean, std and the cell flags, [channel][block]: a channel's blocks lie side by side for the medians
  std::vector<double> mean((size_t)nchan * nblk), sdev((size_t)nchan * nblk);
  std::vector<uint8_t> bad((size_t)nchan * nblk), cell((size_t)nchan * nblk);
  std::vector<double> m_c(nchan), s_c(nchan);
  std::vector<uint32_t> nbad(nchan), ncell(nchan);
  rfi_over_channels(nchan, nblk, [&](uint32_t c0, uint32_t c1) {
    POST_NO_CONTRACT
    std::vector<double> a, w, d;
    try { a.resize(nblk); w.resize(nblk); d.resize(nblk); } catch (const std::bad_alloc&) { oom = true; return; }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t cc = c0; cc < c1; cc += 16) {                                      // step 1, 16 channels of a table row at a time
      for (uint32_t b = 0; b < nblk; ++b) {
        const double nb = (double)(b + 1 < nblk ? (uint64_t)par->block_rows : n_last);
        for (uint32_t c = cc; c < std::min(c1, cc + 16); ++c) {
          const size_t i = ((size_t)b * nchan + c) * 2;
          const double S = integer_rows ? (double)((const uint64_t*)stats)[i] : ((const double*)stats)[i];
          const double Q = integer_rows ? (double)((const uint64_t*)stats)[i + 1] : ((const double*)stats)[i + 1];
          const double m = S / nb;
          const double mm = m * m;
          const double qn = Q / nb;
          double var = qn - mm;
          if (var < 0.0) var = 0.0;                                                  // (a NaN stays a NaN)
          const double sg = sqrt(var);
          mean[(size_t)c * nblk + b] = m;
          sdev[(size_t)c * nblk + b] = sg;
          bad[(size_t)c * nblk + b] = (uint8_t)(std::isfinite(m) && std::isfinite(sg) ? 0 : 1);
        }
      }
    }
    for (uint32_t c = c0; c < c1; ++c) {
      double* mu = &mean[(size_t)c * nblk];
      double* sd = &sdev[(size_t)c * nblk];
      uint8_t* bd = &bad[(size_t)c * nblk];
      uint8_t* fl = &cell[(size_t)c * nblk];
      size_t n = 0;
      for (uint32_t b = 0; b < nblk; ++b)
        if (!bd[b]) { a[n] = mu[b]; w[n] = sd[b]; ++n; }
      nbad[c] = (uint32_t)(nblk - n);
      if (!n) {
        m_c[c] = s_c[c] = nan;
        for (uint32_t b = 0; b < nblk; ++b) fl[b] = 1;
        ncell[c] = nblk;
        continue;
      }
      for (size_t i = 0; i < n; ++i) d[i] = a[i];                                  // step 2
      const double mc = rfi_median(d.data(), n);
      for (size_t i = 0; i < n; ++i) d[i] = w[i];
      const double sc = rfi_median(d.data(), n);
      for (size_t i = 0; i < n; ++i) d[i] = fabs(a[i] - mc);
      const double dmc = 1.4826 * rfi_median(d.data(), n);
      for (size_t i = 0; i < n; ++i) d[i] = fabs(w[i] - sc);
      const double dsc = 1.4826 * rfi_median(d.data(), n);
      m_c[c] = mc;
      s_c[c] = sc;
      double lim_m[2], lim_s[2];                                                   // step 3: [0] a whole block, [1] the last one
      for (int k = 0; k < 2; ++k) {
        const double nb = (double)(k ? n_last : (uint64_t)par->block_rows);
        const double fm = sc / sqrt(nb);
        const double two_n = 2.0 * nb;
        const double fs = sc / sqrt(two_n);
        lim_m[k] = t_cell * (dmc > fm ? dmc : fm);
        lim_s[k] = t_cell * (dsc > fs ? dsc : fs);
      }
      uint32_t cnt = 0;
      for (uint32_t b = 0; b < nblk; ++b) {
        if (bd[b]) { fl[b] = 1; ++cnt; continue; }
        const int k = b + 1 < nblk ? 0 : 1;
        fl[b] = (uint8_t)((fabs(mu[b] - mc) > lim_m[k] || fabs(sd[b] - sc) > lim_s[k]) ? 1 : 0);
        cnt += fl[b];
      }
      ncell[c] = cnt;
    }
  });
  if (oom) return e.fail(FRBCH_E_NOMEM, "host memory for the mask decision");
  for (uint32_t c = 0; c < nchan; ++c)                                             // step 4
    chan_flag[c] = (uint8_t)(((zap && zap[c]) || nbad[c] == nblk || s_c[c] == 0.0) ? 1 : 0);
  if (par->t_chan > 0.0) {                                                         // step 5
    std::vector<double> v, d;
    for (uint32_t c = 0; c < nchan; ++c)
      if (!chan_flag[c]) v.push_back(s_c[c]);
    if (!v.empty()) {
      d = v;
      const double M = rfi_median(d.data(), d.size());
      for (size_t i = 0; i < v.size(); ++i) d[i] = fabs(v[i] - M);
      const double D = 1.4826 * rfi_median(d.data(), d.size());
      const double lim = par->t_chan * D;
      for (uint32_t c = 0; c < nchan; ++c)
        if (!chan_flag[c] && fabs(s_c[c] - M) > lim) chan_flag[c] = 1;
    }
  }
  const double chan_lim = par->chan_frac * (double)nblk;                           // step 6
  uint32_t n_u = 0;
  for (uint32_t c = 0; c < nchan; ++c) {
    if (!chan_flag[c] && (double)ncell[c] > chan_lim) chan_flag[c] = 1;
    n_u += chan_flag[c] ? 0u : 1u;
  }
  const double blk_lim = par->block_frac * (double)n_u;
  std::vector<uint32_t> nb_cells(nblk, 0);
  for (uint32_t c = 0; c < nchan; ++c)
    if (!chan_flag[c])
      for (uint32_t b = 0; b < nblk; ++b) nb_cells[b] += cell[(size_t)c * nblk + b];
  for (uint32_t b = 0; b < nblk; ++b) blk_flag[b] = (uint8_t)((double)nb_cells[b] > blk_lim ? 1 : 0);
  rfi_over_channels(nchan, nblk, [&](uint32_t c0, uint32_t c1) {                   // step 7 (`cell` becomes the mask, transposed)
    for (uint32_t c = c0; c < c1; ++c)
      for (uint32_t b = 0; b < nblk; ++b)
        if (chan_flag[c] || blk_flag[b]) cell[(size_t)c * nblk + b] = 1;
    for (uint32_t b = 0; b < nblk; ++b)
      for (uint32_t c = c0; c < c1; ++c) {
        const size_t i = (size_t)b * nchan + c;
        if (prior && prior[i]) cell[(size_t)c * nblk + b] = 1;
        mask[i] = cell[(size_t)c * nblk + b];
      }
  });
  const double code_max = fil->nbits == 8 ? 255.0 : 65535.0;
  rfi_over_channels(nchan, nblk, [&](uint32_t c0, uint32_t c1) {                   // step 8
    POST_NO_CONTRACT
    std::vector<double> d;
    try { d.resize(nblk); } catch (const std::bad_alloc&) { oom = true; return; }
    for (uint32_t c = c0; c < c1; ++c) {
      size_t n = 0, nmask = 0;
      for (uint32_t b = 0; b < nblk; ++b) {
        if (!cell[(size_t)c * nblk + b]) d[n++] = mean[(size_t)c * nblk + b];
        else ++nmask;
      }
      // (no masked cell: the cells of m_c, the same median; none left: m_c as well)
      double r = (n && nmask) ? rfi_median(d.data(), n) : m_c[c];
      if (!std::isfinite(r)) r = 0.0;
      if (integer_rows) {
        r = floor(r + 0.5);
        if (r < 0.0) r = 0.0;
        if (r > code_max) r = code_max;
      }
      repl[c] = r;
    }
  });
  if (oom) return e.fail(FRBCH_E_NOMEM, "host memory for the mask decision");
  } catch (const std::bad_alloc&) {
    return e.fail(FRBCH_E_NOMEM, "host memory for the mask decision");
  }
  return FRBCH_OK;
}

extern "C" int frbch_rfi_apply_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                      const uint8_t* d_mask, const double* d_repl, int device, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!d_rows || !d_mask || !d_repl) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  RfiParams p = rfi_params(fil, d_rows, nrows, par, nblk);
  p.mask = d_mask;
  p.repl = d_repl;
  for (uint32_t b0 = 0; b0 < nblk; b0 += kRfiGridBlocks) {
    p.blk0 = b0;
    DEV_LAUNCH(frbch_post_rfi_apply, (fil->nchan + 255) / 256, std::min(kRfiGridBlocks, nblk - b0), 256, 0, s, p);
    POST_DEV(dev_check_launch(), "launch apply");
  }
  POST_DEV(dev_sync(s), "sync");
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_apply_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                    const uint8_t* mask, const double* repl, int device, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!rows || !mask || !repl) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.inout(rows, post_rows_bytes(fil, nrows));
  uint8_t* d_mask = hs.in(mask, (size_t)nblk * fil->nchan);
  double* d_repl = hs.in(repl, fil->nchan * sizeof(double));
  return hs.run(e, "device memory for the rows", "upload rows", "download rows",
                [&]() { return frbch_rfi_apply_device(fil, d_rows, nrows, par, d_mask, d_repl, device, err, err_cap); });
}

extern "C" int frbch_rfi_clean_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                      const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag,
                                      uint8_t* blk_flag, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!d_rows || !mask || !repl || !chan_flag || !blk_flag) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t ncell = (size_t)nblk * fil->nchan;
  std::vector<uint64_t> stats(ncell * 2);                        // (S, Q): uint64 or double, 16 bytes a cell either way
  HostStage hs;
  void* d_stats = hs.out((void*)stats.data(), ncell * 16);
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the statistics");
  rc = frbch_rfi_stats_device(fil, d_rows, nrows, par, device, d_stats, kernel_used, err, err_cap);
  if (!rc && hs.download() != 0) rc = e.fail(FRBCH_E_DEVICE, "download statistics");
  if (!rc) rc = frbch_rfi_mask(fil, stats.data(), nblk, nrows, par, zap, nullptr, mask, repl, chan_flag, blk_flag, err, err_cap);
  if (rc || std::none_of(mask, mask + ncell, [](uint8_t m) { return m != 0; })) return rc;     // (nothing masked: nothing to write)
  uint8_t* d_mask = hs.in(mask, ncell);
  double* d_repl = hs.in(repl, fil->nchan * sizeof(double));
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the mask");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload mask");
  return frbch_rfi_apply_device(fil, d_rows, nrows, par, d_mask, d_repl, device, err, err_cap);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_clean_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                    const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag,
                                    uint8_t* blk_flag, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int rc = rfi_check(fil, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!rows || !mask || !repl || !chan_flag || !blk_flag) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.inout(rows, post_rows_bytes(fil, nrows));
  return hs.run(e, "device memory for the rows", "upload rows", "download rows",
                [&]() { return frbch_rfi_clean_device(fil, d_rows, nrows, par, zap, device, mask, repl, chan_flag, blk_flag, kernel_used, err, err_cap); });
}

// ---------------------------------------------------------------------------------------------------------------------
// interference: the periodicity test (the spectral peak of every block and channel)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kPeaksGenericThreads = 256;

// rfi_check, and block_rows as the transform length: *log2n = 3 .. 12
int rfi_pcheck(const frbch_fil_desc* f, uint64_t nrows, const frbch_rfi_params* par, uint32_t* nblk, int* log2n, const PostErr& e) {
  const int rc = rfi_check(f, nrows, par, nblk, e);
  if (rc) return rc;
  const uint32_t n = par->block_rows;
  if (n < 8 || n > 4096 || (n & (n - 1)) != 0)
    return e.fail(FRBCH_E_ARG, "the periodic test transforms whole blocks: block_rows must be a power of two in 8 .. 4096 (it is " +
                                   std::to_string(n) + "); choose such a block_rows, or flag without the periodic test");
  int L = 0;
  while ((1u << L) < n) ++L;
  *log2n = L;
  return FRBCH_OK;
}

int rfi_fcheck(const frbch_rfi_fparams* fpar, const PostErr& e) {
  if (!fpar || fpar->size != sizeof(frbch_rfi_fparams)) return e.fail(FRBCH_E_ARG, "frbch_rfi_fparams: wrong size");
  if (!(fpar->t_pow > 0) || std::isinf(fpar->t_pow)) return e.fail(FRBCH_E_ARG, "t_pow must be positive and finite");
  if (!(fpar->chan_frac >= 0) || fpar->chan_frac > 1.0) return e.fail(FRBCH_E_ARG, "chan_frac (periodic) must lie in 0..1");
  return FRBCH_OK;
}

// The one decision behind frbch_rfi_peaks_device's launch, *kernel_used and frbch_rfi_peaks_kernel's answer: the clauses of the
// fast statistics kernel, and a transform length the fast kernel has a plan for.
bool rfi_peaks_fast(const frbch_fil_desc* fil, const void* d_rows, int log2n) {
  return rfi_fast_tile(fil, d_rows) > 0 && log2n >= 8 && log2n <= 11;
}

// W[k] = ((float)cos(a), (float)(-sin(a))), a = 2.0 pi k / n in double, k < n / 2
std::vector<float> rfi_twiddles(uint32_t n) {
  std::vector<float> tw(n);
  for (uint32_t k = 0; k < n / 2; ++k) {
    const double a = 2.0 * M_PI * (double)k / (double)n;
    tw[2 * k] = (float)cos(a);
    tw[2 * k + 1] = (float)(-sin(a));
  }
  return tw;
}

#ifndef FRBCH_NO_FAST
template <int BPV> int launch_peaks_fast(int log2n, dim3 grid, dev_stream_t s, const RfiParams& p) {
  const dim3 block(fast::kPkThreads);
  switch (log2n) {
    case 8: return launch_lds(fast::frbch_post_rfi_peaks_fast<8, BPV, 4, 4, 0>, grid, block, fast::pk_lds(8), s, p);
    case 9: return launch_lds(fast::frbch_post_rfi_peaks_fast<9, BPV, 3, 3, 3>, grid, block, fast::pk_lds(9), s, p);
    case 10: return launch_lds(fast::frbch_post_rfi_peaks_fast<10, BPV, 4, 3, 3>, grid, block, fast::pk_lds(10), s, p);
    case 11: return launch_lds(fast::frbch_post_rfi_peaks_fast<11, BPV, 4, 4, 3>, grid, block, fast::pk_lds(11), s, p);
  }
  return -1;
}
#endif
}  // namespace

extern "C" int frbch_rfi_peaks_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par) {
  PostErr e{nullptr, 0};
  uint32_t nblk = 0;
  int log2n = 0;
  const int rc = rfi_pcheck(fil, nrows, par, &nblk, &log2n, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  return rfi_peaks_fast(fil, d_rows, log2n) ? 1 : 0;
}

extern "C" int frbch_rfi_peaks_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                      int device, const void* d_stats, void* d_peaks, uint32_t* kernel_used, char* err,
                                      size_t err_cap) try {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int log2n = 0;
  int rc = rfi_pcheck(fil, nrows, par, &nblk, &log2n, e);
  if (rc) return rc;
  if (!d_rows || !d_stats || !d_peaks) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const dev_stream_t s = ps.s;
  const uint32_t n = par->block_rows;
  const std::vector<float> tw = rfi_twiddles(n);
  float* d_tw = nullptr;
  if (ps.alloc(&d_tw, tw.size() * sizeof(float)) != 0) return e.fail(FRBCH_E_NOMEM, "device memory for the twiddle table");
  POST_DEV(dev_h2d(d_tw, tw.data(), tw.size() * sizeof(float), s), "upload the twiddle table");
  RfiParams p = rfi_params(fil, d_rows, nrows, par, nblk);
  p.stats_i = (unsigned long long*)d_stats;                      // (read only)
  p.stats_f = (double*)d_stats;
  p.peaks = (RfiPeak*)d_peaks;
  p.tw = d_tw;
  p.log2n = log2n;
  const bool fast_k = rfi_peaks_fast(fil, d_rows, log2n);
  for (uint32_t b0 = 0; b0 < nblk; b0 += kRfiGridBlocks) {
    const uint32_t nb = std::min(kRfiGridBlocks, nblk - b0);
    p.blk0 = b0;
#ifndef FRBCH_NO_FAST
    if (fast_k) {
      const size_t piece = (size_t)fast::pk_piece(log2n);
      const dim3 grid((unsigned)((size_t)fil->nchan * (fil->nbits / 8) / piece), nb);
      const int lr = fil->nbits == 8 ? launch_peaks_fast<1>(log2n, grid, s, p) : launch_peaks_fast<2>(log2n, grid, s, p);
      if (lr != 0) return e.fail(FRBCH_E_DEVICE, "the LDS of the peaks kernel was refused");
    }
#endif
    if (!fast_k)
      DEV_LAUNCH(frbch_post_rfi_peaks, (fil->nchan + 1) / 2, nb, kPeaksGenericThreads, (size_t)n * 8 + 2 * kPeaksGenericThreads * sizeof(RfiPeak), s, p);
    POST_DEV(dev_check_launch(), "launch peaks");
  }
  POST_DEV(dev_sync(s), "sync");
  if (kernel_used) *kernel_used = fast_k ? 1 : 0;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_peaks_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                    int device, void* stats, void* peaks, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int log2n = 0;
  int rc = rfi_pcheck(fil, nrows, par, &nblk, &log2n, e);
  if (rc) return rc;
  if (!rows || !peaks) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t ncell = (size_t)nblk * fil->nchan;
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  void* d_stats = hs.out(stats, ncell * 16);                     // (no host array: not downloaded)
  void* d_peaks = hs.out(peaks, ncell * sizeof(frbch_rfi_peak));
  return hs.run(e, "device memory for the rows", "upload rows", "download peaks", [&]() {
    uint32_t used[2] = {0, 0};
    int r = frbch_rfi_stats_device(fil, d_rows, nrows, par, device, d_stats, &used[0], err, err_cap);
    if (!r) r = frbch_rfi_peaks_device(fil, d_rows, nrows, par, device, d_stats, d_peaks, &used[1], err, err_cap);
    if (!r && kernel_used) { kernel_used[0] = used[0]; kernel_used[1] = used[1]; }
    return r;
  });
}

// The decision on the peaks (include/frbch.h), host only: IEEE double, every operation rounded on its own.
extern "C" int frbch_rfi_periodic(const frbch_fil_desc* fil, const void* stats, const void* peaks, uint32_t nblk, uint64_t nrows,
                                  const frbch_rfi_params* par, const frbch_rfi_fparams* fpar, uint8_t* pflag, uint8_t* pchan,
                                  double* power, char* err, size_t err_cap) try {
  POST_NO_CONTRACT
  PostErr e{err, err_cap};
  uint32_t want = 0;
  int log2n = 0;
  int rc = rfi_pcheck(fil, nrows, par, &want, &log2n, e);
  if (rc) return rc;
  if ((rc = rfi_fcheck(fpar, e)) != 0) return rc;
  if (nblk != want) return e.fail(FRBCH_E_ARG, "nblk must be frbch_rfi_nblk()");
  if (!stats || !peaks || !pflag || !pchan) return e.fail(FRBCH_E_ARG, "null argument");
  const uint32_t nchan = fil->nchan;
  const bool integer_rows = fil->nbits != 32;
  const uint64_t n = par->block_rows;
  const uint64_t n_last = nrows - (uint64_t)(nblk - 1) * n;
  const frbch_rfi_peak* pk = (const frbch_rfi_peak*)peaks;
  std::vector<uint32_t> count(nchan, 0);
  for (uint32_t b = 0; b < nblk; ++b) {
    const uint64_t rows_b = b + 1 < nblk ? n : n_last;
    const double nb = (double)rows_b;
    const double four_nb = 4.0 * nb;
    for (uint32_t c = 0; c < nchan; ++c) {
      const size_t cell = (size_t)b * nchan + c, i = cell * 2;
      const double S = integer_rows ? (double)((const uint64_t*)stats)[i] : ((const double*)stats)[i];
      const double Q = integer_rows ? (double)((const uint64_t*)stats)[i + 1] : ((const double*)stats)[i + 1];
      const double m = S / nb;
      const double mm = m * m;
      const double qn = Q / nb;
      double var = qn - mm;
      if (var < 0.0) var = 0.0;
      double p = 0.0;
      if (2 * rows_b >= n && std::isfinite(m) && std::isfinite(var) && var != 0.0) {
        const double den = four_nb * var;
        p = (double)pk[cell].num / den;
      }
      if (power) power[cell] = p;
      pflag[cell] = (uint8_t)(p > fpar->t_pow ? 1 : 0);
      count[c] += pflag[cell];
    }
  }
  const double chan_lim = fpar->chan_frac * (double)nblk;
  for (uint32_t c = 0; c < nchan; ++c) pchan[c] = (uint8_t)((double)count[c] > chan_lim ? 1 : 0);
  for (uint32_t b = 0; b < nblk; ++b)
    for (uint32_t c = 0; c < nchan; ++c)
      if (pchan[c]) pflag[(size_t)b * nchan + c] = 1;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_cleanf_device(const frbch_fil_desc* fil, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                       const frbch_rfi_fparams* fpar, const uint8_t* zap, int device, uint8_t* mask, double* repl,
                                       uint8_t* chan_flag, uint8_t* blk_flag, uint8_t* pflag, uint8_t* pchan, void* peaks,
                                       uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int log2n = 0;
  int rc = rfi_pcheck(fil, nrows, par, &nblk, &log2n, e);
  if (rc) return rc;
  if ((rc = rfi_fcheck(fpar, e)) != 0) return rc;
  if (!d_rows || !mask || !repl || !chan_flag || !blk_flag || !pflag || !pchan) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t ncell = (size_t)nblk * fil->nchan;
  std::vector<uint64_t> stats(ncell * 2);
  std::vector<frbch_rfi_peak> own;
  if (!peaks) own.resize(ncell);
  void* pk = peaks ? peaks : (void*)own.data();
  HostStage hs;
  void* d_stats = hs.out((void*)stats.data(), ncell * 16);
  void* d_peaks = hs.out(pk, ncell * sizeof(frbch_rfi_peak));
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the statistics and the peaks");
  uint32_t used[2] = {0, 0};
  rc = frbch_rfi_stats_device(fil, d_rows, nrows, par, device, d_stats, &used[0], err, err_cap);
  if (!rc) rc = frbch_rfi_peaks_device(fil, d_rows, nrows, par, device, d_stats, d_peaks, &used[1], err, err_cap);
  if (!rc && hs.download() != 0) rc = e.fail(FRBCH_E_DEVICE, "download statistics and peaks");
  if (!rc) rc = frbch_rfi_periodic(fil, stats.data(), pk, nblk, nrows, par, fpar, pflag, pchan, nullptr, err, err_cap);
  if (!rc) rc = frbch_rfi_mask(fil, stats.data(), nblk, nrows, par, zap, pflag, mask, repl, chan_flag, blk_flag, err, err_cap);
  if (rc) return rc;
  for (uint32_t c = 0; c < fil->nchan; ++c) chan_flag[c] = (uint8_t)(chan_flag[c] | pchan[c]);
  if (kernel_used) { kernel_used[0] = used[0]; kernel_used[1] = used[1]; }
  if (std::none_of(mask, mask + ncell, [](uint8_t m) { return m != 0; })) return FRBCH_OK;       // (nothing masked: nothing to write)
  uint8_t* d_mask = hs.in(mask, ncell);
  double* d_repl = hs.in(repl, fil->nchan * sizeof(double));
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory for the mask");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload mask");
  return frbch_rfi_apply_device(fil, d_rows, nrows, par, d_mask, d_repl, device, err, err_cap);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_cleanf_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                     const frbch_rfi_fparams* fpar, const uint8_t* zap, int device, uint8_t* mask, double* repl,
                                     uint8_t* chan_flag, uint8_t* blk_flag, uint8_t* pflag, uint8_t* pchan, void* peaks,
                                     uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  uint32_t nblk = 0;
  int log2n = 0;
  int rc = rfi_pcheck(fil, nrows, par, &nblk, &log2n, e);
  if (rc) return rc;
  if ((rc = rfi_fcheck(fpar, e)) != 0) return rc;
  if (!rows || !mask || !repl || !chan_flag || !blk_flag || !pflag || !pchan) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.inout(rows, post_rows_bytes(fil, nrows));
  return hs.run(e, "device memory for the rows", "upload rows", "download rows", [&]() {
    return frbch_rfi_cleanf_device(fil, d_rows, nrows, par, fpar, zap, device, mask, repl, chan_flag, blk_flag, pflag, pchan, peaks,
                                   kernel_used, err, err_cap);
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// resident rows: every product cleaned in one residency; flagging, search, grouping and cut-outs in one call
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int frbch_rfi_cleanp_device(const frbch_fil_desc* fil_in, void* d_rows, uint64_t nrows, const frbch_rfi_params* par,
                                       const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag,
                                       uint8_t* blk_flag, void* stats_out, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!fil_in || fil_in->size != sizeof(frbch_fil_desc)) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size");
  frbch_fil_desc fd = *fil_in;
  fd.product = 0;                                          // every product is cleaned
  uint32_t nblk = 0;
  int rc = rfi_check(&fd, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!d_rows || !mask || !repl || !chan_flag || !blk_flag) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const uint32_t nifs = fd.nifs, nchan = fd.nchan;
  const size_t ncell = (size_t)nblk * nchan;
  HostStage hs;                           // (the statistics and the replacements go product by product: copied by hand)
  void* d_stats = nullptr;
  uint32_t used_min = 1;
  try {
    std::vector<uint64_t> own;                                     // (S, Q): uint64 or double, 16 bytes a cell either way
    if (!stats_out) own.resize((size_t)nifs * ncell * 2);
    uint64_t* st = stats_out ? (uint64_t*)stats_out : own.data();
    d_stats = hs.scratch(ncell * 16);
    if (hs.failed) rc = e.fail(FRBCH_E_NOMEM, "device memory for the statistics");
    for (uint32_t p = 0; p < nifs && !rc; ++p) {
      uint32_t used = 0;
      fd.product = p;
      rc = frbch_rfi_stats_device(&fd, d_rows, nrows, par, device, d_stats, &used, err, err_cap);
      if (!rc && (dev_d2h(st + (size_t)p * ncell * 2, d_stats, ncell * 16, 0) != 0 || dev_sync(0) != 0))
        rc = e.fail(FRBCH_E_DEVICE, "download statistics");
      used_min = std::min(used_min, used);
    }
    // every product's own decision, their union, then -- several products -- the decision again with the union as prior
    std::vector<uint8_t> m1(ncell), cf1(nchan), bf1(nblk);
    memset(mask, 0, ncell);
    memset(chan_flag, 0, nchan);
    memset(blk_flag, 0, nblk);
    for (uint32_t p = 0; p < nifs && !rc; ++p) {
      fd.product = p;
      rc = frbch_rfi_mask(&fd, st + (size_t)p * ncell * 2, nblk, nrows, par, zap, nullptr, m1.data(), repl + (size_t)p * nchan,
                          cf1.data(), bf1.data(), err, err_cap);
      for (size_t i = 0; i < ncell; ++i) mask[i] |= m1[i];
      for (uint32_t c = 0; c < nchan; ++c) chan_flag[c] |= cf1[c];
      for (uint32_t b = 0; b < nblk; ++b) blk_flag[b] |= bf1[b];
    }
    for (uint32_t p = 0; p < nifs && nifs > 1 && !rc; ++p) {
      fd.product = p;
      rc = frbch_rfi_mask(&fd, st + (size_t)p * ncell * 2, nblk, nrows, par, zap, mask, m1.data(), repl + (size_t)p * nchan,
                          cf1.data(), bf1.data(), err, err_cap);
    }
  } catch (const std::bad_alloc&) {
    rc = e.fail(FRBCH_E_NOMEM, "host memory for the statistics");
  }
  if (!rc && std::any_of(mask, mask + ncell, [](uint8_t m) { return m != 0; })) {      // (nothing masked: nothing to write)
    uint8_t* d_mask = hs.in(mask, ncell);
    double* d_repl = (double*)hs.scratch(nchan * sizeof(double));
    if (hs.failed) rc = e.fail(FRBCH_E_NOMEM, "device memory for the mask");
    if (!rc && hs.upload() != 0) rc = e.fail(FRBCH_E_DEVICE, "upload mask");
    for (uint32_t p = 0; p < nifs && !rc; ++p) {
      fd.product = p;
      if (dev_h2d(d_repl, repl + (size_t)p * nchan, nchan * sizeof(double), 0) != 0 || dev_sync(0) != 0)
        rc = e.fail(FRBCH_E_DEVICE, "upload replacements");
      if (!rc) rc = frbch_rfi_apply_device(&fd, d_rows, nrows, par, d_mask, d_repl, device, err, err_cap);
    }
  }
  if (!rc && kernel_used) *kernel_used = used_min;
  return rc;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rfi_cleanp_host(const frbch_fil_desc* fil, void* rows, uint64_t nrows, const frbch_rfi_params* par,
                                     const uint8_t* zap, int device, uint8_t* mask, double* repl, uint8_t* chan_flag,
                                     uint8_t* blk_flag, void* stats, uint32_t* kernel_used, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  if (!fil || fil->size != sizeof(frbch_fil_desc)) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size");
  frbch_fil_desc fd = *fil;
  fd.product = 0;
  uint32_t nblk = 0;
  int rc = rfi_check(&fd, nrows, par, &nblk, e);
  if (rc) return rc;
  if (!rows || !mask || !repl || !chan_flag || !blk_flag) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.inout(rows, post_rows_bytes(fil, nrows));
  return hs.run(e, "device memory for the rows", "upload rows", "download rows",
                [&]() { return frbch_rfi_cleanp_device(fil, d_rows, nrows, par, zap, device, mask, repl, chan_flag, blk_flag, stats, kernel_used, err, err_cap); });
}

struct frbch_cand_result {
  uint64_t nout = 0, nclipped = 0, ngroup_all = 0;
  std::vector<frbch_sp_cand> cands;
  std::vector<frbch_sp_group> groups;
  std::vector<frbch_cutout_cand> cut_cands;
  bool planes = false, rfi = false, keep_series = false;
  std::vector<float> ft, dt, series;
  std::vector<uint32_t> ft_hits, dt_hits;
  uint32_t nblk = 0;
  std::vector<uint8_t> mask, chan_flag, blk_flag;
  std::vector<double> repl;
  uint32_t kernel_used[4] = {0, 0, 0, 0}, cutout_calls = 0, row_uploads = 0;
  double wall_ms[FRBCH_CAND_NSTAGE] = {0}, device_ms[FRBCH_CAND_NSTAGE] = {0};
};

namespace {
std::vector<uint64_t> cand_select(const frbch_sp_group* g, uint64_t n, uint32_t min_members, uint32_t max_cands) {
  std::vector<uint64_t> idx;
  for (uint64_t i = 0; i < n; ++i)
    if (g[i].nmember >= min_members) idx.push_back(i);
  if (max_cands > 0 && idx.size() > max_cands) {
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return g[a].best.sigma > g[b].best.sigma; });
    idx.resize(max_cands);
    std::sort(idx.begin(), idx.end());
  }
  return idx;
}

frbch_cutout_cand cand_cutout_of(const frbch_sp_cand& b, const double* dms, double dm_span) {
  POST_NO_CONTRACT
  frbch_cutout_cand c;
  memset(&c, 0, sizeof c);
  c.dm = dms[b.dm_index];
  if (dm_span > 0.0) {
    const double half = 0.5 * dm_span;
    const double lo = c.dm - half;
    c.dm_lo = lo > 0.0 ? lo : 0.0;
    c.dm_hi = c.dm_lo + dm_span;
  } else {
    c.dm_lo = 0.0;
    c.dm_hi = 2.0 * c.dm;
  }
  c.sample = (int64_t)b.sample;
  c.tfactor = std::min<uint32_t>(std::max<uint32_t>(b.width / 2, 1u), 512u);
  return c;
}

// candidates of one frbch_cutout_* call: the three per-call limits
uint64_t cand_per_call(const frbch_fil_desc* fil, const frbch_cutout_params* cut) {
  const uint64_t by_plane = ((1ull << 31) - 1) / ((uint64_t)std::max(cut->nf, cut->ndm) * cut->nt);
  const uint64_t by_table = kCutTableCap / ((uint64_t)cut->ndm * fil->nchan);
  return std::max<uint64_t>(1, std::min<uint64_t>(65535, std::min(by_plane, by_table)));
}

int cand_run(const frbch_fil_desc* fil, const void* rows_h, const void* d_rows_in, uint64_t nrows, const double* dms, uint32_t ndm,
             const frbch_cand_params* par, int device, frbch_cand_result** out, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  if (!out) return e.fail(FRBCH_E_ARG, "null argument: out");
  *out = nullptr;
  if (!par || par->size != sizeof(frbch_cand_params)) return e.fail(FRBCH_E_ARG, "frbch_cand_params: wrong size");
  if (par->flags & ~(FRBCH_CAND_RFI | FRBCH_CAND_SERIES)) return e.fail(FRBCH_E_ARG, "unknown flag");
  int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!(rows_h || d_rows_in) || !dms || !ndm) return e.fail(FRBCH_E_ARG, "null argument");
  uint64_t blk_len = 0;
  rc = sp_check(&par->sp, &blk_len, e);
  if (rc) return rc;
  if (ndm > 65535) return e.fail(FRBCH_E_ARG, "ndm must be 1..65535");
  if (par->min_members < 1) return e.fail(FRBCH_E_ARG, "min_members must be at least 1");
  if (par->dm_gap < 1 || par->dm_gap > 16) return e.fail(FRBCH_E_ARG, "dm_gap must be 1..16");
  const bool rfi = (par->flags & FRBCH_CAND_RFI) != 0, keep_series = (par->flags & FRBCH_CAND_SERIES) != 0, cut = par->cut.nt != 0;
  uint32_t nblk = 0;
  if (rfi && (rc = rfi_check(fil, nrows, &par->rfi, &nblk, e)) != 0) return rc;
  if (cut && (rc = cut_check_par(fil, &par->cut, e)) != 0) return rc;
  const long want = frbch_dedisperse_nout(fil, nrows, dms, ndm);
  if (want <= 0) return e.fail(FRBCH_E_ARG, "a DM outside [0, 1e5), or the largest dispersion delay exceeds the data");
  const uint64_t nout = (uint64_t)want;
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const uint32_t nchan = fil->nchan;
  const size_t in_bytes = post_rows_bytes(fil, nrows);
  const size_t out_bytes = (size_t)ndm * nout * sizeof(float), ncell = (size_t)nblk * nchan;
  const uint64_t per_call = cut ? cand_per_call(fil, &par->cut) : 0;
  // what the call asks of the device, for the message of FRBCH_E_NOMEM
  auto nomem = [&](const char* what) {
    std::string m = std::string("device memory for ") + what + "; the call needs:";
    auto add = [&](const std::string& name, uint64_t bytes) { m += " " + name + " " + std::to_string(bytes) + " B,"; };
    if (rows_h) add("rows", in_bytes);
    if (rfi) {
      if (!rows_h) add("cleaned copy of the rows (when a cell is masked)", in_bytes);
      add("block statistics", ncell * 16);
      add("mask", ncell);
      add("replacement values", nchan * sizeof(double));
    }
    add("series", out_bytes);
    add("search statistics", (uint64_t)ndm * std::max<uint64_t>(1, nout / blk_len) * 2 * sizeof(double));
    add("raw peaks", (uint64_t)kSpRawCap * sizeof(SpPeak));
    if (cut) {
      add("planes of a batch of at most " + std::to_string(per_call) + " candidates, each",
          ((uint64_t)par->cut.nf + par->cut.ndm) * par->cut.nt * 8);
      add("delay tables of a batch, each candidate", ((uint64_t)par->cut.ndm + 1) * nchan * sizeof(int32_t));
    }
    m.back() = '.';
    return e.fail(FRBCH_E_NOMEM, m);
  };
  try {
    std::unique_ptr<frbch_cand_result> res(new frbch_cand_result());
    res->nout = nout;
    res->rfi = rfi;
    res->keep_series = keep_series;
    // everything the call holds on the device: the uploaded rows (`up`, given back first) and what the stages allocate (`cd`)
    void *d_rows = nullptr, *d_work = nullptr, *d_stats = nullptr;
    uint8_t* d_mask = nullptr; double* d_repl = nullptr;
    float *d_series = nullptr, *d_ft = nullptr, *d_dt = nullptr;
    uint32_t *d_fth = nullptr, *d_dth = nullptr;
    PostScope cd(false);                                           // (every stage has a clock of its own)
    if (!cd.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
    HostStage up;
    const auto now = []() { return std::chrono::steady_clock::now(); };
    // fn() as stage k: its wall time, and the device time its _device calls (or a StageClock of its own) report
    auto stage = [&](int k, auto&& fn) -> int {
      const auto t0 = now();
      tl_stage_ms = &res->device_ms[k];
      const int r = fn();
      tl_stage_ms = nullptr;
      res->wall_ms[k] += std::chrono::duration<double, std::milli>(now() - t0).count();
      return r;
    };
    const void* d_use = d_rows_in;
    if (rows_h) {
      d_rows = up.in(rows_h, in_bytes);
      if (up.failed) return nomem("the rows");
      rc = stage(FRBCH_CAND_T_UPLOAD, [&]() {
        StageClock clk(cd.s);
        const bool bad = up.upload(cd.s) != 0;
        clk.finish();
        return bad ? e.fail(FRBCH_E_DEVICE, "upload rows") : FRBCH_OK;
      });
      if (rc) return rc;
      d_use = d_rows;
      res->row_uploads = 1;
    }
    if (rfi) {
      res->nblk = nblk;
      res->mask.assign(ncell, 0);
      res->repl.assign(nchan, 0.0);
      res->chan_flag.assign(nchan, 0);
      res->blk_flag.assign(nblk, 0);
      std::vector<uint64_t> st(ncell * 2);                        // (S, Q): uint64 or double, 16 bytes a cell either way
      if (cd.alloc(&d_stats, ncell * 16) != 0) return nomem("the block statistics");
      rc = stage(FRBCH_CAND_T_FLAG, [&]() {
        int r = frbch_rfi_stats_device(fil, d_use, nrows, &par->rfi, device, d_stats, &res->kernel_used[0], err, err_cap);
        if (!r && (dev_d2h(st.data(), d_stats, ncell * 16, cd.s) != 0 || dev_sync(cd.s) != 0)) r = e.fail(FRBCH_E_DEVICE, "download statistics");
        if (!r) r = frbch_rfi_mask(fil, st.data(), nblk, nrows, &par->rfi, par->zap, nullptr, res->mask.data(), res->repl.data(),
                                   res->chan_flag.data(), res->blk_flag.data(), err, err_cap);
        return r;
      });
      if (rc) return rc;
      cd.drop(d_stats);
      if (std::any_of(res->mask.begin(), res->mask.end(), [](uint8_t m) { return m != 0; })) {   // (nothing masked: nothing to write)
        void* target = d_rows;
        if (!rows_h) {                                            // the caller's rows keep every byte: a copy is cleaned
          if (cd.alloc(&d_work, in_bytes) != 0) return nomem("the cleaned copy of the rows");
          target = d_work;
        }
        if (cd.alloc(&d_mask, ncell) != 0 || cd.alloc(&d_repl, nchan * sizeof(double)) != 0) return nomem("the mask");
        rc = stage(FRBCH_CAND_T_FLAG, [&]() {
          if ((!rows_h && dev_d2d(d_work, d_rows_in, in_bytes, cd.s) != 0) || dev_h2d(d_mask, res->mask.data(), ncell, cd.s) != 0 ||
              dev_h2d(d_repl, res->repl.data(), nchan * sizeof(double), cd.s) != 0 || dev_sync(cd.s) != 0)
            return e.fail(FRBCH_E_DEVICE, "copy rows / upload mask");
          return frbch_rfi_apply_device(fil, target, nrows, &par->rfi, d_mask, d_repl, device, err, err_cap);
        });
        if (rc) return rc;
        d_use = target;
        cd.drop(d_mask);
        cd.drop(d_repl);
      }
    }
    if (cd.alloc(&d_series, out_bytes) != 0) return nomem("the series");
    res->kernel_used[1] = frbch_dedisperse_kernel(fil, d_use, nrows, dms, ndm) > 0 ? 1u : 0u;
    rc = stage(FRBCH_CAND_T_DEDISPERSE, [&]() {
      return frbch_dedisperse_device(fil, d_use, nrows, dms, ndm, par->zerodm, par->clip_sigma, device, d_series, nout, &res->nclipped,
                                     err, err_cap);
    });
    if (rc) return rc;
    if (keep_series) {
      res->series.resize((size_t)ndm * nout);
      rc = stage(FRBCH_CAND_T_DOWNLOAD, [&]() {
        StageClock clk(cd.s);
        const bool bad = dev_d2h(res->series.data(), d_series, out_bytes, cd.s) != 0 || dev_sync(cd.s) != 0;
        clk.finish();
        return bad ? e.fail(FRBCH_E_DEVICE, "download series") : FRBCH_OK;
      });
      if (rc) return rc;
    }
    uint64_t ncand = 0;
    rc = stage(FRBCH_CAND_T_SEARCH, [&]() {
      return sp_search_run(d_series, ndm, nout, &par->sp, device, nullptr, 0, &ncand, &res->kernel_used[2], &res->cands, err, err_cap);
    });
    if (rc) return rc;
    cd.drop(d_series);                                             // the plane is done with; the rows stay for the cut-outs
    std::vector<frbch_sp_group> all(std::max<size_t>(1, res->cands.size()));
    uint64_t ngroup_all = 0;
    rc = frbch_sp_group_cands(fil, dms, ndm, res->cands.data(), res->cands.size(), par->dm_gap, all.data(), all.size(), &ngroup_all,
                              err, err_cap);
    if (rc) return rc;
    res->ngroup_all = ngroup_all;
    for (uint64_t i : cand_select(all.data(), ngroup_all, par->min_members, par->max_cands)) {
      res->groups.push_back(all[i]);
      res->cut_cands.push_back(cand_cutout_of(all[i].best, dms, par->dm_span));
    }
    const uint64_t n = res->groups.size();
    if (cut && n) {
      const uint32_t nt = par->cut.nt, nf = par->cut.nf, cdm = par->cut.ndm;
      const size_t ft1 = (size_t)nf * nt, dt1 = (size_t)cdm * nt;
      res->ft.resize(n * ft1); res->ft_hits.resize(n * ft1);
      res->dt.resize(n * dt1); res->dt_hits.resize(n * dt1);
      res->planes = true;
      const uint64_t bmax = std::min(n, per_call);
      if (cd.alloc(&d_ft, bmax * ft1 * 4) != 0 || cd.alloc(&d_fth, bmax * ft1 * 4) != 0 || cd.alloc(&d_dt, bmax * dt1 * 4) != 0 ||
          cd.alloc(&d_dth, bmax * dt1 * 4) != 0)
        return nomem("the planes");
      uint32_t used_min = 1;
      for (uint64_t a = 0; a < n; a += per_call) {
        const uint32_t cnt = (uint32_t)std::min(per_call, n - a);
        uint32_t used = 0;
        rc = stage(FRBCH_CAND_T_CUT, [&]() {
          return frbch_cutout_device(fil, d_use, nrows, &par->cut, &res->cut_cands[a], cnt, device, d_ft, d_fth, d_dt, d_dth, &used,
                                     err, err_cap);
        });
        if (rc) return rc;
        used_min = std::min(used_min, used);
        ++res->cutout_calls;
        rc = stage(FRBCH_CAND_T_DOWNLOAD, [&]() {
          StageClock clk(cd.s);
          const bool bad = dev_d2h(&res->ft[a * ft1], d_ft, cnt * ft1 * 4, cd.s) != 0 || dev_d2h(&res->ft_hits[a * ft1], d_fth, cnt * ft1 * 4, cd.s) != 0 ||
                           dev_d2h(&res->dt[a * dt1], d_dt, cnt * dt1 * 4, cd.s) != 0 || dev_d2h(&res->dt_hits[a * dt1], d_dth, cnt * dt1 * 4, cd.s) != 0 ||
                           dev_sync(cd.s) != 0;
          clk.finish();
          return bad ? e.fail(FRBCH_E_DEVICE, "download planes") : FRBCH_OK;
        });
        if (rc) return rc;
      }
      res->kernel_used[3] = used_min;
    }
    *out = res.release();
  } catch (const std::bad_alloc&) {
    tl_stage_ms = nullptr;
    return e.fail(FRBCH_E_NOMEM, "host memory for the result");
  }
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_candidates_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                     const frbch_cand_params* par, int device, frbch_cand_result** out, char* err, size_t err_cap) {
  if (out) *out = nullptr;
  if (!rows) return PostErr{err, err_cap}.fail(FRBCH_E_ARG, "null argument");
  return cand_run(fil, rows, nullptr, nrows, dms, ndm, par, device, out, err, err_cap);
}

extern "C" int frbch_candidates_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const double* dms, uint32_t ndm,
                                       const frbch_cand_params* par, int device, frbch_cand_result** out, char* err, size_t err_cap) {
  if (out) *out = nullptr;
  if (!d_rows) return PostErr{err, err_cap}.fail(FRBCH_E_ARG, "null argument");
  return cand_run(fil, nullptr, d_rows, nrows, dms, ndm, par, device, out, err, err_cap);
}

extern "C" int frbch_cand_result_view(const frbch_cand_result* r, frbch_cand_view* v) {
  if (!r || !v || v->size != sizeof(frbch_cand_view)) return FRBCH_E_ARG;
  memset(v, 0, sizeof *v);
  v->size = sizeof *v;
  v->nout = r->nout;
  v->nclipped = r->nclipped;
  v->ncand = r->cands.size();
  v->cands = r->cands.empty() ? nullptr : r->cands.data();
  v->ngroup_all = r->ngroup_all;
  v->ngroup = r->groups.size();
  v->groups = r->groups.empty() ? nullptr : r->groups.data();
  v->cut_cands = r->cut_cands.empty() ? nullptr : r->cut_cands.data();
  if (r->planes) {
    v->ft = r->ft.data(); v->ft_hits = r->ft_hits.data();
    v->dt = r->dt.data(); v->dt_hits = r->dt_hits.data();
  }
  if (r->rfi) {
    v->nblk = r->nblk;
    v->mask = r->mask.data(); v->repl = r->repl.data();
    v->chan_flag = r->chan_flag.data(); v->blk_flag = r->blk_flag.data();
  }
  if (r->keep_series) v->series = r->series.data();
  for (int k = 0; k < 4; ++k) v->kernel_used[k] = r->kernel_used[k];
  v->cutout_calls = r->cutout_calls;
  v->row_uploads = r->row_uploads;
  for (int k = 0; k < FRBCH_CAND_NSTAGE; ++k) { v->wall_ms[k] = r->wall_ms[k]; v->device_ms[k] = r->device_ms[k]; }
  return FRBCH_OK;
}

extern "C" void frbch_cand_result_free(frbch_cand_result* r) { delete r; }

extern "C" int frbch_cand_select(const frbch_sp_group* groups, uint64_t ngroup, uint32_t min_members, uint32_t max_cands,
                                 uint64_t* keep, uint64_t cap, uint64_t* nkeep) {
  if (!nkeep || (ngroup && !groups) || (cap && !keep) || min_members < 1) return FRBCH_E_ARG;
  try {
    const std::vector<uint64_t> idx = cand_select(groups, ngroup, min_members, max_cands);
    *nkeep = idx.size();
    for (uint64_t i = 0; i < std::min<uint64_t>(cap, idx.size()); ++i) keep[i] = idx[i];
    return idx.size() > cap ? FRBCH_E_CAPACITY : FRBCH_OK;
  } catch (const std::bad_alloc&) {
    return FRBCH_E_NOMEM;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// corner turn
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// "[swap_sign_mag+]<W>>[b,b,..][b,b,..]...:<t0>[-<t1>]"   (spif2file.sh:31-113)
int parse_recipe(const char* text, CornerParams* cp, uint32_t* first_tag, const PostErr& e) {
  if (!text) return e.fail(FRBCH_E_ARG, "null recipe");
  std::string s(text);
  memset(cp, 0, sizeof *cp);
  const std::string pre = "swap_sign_mag+";
  if (s.compare(0, pre.size(), pre) == 0) {
    cp->swap_sign_mag = 1;
    s = s.substr(pre.size());
  }
  const size_t gt = s.find('>');
  if (gt == std::string::npos) return e.fail(FRBCH_E_ARG, "recipe: no '>'");
  cp->word_bits = atoi(s.substr(0, gt).c_str());
  if (cp->word_bits != 4 && cp->word_bits != 8 && cp->word_bits != 16 && cp->word_bits != 32 && cp->word_bits != 64)
    return e.fail(FRBCH_E_ARG, "recipe: word width must be 4, 8, 16, 32 or 64 bits");
  size_t pos = gt + 1;
  int ng = 0, glen = -1;
  while (pos < s.size() && s[pos] == '[') {
    const size_t close = s.find(']', pos);
    if (close == std::string::npos || ng >= 16) return e.fail(FRBCH_E_ARG, "recipe: bad bracket list (at most 16 groups)");
    std::stringstream ls(s.substr(pos + 1, close - pos - 1));
    std::string item;
    int k = 0;
    while (std::getline(ls, item, ',')) {
      const int b = atoi(item.c_str());
      if (b < 0 || b >= cp->word_bits || k >= 8) return e.fail(FRBCH_E_ARG, "recipe: bit index outside the word, or more than 8 bits in a group");
      cp->src[ng][k++] = (uint8_t)b;
    }
    if (glen < 0) glen = k;
    if (k != glen || (k != 1 && k != 2 && k != 4 && k != 8)) return e.fail(FRBCH_E_ARG, "recipe: every group must take the same 1, 2, 4 or 8 bits");
    ++ng;
    pos = close + 1;
  }
  if (!ng) return e.fail(FRBCH_E_ARG, "recipe: no groups");
  cp->ngroup = ng;
  cp->glen = glen;
  int t0 = 0, t1 = ng - 1;
  if (pos < s.size() && s[pos] == ':') {
    const std::string tags = s.substr(pos + 1);
    const size_t dash = tags.find('-');
    t0 = atoi(tags.substr(0, dash).c_str());
    t1 = dash == std::string::npos ? t0 : atoi(tags.substr(dash + 1).c_str());
  }
  if (t1 - t0 + 1 != ng) return e.fail(FRBCH_E_ARG, "recipe: tag range does not match the number of groups");
  if (first_tag) *first_tag = (uint32_t)t0;
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_cornerturn_info(const char* recipe, uint32_t* word_bits, uint32_t* ntags, uint32_t* bits_per_word,
                                     uint32_t* first_tag, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  CornerParams cp;
  const int rc = parse_recipe(recipe, &cp, first_tag, e);
  if (rc) return rc;
  if (word_bits) *word_bits = (uint32_t)cp.word_bits;
  if (ntags) *ntags = (uint32_t)cp.ngroup;
  if (bits_per_word) *bits_per_word = (uint32_t)cp.glen;
  return FRBCH_OK;
}

extern "C" int frbch_cornerturn_device(const char* recipe, const void* d_frames, size_t nframes, uint32_t frame_bytes,
                                       uint32_t header_bytes, void* const* d_out, uint32_t ntags, size_t out_bytes_each,
                                       int device, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  CornerParams cp;
  int rc = parse_recipe(recipe, &cp, nullptr, e);
  if (rc) return rc;
  if (!d_frames || !d_out || frame_bytes <= header_bytes) return e.fail(FRBCH_E_ARG, "null argument or bad frame geometry");
  if (ntags != (uint32_t)cp.ngroup) return e.fail(FRBCH_E_ARG, "ntags differs from the recipe's groups");
  const uint64_t pay = (uint64_t)nframes * (frame_bytes - header_bytes);
  if ((frame_bytes - header_bytes) * 8ull % (uint64_t)cp.word_bits) return e.fail(FRBCH_E_ARG, "payload is not a whole number of words");
  const uint64_t nwords = pay * 8 / (uint64_t)cp.word_bits;
  const uint64_t wpt = 64 / (uint64_t)cp.glen;
  if ((nwords * cp.glen) % 8) return e.fail(FRBCH_E_ARG, "the frames must hold a whole number of output bytes per stream");
  if (out_bytes_each != nwords * cp.glen / 8) return e.fail(FRBCH_E_CAPACITY, "out_bytes_each must be words * bits per word / 8");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  cp.frames = (const uint8_t*)d_frames;
  cp.frame_bytes = frame_bytes;
  cp.header_bytes = header_bytes;
  cp.payload_bytes = frame_bytes - header_bytes;
  cp.nwords = nwords;
  for (uint32_t g = 0; g < ntags; ++g) {
    if (!d_out[g]) return e.fail(FRBCH_E_ARG, "null output stream");
    cp.out[g] = (uint8_t*)d_out[g];
  }
  if (nwords) {
    DEV_LAUNCH(frbch_post_cornerturn, ((nwords + wpt - 1) / wpt + 255) / 256, 1, 256, 0, (dev_stream_t)0, cp);
    if (dev_check_launch() != 0 || dev_sync(0) != 0) return e.fail(FRBCH_E_DEVICE, std::string("corner turn: ") + dev_last_error_string());
  }
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_cornerturn_host(const char* recipe, const void* frames, size_t nframes, uint32_t frame_bytes,
                                     uint32_t header_bytes, void* const* out, uint32_t ntags, size_t out_bytes_each,
                                     int device, char* err, size_t err_cap) {
  PostErr e{err, err_cap};
  if (!frames || !out || ntags > 16) return e.fail(FRBCH_E_ARG, "null argument");
  if (int rc = post_check_device(device, e)) return rc;
  DeviceGuard dg(device);
  void* d_o[16] = {nullptr};
  HostStage hs;
  void* d_in = hs.in(frames, nframes * (size_t)frame_bytes);
  for (uint32_t g = 0; g < ntags; ++g) d_o[g] = hs.scratch(out_bytes_each);       // (downloaded stream by stream, below)
  if (hs.failed) return e.fail(FRBCH_E_NOMEM, "device memory");
  if (hs.upload() != 0) return e.fail(FRBCH_E_DEVICE, "upload frames");
  int rc = frbch_cornerturn_device(recipe, d_in, nframes, frame_bytes, header_bytes, d_o, ntags, out_bytes_each, device, err, err_cap);
  for (uint32_t g = 0; g < ntags && !rc; ++g)
    if (dev_d2h(out[g], d_o[g], out_bytes_each, 0) != 0) rc = e.fail(FRBCH_E_DEVICE, "download streams");
  if (!rc && dev_sync(0) != 0) rc = e.fail(FRBCH_E_DEVICE, "sync");
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------------
// burst polarisation: spectra of every product, RM synthesis, peaks (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kBurstMaxCand = 4096, kBurstMaxWidth = 65536, kBurstMaxOff = 1u << 20;
constexpr uint32_t kRmMaxPhi = 1u << 20, kRmMaxChan = 16384, kRmTableN = 16384;
constexpr uint64_t kRmMaxOut = 1ull << 26;
constexpr double kRmPhiMax = 1.0e7, kRmC = 299.792458, kRmPi = 3.14159265358979323846;

int burst_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_burst_params* par, const frbch_burst_cand* cands,
                uint32_t ncand, const PostErr& e) {
  const int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (!par || par->size != sizeof(frbch_burst_params)) return e.fail(FRBCH_E_ARG, "frbch_burst_params: wrong size");
  if (par->products > FRBCH_BURST_COHERENCY) return e.fail(FRBCH_E_ARG, "products must be 0 (Stokes) or 1 (coherency)");
  if (par->products == FRBCH_BURST_COHERENCY && fil->nifs != 4) return e.fail(FRBCH_E_ARG, "coherency products need nifs = 4");
  if (!cands || ncand < 1 || ncand > kBurstMaxCand) return e.fail(FRBCH_E_ARG, "1..4096 candidates");
  if ((uint64_t)ncand * fil->nchan > kCutTableCap) return e.fail(FRBCH_E_ARG, "ncand * nchan exceeds 2^26: cut the batch into several calls");
  if ((uint64_t)ncand * fil->nifs > 65535) return e.fail(FRBCH_E_ARG, "ncand * nifs exceeds 65535 (the second grid dimension): cut the batch");
  if (nrows >= (1ull << 62) || (uint64_t)fil->nchan > 0x7FFFFFFFull / fil->nifs) return e.fail(FRBCH_E_ARG, "too many rows or channels");
  for (uint32_t i = 0; i < ncand; ++i) {
    const frbch_burst_cand& c = cands[i];
    const std::string who = "candidate " + std::to_string(i) + ": ";
    if (c.width < 1 || c.width > kBurstMaxWidth) return e.fail(FRBCH_E_ARG, who + "width must be 1..65536");
    if (c.off_len < 2 || c.off_len > kBurstMaxOff) return e.fail(FRBCH_E_ARG, who + "off_len must be 2..2^20");
    if (!(c.dm >= 0.0) || !(c.dm < 1.0e5)) return e.fail(FRBCH_E_ARG, who + "a DM outside [0, 1e5)");
    if (c.sample < -(1ll << 62) || c.sample > (1ll << 62)) return e.fail(FRBCH_E_ARG, who + "sample out of range");
  }
  return FRBCH_OK;
}

// The checks that every windowed analysis of the family (profile, DM scan, burst ACF, scattering fit) makes on its rows and
// its grid, in the family's one order: the float32 refusal, the size of the parameter block `P` (named `pname`), nbin, tfactor,
// nchan and -- own.ffactor given -- ffactor.  An analysis's own refusals that stand between these keep their place: own.pre in
// front of nbin, own.mid in front of nchan, each a function that returns its message or NULL (a NULL function: none).  The
// first failing check decides the message.
constexpr uint32_t kWinMaxBin = 1024, kWinMaxT = 512;
template <class P> struct WindowOwn {
  const char* (*pre)(const P&);
  const char* (*mid)(const P&);
  const uint32_t P::*ffactor;
};
template <class P>
int window_check(const frbch_fil_desc* fil, const P* par, const char* what, const char* pname, const WindowOwn<P>& own, const PostErr& e) {
  const char* msg;
  if (fil->nbits == 32) return e.fail(FRBCH_E_ARG, std::string(what) + " is not built for float32 rows: its fixed-point scale needs a bound on the samples");
  if (!par || par->size != sizeof(P)) return e.fail(FRBCH_E_ARG, std::string(pname) + ": wrong size");
  if (own.pre && (msg = own.pre(*par)) != nullptr) return e.fail(FRBCH_E_ARG, msg);
  if (par->nbin < 1 || par->nbin > kWinMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 1..1024");
  if (par->tfactor < 1 || par->tfactor > kWinMaxT) return e.fail(FRBCH_E_ARG, "tfactor must be 1..512");
  if (own.mid && (msg = own.mid(*par)) != nullptr) return e.fail(FRBCH_E_ARG, msg);
  if (fil->nchan > kRmMaxChan) return e.fail(FRBCH_E_ARG, "more than 16384 channels");
  if (own.ffactor && (par->*own.ffactor < 1 || par->*own.ffactor > fil->nchan || fil->nchan % (par->*own.ffactor))) return e.fail(FRBCH_E_ARG, "ffactor must be 1..nchan and divide nchan");
  return FRBCH_OK;
}

// A _device entry point of the family from where its arguments have passed: the device check, the device made current, a
// scope, then run(scope) -- the scope and what it holds are gone when this returns.
template <class F> int burst_device_call(int device, const PostErr& e, F run) {
  const int rc = post_check_device(device, e);
  if (rc) return rc;
  DeviceGuard dg(device);
  PostScope ps;
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  return run(ps);
}

// The _host twin of a composite from where its arguments have passed: rows up, device_twin(d_rows), nothing else (the
// outputs of a composite are host arrays already).
template <class F> int burst_host_twin(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, int device, const PostErr& e, F device_twin) {
  const int rc = post_check_device(device, e);
  if (rc) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  return hs.run(e, "device memory for the rows", "upload rows", "download", [&]() { return device_twin(d_rows); });
}

// an optional output of an entry point: the caller's array gets the vector (or the kernel_used words), a NULL gets nothing
template <class T, class V> void deliver(T* dst, const std::vector<V>& v) {
  static_assert(sizeof(T) == sizeof(V), "deliver: the element sizes differ");
  if (dst) memcpy((void*)dst, v.data(), v.size() * sizeof(V));
}
template <size_t N> void deliver(uint32_t* dst, const uint32_t (&k)[N]) {
  if (dst) memcpy(dst, k, sizeof k);
}

struct BurstPlan {
  std::vector<BurstCand> cand;
  std::vector<int32_t> delays;                   // [ncand][nchan]
};

int burst_build(const frbch_fil_desc* fil, const frbch_burst_cand* cands, uint32_t ncand, BurstPlan* plan, const PostErr& e) {
  std::vector<double> dms(ncand);
  plan->cand.resize(ncand);
  for (uint32_t i = 0; i < ncand; ++i) {
    dms[i] = cands[i].dm;
    BurstCand& b = plan->cand[i];
    b.on_lo = (long long)cands[i].sample - (long long)(cands[i].width / 2);
    b.width = cands[i].width; b.off_gap = cands[i].off_gap; b.off_len = cands[i].off_len; b.pad = 0;
  }
  int64_t maxd = 0;
  plan->delays = post_delays(fil, dms.data(), ncand, &maxd);      // n_c(.) of frbch_dedisperse_*: the same function
  if (maxd > (int64_t)1 << 30) return e.fail(FRBCH_E_ARG, "a dispersion delay of more than 2^30 samples");
  return FRBCH_OK;
}

// Which burst-sums kernel a call takes -- the one decision behind frbch_burstspec_device's launch, *kernel_used and
// frbch_burstspec_kernel's answer.  true = the fast kernel (kernels_post_fast.inc): 8- / 16-bit rows, at most 4 products,
// whole 64-byte channel tiles, 16-byte pieces of every row (only the ADDRESS of d_rows is examined).  The emulator build
// has no such kernel: false.
bool burst_fast_layout(const frbch_fil_desc* fil, const void* d_rows) {
#ifndef FRBCH_NO_FAST
  if (fil->nbits != 8 && fil->nbits != 16) return false;
  const size_t piece = (size_t)fil->nchan * (size_t)(fil->nbits / 8);
  return fil->nifs <= (uint32_t)fast::kBsMaxIfs && piece % 64 == 0 && ((uintptr_t)d_rows % 16) == 0 && ((size_t)fil->nifs * piece) % 16 == 0;
#else
  (void)fil; (void)d_rows;
  return false;
#endif
}

#ifndef FRBCH_NO_FAST
// The smallest and largest delay of every 64-byte channel tile of a delay table [record][nchan] -> lo, hi [record][tile]: what
// the fast profile, DM scan and dynamic spectrum kernels size their stage by (a record: a candidate, or a trial of one).
struct TileScan {
  uint32_t ntile = 0;
  std::vector<int32_t> lo, hi;
  // The bins of a run that a stage of `cap` rows holds behind the widest delay range that any tile spans over `trun`
  // consecutive records of a candidate's `nt` -- the same for every workgroup; 0: not even one bin of tfactor rows fits.
  int brun(uint32_t ncand, uint32_t nt, uint32_t trun, int64_t cap, uint32_t nbin, uint32_t tfactor) const {
    int64_t range = 0;
    for (uint32_t i = 0; i < ncand; ++i)
      for (uint32_t k0 = 0; k0 < nt; k0 += trun)
        for (uint32_t t = 0; t < ntile; ++t) {
          int32_t a = INT32_MAX, b = INT32_MIN;
          for (uint32_t k = k0; k < std::min(nt, k0 + trun); ++k) {
            a = std::min(a, lo[((size_t)i * nt + k) * ntile + t]);
            b = std::max(b, hi[((size_t)i * nt + k) * ntile + t]);
          }
          range = std::max<int64_t>(range, (int64_t)b - (int64_t)a);
        }
    if ((int64_t)tfactor + range > cap) return 0;
    return (int)std::min<int64_t>((int64_t)nbin, (cap - range) / (int64_t)tfactor);
  }
};
TileScan tile_scan(const frbch_fil_desc* fil, const std::vector<int32_t>& delays) {
  TileScan ts;
  const uint32_t ct = 64u / (uint32_t)(fil->nbits / 8);
  const size_t nrec = delays.size() / fil->nchan;
  ts.ntile = fil->nchan / ct;
  ts.lo.resize(nrec * ts.ntile);
  ts.hi.resize(nrec * ts.ntile);
  for (size_t r = 0; r < nrec; ++r)
    for (uint32_t t = 0; t < ts.ntile; ++t) {
      const int32_t* d = delays.data() + r * fil->nchan + (size_t)t * ct;
      const auto mm = std::minmax_element(d, d + ct);
      ts.lo[r * ts.ntile + t] = *mm.first;
      ts.hi[r * ts.ntile + t] = *mm.second;
    }
  return ts;
}
#endif

// the launch of step 1 on the scope's stream; `plan` stays alive until the caller has synchronised
int burst_launch(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const BurstPlan& plan, uint32_t ncand,
                 BurstSums* d_sums, bool fastk, PostScope& ps, const PostErr& e) {
  BurstCand* d_cand = nullptr;
  int32_t* d_dly = nullptr;
  POST_DEV(ps.alloc(&d_cand, plan.cand.size() * sizeof(BurstCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dly, plan.delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_cand, plan.cand.data(), plan.cand.size() * sizeof(BurstCand), ps.s), "upload candidates");
  POST_DEV(dev_h2d(d_dly, plan.delays.data(), plan.delays.size() * sizeof(int32_t), ps.s), "upload delays");
  BurstParams p = post_params<BurstParams>(fil, d_rows, nrows);
  p.ncand = (int)ncand;
  p.cand = d_cand;
  p.delays = d_dly;
  p.sums = d_sums;
#ifndef FRBCH_NO_FAST
  if (fastk) {
    const int bpv = fil->nbits / 8;
    const dim3 grid((unsigned)((size_t)fil->nchan * bpv / 64), ncand), block(fast::kBsThreads);
    if (bpv == 1) hipLaunchKernelGGL(fast::frbch_post_burst_sums_fast<1>, grid, block, 0, ps.s, p);
    else hipLaunchKernelGGL(fast::frbch_post_burst_sums_fast<2>, grid, block, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch burst sums");
    return FRBCH_OK;
  }
#else
  (void)fastk;
#endif
  DEV_LAUNCH(frbch_post_burst_sums, (fil->nchan + 255) / 256, (uint64_t)ncand * fil->nifs, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch burst sums");
  return FRBCH_OK;
}

bool rm_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
bool rm_finitef(float x) { return fabsf(x) <= 3.402823466e38f; }

// mean and variance of the off-pulse window of one (candidate, product, channel), off_hits >= 2 (host, double, no FMA): the
// one statement of the operation order that the oracles restate bit for bit
struct OffStat { double mean, var; };
inline OffStat burst_off_stat(const frbch_burst_sums& s) {
  POST_NO_CONTRACT
  const double noff = (double)s.off_hits;
  const double ss = s.off_sum * s.off_sum;
  const double sn = ss / noff;
  const double num = s.off_sumsq - sn;
  double var = num / (noff - 1.0);
  if (var < 0.0) var = 0.0;
  return OffStat{s.off_sum / noff, var};
}

// spectra, noise and `used` from the sums (host, double, no FMA): step 1 of the header
void burst_derive(const frbch_fil_desc* fil, uint32_t products, const frbch_burst_sums* sums, uint32_t ncand, const float* gain,
                  float* spec, float* noise, uint8_t* used) {
  POST_NO_CONTRACT
  const size_t nchan = fil->nchan, nifs = fil->nifs;
  for (uint32_t i = 0; i < ncand; ++i)
    for (size_t c = 0; c < nchan; ++c) {
      bool ok = true;
      for (size_t pr = 0; pr < nifs; ++pr) {
        const size_t o = ((size_t)i * nifs + pr) * nchan + c;
        const frbch_burst_sums& s = sums[o];
        float sp = 0.f, nz = 0.f;
        if (s.on_hits == 0 || s.off_hits < 2) {
          ok = false;
        } else {
          const double g = gain ? (double)gain[pr * nchan + c] : 1.0;
          const double non = (double)s.on_hits;
          const OffStat off = burst_off_stat(s);
          const double mon = s.on_sum / non;
          const double d = mon - off.mean;
          sp = (float)(d * g);
          const double vn = off.var / non;
          nz = (float)(sqrt(vn) * fabs(g));
          if (!rm_finitef(sp) || !rm_finitef(nz)) ok = false;
        }
        spec[o] = sp;
        noise[o] = nz;
      }
      if (ok && products == FRBCH_BURST_COHERENCY) {
        float* s0 = spec + (size_t)i * 4 * nchan + c;
        float* n0 = noise + (size_t)i * 4 * nchan + c;
        const float pp = s0[0], qq = s0[nchan], re = s0[2 * nchan], im = s0[3 * nchan];
        const double npp = (double)n0[0], nqq = (double)n0[nchan];
        const double a = npp * npp, b = nqq * nqq;
        const float nq = (float)sqrt(a + b);
        s0[0] = pp + qq; s0[nchan] = 2.0f * re; s0[2 * nchan] = 2.0f * im; s0[3 * nchan] = pp - qq;
        n0[nchan] = 2.0f * n0[2 * nchan];             // noise_Q = 2 nRe (before nRe's slot takes noise_U)
        n0[2 * nchan] = 2.0f * n0[3 * nchan];         // noise_U = 2 nIm
        n0[0] = nq; n0[3 * nchan] = nq;
        for (size_t pr = 0; pr < 4; ++pr)
          if (!rm_finitef(s0[pr * nchan]) || !rm_finitef(n0[pr * nchan])) ok = false;
      }
      if (!ok)
        for (size_t pr = 0; pr < nifs; ++pr) spec[((size_t)i * nifs + pr) * nchan + c] = noise[((size_t)i * nifs + pr) * nchan + c] = 0.f;
      used[(size_t)i * nchan + c] = ok ? 1 : 0;
    }
}

void rm_table_fill(int32_t* C) {
  POST_NO_CONTRACT
  for (int j = 0; j < 4096; ++j) {
    const double x = (2.0 * kRmPi * (double)j) / 16384.0;
    C[j] = (int32_t)rint(cos(x) * 4194304.0);
  }
  C[4096] = 0;
  for (int j = 4097; j <= 8192; ++j) C[j] = -C[8192 - j];
  for (int j = 8193; j < 16384; ++j) C[j] = C[16384 - j];
}

// ---- RM synthesis and the delay x RM transform: one family (include/frbch.h states the arithmetic of both) ----------------
// The second is the first with a tau axis in front of phi: a fifth field in the record, a tau tile in the plan, a plane where
// the first has a row.  The grid record names the member; everything below is written once for both and reads the delay axis
// from it.  ntau = 1, tau_lo = 0 of the delay family gives RM synthesis to the bit (through its own kernels and records).
constexpr uint32_t kRmdMaxTau = 4096;
constexpr double kRmdTauLim = 100.0;

template <class Par> struct RmFam;
template <> struct RmFam<frbch_rm_params> {
  using Rec = RmRec;
  using KPar = RmParams;
  using Res = frbch_rm_result;
  static constexpr bool delay = false;
  static constexpr const char *wrong_size = "frbch_rm_params: wrong size", *launch = "launch RM synthesis", *join = "launch RM join";
  static uint32_t ntau(const frbch_rm_params*) { return 1; }
};
template <> struct RmFam<frbch_rmd_params> {
  using Rec = RmdRec;
  using KPar = RmdParams;
  using Res = frbch_rmd_result;
  static constexpr bool delay = true;
  static constexpr const char *wrong_size = "frbch_rmd_params: wrong size", *launch = "launch delay x RM transform", *join = "launch delay x RM join";
  static uint32_t ntau(const frbch_rmd_params* par) { return par->ntau; }
};

// the grid checks; the delay family refuses a record of the wrong size before it looks at the file, RM synthesis after
template <class Par> int rm_check(const frbch_fil_desc* fil, uint32_t ncand, const Par* par, const PostErr& e) {
  POST_NO_CONTRACT
  using Fam = RmFam<Par>;
  const bool sized = par && par->size == sizeof(Par);
  if (Fam::delay && !sized) return e.fail(FRBCH_E_ARG, Fam::wrong_size);
  const int rc = post_check_fil(fil, 1, e);
  if (rc) return rc;
  if (fil->nchan > kRmMaxChan) return e.fail(FRBCH_E_ARG, "more than 16384 channels");
  if (!(fil->fch1_mhz + (double)(fil->nchan - 1) * fil->foff_mhz > 0)) return e.fail(FRBCH_E_ARG, "a channel frequency that is not positive");
  if (ncand < 1 || ncand > kBurstMaxCand) return e.fail(FRBCH_E_ARG, "1..4096 candidates");
  if (!sized) return e.fail(FRBCH_E_ARG, Fam::wrong_size);
  if (par->nphi < 1 || par->nphi > kRmMaxPhi) return e.fail(FRBCH_E_ARG, "nphi must be 1..2^20");
  if ((uint64_t)ncand * par->nphi > kRmMaxOut) return e.fail(FRBCH_E_ARG, "ncand * nphi exceeds 2^26");
  if (!(par->dphi > 0) || !rm_finite(par->dphi)) return e.fail(FRBCH_E_ARG, "dphi must be positive and finite");
  const double hi = par->phi_lo + (double)par->nphi * par->dphi;
  if (!(fabs(par->phi_lo) <= kRmPhiMax) || !(fabs(hi) <= kRmPhiMax)) return e.fail(FRBCH_E_ARG, "|phi| above 1e7 rad m^-2");
  if constexpr (Fam::delay) {
    if (par->ntau < 1 || par->ntau > kRmdMaxTau) return e.fail(FRBCH_E_ARG, "ntau must be 1..4096");
    if ((uint64_t)ncand * par->nphi * par->ntau > kRmMaxOut) return e.fail(FRBCH_E_ARG, "ncand * ntau * nphi exceeds 2^26");
    if (!(par->dtau > 0) || !rm_finite(par->dtau)) return e.fail(FRBCH_E_ARG, "dtau must be positive and finite");
    const double thi = par->tau_lo + (double)par->ntau * par->dtau;
    if (!(fabs(par->tau_lo) <= kRmdTauLim) || !(fabs(thi) <= kRmdTauLim)) return e.fail(FRBCH_E_ARG, "|tau| above 100 microseconds");
  }
  return FRBCH_OK;
}

// The plan rule of the family -- the one decision behind the launches of frbch_rmsynth_device and frbch_rmdelay_device, their
// kernel_used, and the answers of frbch_rmsynth_kernel and frbch_rmdelay_kernel; RM synthesis is ntau = 1.  The fast kernel
// wants whole waves along k (nphi >= 64) and stores a trial as one 8-byte piece (only the ADDRESS of d_F is examined).  The
// tau tile is the largest of 8, 4, 2, 1 whose tail -- trials beyond ntau that the last tile computes in vain -- is at most an
// eighth of ntau: the registers hold 8 (kernels_post_fast.inc), and a term saved by sharing a record is worth far less than
// a term wasted; at ntau = 1 it is 1.  A candidate's channels are split until (ncand x tau tiles x k tiles x split) reaches
// two workgroups per CU, in pieces of at least 64 channels, so that the 64 KiB table a workgroup loads serves at least 65536
// terms.  The emulator build has no such kernel: generic, split 1.
struct RmPlanRule { bool fastk; int nsplit, chunk, ttile; };
RmPlanRule rm_plan_rule(uint32_t nchan, uint32_t ncand, uint32_t nphi, uint32_t ntau, const float* d_F) {
  RmPlanRule r{false, 1, (int)nchan, 1};
#ifndef FRBCH_NO_FAST
  if (nphi < 64 || ((uintptr_t)d_F % 8) != 0) return r;
  r.fastk = true;
  for (uint32_t t = fast::kRmdTauMax; t > 1; t /= 2)
    if ((((ntau + t - 1) / t) * t - ntau) * 8 <= ntau) { r.ttile = (int)t; break; }
  const uint64_t ttiles = (ntau + (uint32_t)r.ttile - 1) / (uint32_t)r.ttile;
  const uint64_t base = (uint64_t)ncand * ttiles * ((nphi + fast::kRmThreads * fast::kRmKpt - 1) / (fast::kRmThreads * fast::kRmKpt));
  if (base < 512) {
    const uint64_t want = (512 + base - 1) / base, most = (nchan + 63) / 64;
    const uint32_t ns = (uint32_t)std::min(want, most);
    r.chunk = (int)((nchan + ns - 1) / ns);
    r.nsplit = (int)((nchan + (uint32_t)r.chunk - 1) / (uint32_t)r.chunk);
  }
#else
  (void)ncand; (void)nphi; (void)ntau; (void)d_F;
#endif
  return r;
}

template <class Rec> struct RmPlan {
  std::vector<Rec> rec;                          // [ncand][nchan]
  std::vector<RmCand> cand;
  std::vector<int32_t> table;
};

// x 2^64 of the fractional part of x, as the header states it
uint64_t rm_fix(double x) {
  POST_NO_CONTRACT
  const double fr = x - floor(x);
  const double v = fr * 18446744073709551616.0;
  if (!(v < 18446744073709551616.0)) return 0;
  return (uint64_t)v;
}

std::vector<double> rm_l2(const frbch_fil_desc* fil) {
  POST_NO_CONTRACT
  std::vector<double> l2(fil->nchan);
  for (uint32_t c = 0; c < fil->nchan; ++c) {
    const double f = fil->fch1_mhz + (double)c * fil->foff_mhz;
    const double t = kRmC / f;
    l2[c] = t * t;
  }
  return l2;
}

// the records of step 2 (host), written once: l2, l0, the fixed-point phases, the quantised spectra, inv; the delay family
// adds f0, b, T0 (into p0) and E of the same channels
template <class Par>
int rm_build(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand, const Par* par,
             RmPlan<typename RmFam<Par>::Rec>* plan, const PostErr& e) {
  POST_NO_CONTRACT
  using Rec = typename RmFam<Par>::Rec;
  const uint32_t nchan = fil->nchan;
  const std::vector<double> l2 = rm_l2(fil);
  plan->rec.assign((size_t)ncand * nchan, Rec{});
  plan->cand.assign(ncand, RmCand{0u, 0u, 0.0});
  plan->table.resize(kRmTableN);
  rm_table_fill(plan->table.data());
  for (uint32_t i = 0; i < ncand; ++i) {
    const float* qi = q + (size_t)i * nchan;
    const float* ui = u + (size_t)i * nchan;
    const uint8_t* us = used + (size_t)i * nchan;
    uint32_t N = 0;
    double sum = 0.0, fsum = 0.0;
    float m = 0.f;
    for (uint32_t c = 0; c < nchan; ++c)
      if (us[c]) {
        if (!rm_finitef(qi[c]) || !rm_finitef(ui[c]))
          return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": q or u of a used channel is not finite");
        ++N;
        sum = sum + l2[c];
        const double f = fil->fch1_mhz + (double)c * fil->foff_mhz;
        fsum = fsum + f;
        m = std::max(m, std::max(fabsf(qi[c]), fabsf(ui[c])));
      }
    if (N == 0 || m == 0.f) continue;              // F = 0: no records, inv = 0
    const double l0 = sum / (double)N, f0 = fsum / (double)N;
    int ex = 0;
    (void)frexp((double)m, &ex);
    Rec* rec = plan->rec.data() + (size_t)i * nchan;
    uint32_t n = 0;
    for (uint32_t c = 0; c < nchan; ++c)
      if (us[c]) {
        const double a = (l2[c] - l0) / kRmPi;
        Rec& r = rec[n++];
        r.qi = (int32_t)rint(ldexp((double)qi[c], 23 - ex));
        r.ui = (int32_t)rint(ldexp((double)ui[c], 23 - ex));
        r.p0 = rm_fix(par->phi_lo * a);
        r.d = rm_fix(par->dphi * a);
        if constexpr (RmFam<Par>::delay) {
          const double f = fil->fch1_mhz + (double)c * fil->foff_mhz;
          const double b = f - f0;
          r.p0 = r.p0 + rm_fix(par->tau_lo * b);
          r.e = rm_fix(par->dtau * b);
        }
      }
    plan->cand[i].nrec = n;
    plan->cand[i].inv = 1.0 / ldexp((double)N, 45 - ex);
  }
  return FRBCH_OK;
}

#ifndef FRBCH_NO_FAST
// the fast kernel of each member on the grid the plan rule gives
int rm_launch_fast(const RmPlanRule&, dim3 grid, dev_stream_t s, const RmParams& p) {
  return launch_lds(fast::frbch_post_rm_fast, grid, dim3(fast::kRmThreads), fast::kRmLds, s, p);
}
int rm_launch_fast(const RmPlanRule& rule, dim3 grid, dev_stream_t s, const RmdParams& p) {
  const dim3 block(fast::kRmThreads);
  switch (rule.ttile) {
    case 8: return launch_lds(fast::frbch_post_rmd_fast<8>, grid, block, fast::kRmdLds, s, p);
    case 4: return launch_lds(fast::frbch_post_rmd_fast<4>, grid, block, fast::kRmdLds, s, p);
    case 2: return launch_lds(fast::frbch_post_rmd_fast<2>, grid, block, fast::kRmdLds, s, p);
    default: return launch_lds(fast::frbch_post_rmd_fast<1>, grid, block, fast::kRmdLds, s, p);
  }
}
#endif

// the launches of step 2 on the scope's stream; `plan` stays alive until the caller has synchronised
template <class Par>
int rm_launch(const frbch_fil_desc* fil, uint32_t ncand, const Par* par, const RmPlan<typename RmFam<Par>::Rec>& plan, float* d_F,
              PostScope& ps, uint32_t* kernel_used, const PostErr& e) {
  using Fam = RmFam<Par>;
  using Rec = typename Fam::Rec;
  const uint32_t ntau = Fam::ntau(par);
  const RmPlanRule rule = rm_plan_rule(fil->nchan, ncand, par->nphi, ntau, d_F);
  Rec* d_rec = nullptr;
  RmCand* d_cand = nullptr;
  int32_t* d_tab = nullptr;
  POST_DEV(ps.alloc(&d_rec, plan.rec.size() * sizeof(Rec)), "hipMalloc");
  POST_DEV(ps.alloc(&d_cand, plan.cand.size() * sizeof(RmCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_tab, (size_t)kRmTableN * sizeof(int32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_rec, plan.rec.data(), plan.rec.size() * sizeof(Rec), ps.s), "upload records");
  POST_DEV(dev_h2d(d_cand, plan.cand.data(), plan.cand.size() * sizeof(RmCand), ps.s), "upload records");
  POST_DEV(dev_h2d(d_tab, plan.table.data(), (size_t)kRmTableN * sizeof(int32_t), ps.s), "upload table");
  typename Fam::KPar p;
  memset(&p, 0, sizeof p);
  p.rec = d_rec; p.cand = d_cand; p.table = d_tab; p.out = d_F;
  p.nchan = (int)fil->nchan; p.nphi = (int)par->nphi; p.ncand = (int)ncand; p.nsplit = rule.nsplit; p.chunk = rule.chunk;
  if constexpr (Fam::delay) p.ntau = (int)ntau;
  if (kernel_used) { kernel_used[0] = rule.fastk ? 1 : 0; kernel_used[1] = (uint32_t)rule.nsplit; }
  const size_t per = (size_t)ntau * par->nphi;
#ifndef FRBCH_NO_FAST
  if (rule.fastk) {
    if (rule.nsplit > 1) {
      long long* d_part = nullptr;
      POST_DEV(ps.alloc(&d_part, (size_t)rule.nsplit * ncand * per * 2 * sizeof(long long)), "hipMalloc");
      p.part = d_part;
    }
    const unsigned ktiles = (par->nphi + fast::kRmThreads * fast::kRmKpt - 1) / (fast::kRmThreads * fast::kRmKpt);
    const unsigned ttiles = (ntau + (unsigned)rule.ttile - 1) / (unsigned)rule.ttile;
    POST_DEV(rm_launch_fast(rule, dim3(ktiles, ttiles * (unsigned)rule.nsplit, ncand), ps.s, p), "LDS size");
    POST_DEV(dev_check_launch(), Fam::launch);
    if (rule.nsplit > 1) {
      const dim3 jgrid((unsigned)((per + fast::kRmThreads - 1) / fast::kRmThreads), ncand), jblock(fast::kRmThreads);
      if constexpr (Fam::delay) hipLaunchKernelGGL(fast::frbch_post_rmd_join, jgrid, jblock, 0, ps.s, p);
      else hipLaunchKernelGGL(fast::frbch_post_rm_join, jgrid, jblock, 0, ps.s, p);
      POST_DEV(dev_check_launch(), Fam::join);
    }
    return FRBCH_OK;
  }
#endif
  if constexpr (Fam::delay) DEV_LAUNCH(frbch_post_rmd, (per + 255) / 256, ncand, 256, 0, ps.s, p);
  else DEV_LAUNCH(frbch_post_rm, (per + 255) / 256, ncand, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), Fam::launch);
  return FRBCH_OK;
}

// ---- the peaks of step 3: what both members ask of a power series and of a channel selection --------------------------
// the parabola through three neighbouring trials: the vertex offset in trial steps, or false (the grid value stands)
inline bool rm_vertex(bool interior, double ym, double y0, double yp, double* delta) {
  POST_NO_CONTRACT
  if (!interior) return false;
  const double den = (ym - 2.0 * y0) + yp;
  if (!(den < 0.0)) return false;
  const double diff = ym - yp;
  *delta = (0.5 * diff) / den;
  return true;
}

// the sum of noise_q^2 + noise_u^2 over the used channels of one candidate, whose noises begin at `at` (0 without both)
inline double rm_noise_sum(const uint8_t* us, const float* noise_q, const float* noise_u, size_t at, uint32_t nchan) {
  POST_NO_CONTRACT
  double acc = 0.0;
  if (noise_q && noise_u)
    for (uint32_t c = 0; c < nchan; ++c)
      if (us[c]) {
        const double nq = (double)noise_q[at + c], nu = (double)noise_u[at + c];
        const double a = nq * nq, b = nu * nu;
        acc = acc + (a + b);
      }
  return acc;
}

// the used channels of a selection and their spans of lambda^2 and of frequency, as fwhm and fwhm_tau want them
struct RmSpan {
  uint32_t N;
  double l2, f;                                  // hi - lo, 0 where fewer than two values differ
  double fwhm() const { return l2 > 0.0 ? (2.0 * sqrt(3.0)) / l2 : 0.0; }
  double fwhm_tau() const { return f > 0.0 ? (2.0 * sqrt(3.0)) / (kRmPi * f) : 0.0; }
};
inline RmSpan rm_span(const frbch_fil_desc* fil, const std::vector<double>& l2, const uint8_t* us) {
  POST_NO_CONTRACT
  uint32_t N = 0;
  double lo = 0.0, hi = 0.0, flo = 0.0, fhi = 0.0;
  for (uint32_t c = 0; c < fil->nchan; ++c)
    if (us[c]) {
      const double f = fil->fch1_mhz + (double)c * fil->foff_mhz;
      if (!N || l2[c] < lo) lo = l2[c];
      if (!N || l2[c] > hi) hi = l2[c];
      if (!N || f < flo) flo = f;
      if (!N || f > fhi) fhi = f;
      ++N;
    }
  return RmSpan{N, hi > lo ? hi - lo : 0.0, fhi > flo ? fhi - flo : 0.0};
}

int rm_peaks_run(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                 uint32_t ncand, const frbch_rm_params* par, frbch_rm_result* res) {
  POST_NO_CONTRACT
  const uint32_t nchan = fil->nchan, nphi = par->nphi;
  const std::vector<double> l2 = rm_l2(fil);
  for (uint32_t i = 0; i < ncand; ++i) {
    frbch_rm_result& r = res[i];
    memset(&r, 0, sizeof r);
    const float* f = F + (size_t)i * nphi * 2;
    const uint8_t* us = used + (size_t)i * nchan;
    auto power = [&](uint32_t k) {
      const double re = (double)f[2 * (size_t)k], im = (double)f[2 * (size_t)k + 1];
      const double a = re * re, b = im * im;
      return a + b;
    };
    uint32_t kp = 0;
    double best = power(0);
    for (uint32_t k = 1; k < nphi; ++k) {
      const double v = power(k);
      if (v > best) { best = v; kp = k; }
    }
    r.kpeak = kp;
    r.rm = par->phi_lo + (double)kp * par->dphi;
    r.peak = sqrt(best);
    const bool interior = kp > 0 && kp + 1 < nphi;
    const double ym = interior ? power(kp - 1) : 0.0, yp = interior ? power(kp + 1) : 0.0;
    double delta = 0.0;
    if (rm_vertex(interior, ym, best, yp, &delta)) {
      r.rm = par->phi_lo + ((double)kp + delta) * par->dphi;
      const double corr = (0.25 * (ym - yp)) * delta;
      r.peak = sqrt(best - corr);
      r.fitted = 1;
    }
    r.pa0 = atan2((double)f[2 * (size_t)kp + 1], (double)f[2 * (size_t)kp]) / 2.0;
    const RmSpan span = rm_span(fil, l2, us);
    const double acc = rm_noise_sum(us, noise_q, noise_u, (size_t)i * nchan, nchan);
    r.nused = span.N;
    if (span.N) r.sigma_f = sqrt(acc / 2.0) / (double)span.N;
    if (r.sigma_f > 0.0) r.snr = sqrt(best) / r.sigma_f;
    r.fwhm = span.fwhm();
    if (r.snr > 0.0) r.rm_err = r.fwhm / (2.0 * r.snr);
  }
  return FRBCH_OK;
}

// peak and ridge of one map P[ntau][nphi] into r (tau, rm, fitted_*, mpeak, kpeak, ridge_slope, nridge); -> P[mp][kp]
double rmd_map_peak(const double* P, const frbch_rmd_params* par, frbch_rmd_result& r) {
  POST_NO_CONTRACT
  const size_t nphi = par->nphi, ntau = par->ntau;
  size_t at = 0;
  double best = P[0];
  for (size_t x = 1; x < ntau * nphi; ++x)
    if (P[x] > best) { best = P[x]; at = x; }
  const size_t mp = at / nphi, kp = at % nphi;
  r.mpeak = (uint32_t)mp;
  r.kpeak = (uint32_t)kp;
  double delta = 0.0;
  r.tau = par->tau_lo + (double)mp * par->dtau;
  if (rm_vertex(mp > 0 && mp + 1 < ntau, mp > 0 ? P[at - nphi] : 0.0, best, mp + 1 < ntau ? P[at + nphi] : 0.0, &delta)) {
    r.tau = par->tau_lo + ((double)mp + delta) * par->dtau;
    r.fitted_tau = 1;
  }
  r.rm = par->phi_lo + (double)kp * par->dphi;
  if (rm_vertex(kp > 0 && kp + 1 < nphi, kp > 0 ? P[at - 1] : 0.0, best, kp + 1 < nphi ? P[at + 1] : 0.0, &delta)) {
    r.rm = par->phi_lo + ((double)kp + delta) * par->dphi;
    r.fitted_rm = 1;
  }
  std::vector<double> ts, fs;
  const double floor_ = 0.5 * best;
  for (size_t m = 0; m < ntau; ++m) {
    const double* row = P + m * nphi;
    size_t km = 0;
    for (size_t k = 1; k < nphi; ++k)
      if (row[k] > row[km]) km = k;
    if (row[km] >= floor_) {
      ts.push_back(par->tau_lo + (double)m * par->dtau);
      fs.push_back(par->phi_lo + (double)km * par->dphi);
    }
  }
  r.nridge = (uint32_t)ts.size();
  if (ts.size() >= 2) {
    double st = 0.0, sf = 0.0;
    for (size_t j = 0; j < ts.size(); ++j) { st = st + ts[j]; sf = sf + fs[j]; }
    const double mt = st / (double)ts.size(), mf = sf / (double)ts.size();
    double sxx = 0.0, sxy = 0.0;
    for (size_t j = 0; j < ts.size(); ++j) {
      const double dt = ts[j] - mt, df = fs[j] - mf;
      const double a = dt * dt, b = dt * df;
      sxx = sxx + a;
      sxy = sxy + b;
    }
    if (sxx > 0.0) r.ridge_slope = sxy / sxx;
  }
  return best;
}

int rmd_peaks_run(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                  uint32_t ncand, const frbch_rmd_params* par, frbch_rmd_result* res) {
  POST_NO_CONTRACT
  const uint32_t nchan = fil->nchan;
  const size_t per = (size_t)par->ntau * par->nphi;
  const std::vector<double> l2 = rm_l2(fil);
  std::vector<double> P(per), Psum(per, 0.0);
  std::vector<uint8_t> any(nchan, 0);
  uint32_t entered = 0;
  auto widths = [&](const uint8_t* us, frbch_rmd_result& r) {
    const RmSpan span = rm_span(fil, l2, us);
    r.fwhm = span.fwhm();
    r.fwhm_tau = span.fwhm_tau();
    return span.N;
  };
  auto errors = [](frbch_rmd_result& r) {
    if (r.snr > 0.0) {
      r.rm_err = r.fwhm / (2.0 * r.snr);
      r.tau_err = r.fwhm_tau / (2.0 * r.snr);
    }
  };
  for (uint32_t i = 0; i < ncand; ++i) {
    frbch_rmd_result& r = res[i];
    memset(&r, 0, sizeof r);
    const float* f = F + (size_t)i * per * 2;
    const uint8_t* us = used + (size_t)i * nchan;
    for (size_t x = 0; x < per; ++x) {
      const double re = (double)f[2 * x], im = (double)f[2 * x + 1];
      const double a = re * re, b = im * im;
      P[x] = a + b;
    }
    const double best = rmd_map_peak(P.data(), par, r);
    const size_t at = (size_t)r.mpeak * par->nphi + r.kpeak;
    r.peak = sqrt(best);
    r.psi = atan2((double)f[2 * at + 1], (double)f[2 * at]);
    r.nused = widths(us, r);
    const double acc = rm_noise_sum(us, noise_q, noise_u, (size_t)i * nchan, nchan);
    if (r.nused) r.sigma_f = sqrt(acc / 2.0) / (double)r.nused;
    if (r.sigma_f > 0.0) r.snr = sqrt(best) / r.sigma_f;
    errors(r);
    if (r.sigma_f > 0.0 && r.nused) {
      const double s2 = r.sigma_f * r.sigma_f;
      for (size_t x = 0; x < per; ++x) Psum[x] = Psum[x] + P[x] / s2;
      for (uint32_t c = 0; c < nchan; ++c)
        if (us[c]) any[c] = 1;
      ++entered;
    }
  }
  frbch_rmd_result& r = res[ncand];
  memset(&r, 0, sizeof r);
  if (!entered) return FRBCH_OK;
  const double best = rmd_map_peak(Psum.data(), par, r);
  r.peak = r.snr = sqrt(best);
  r.sigma_f = 1.0;
  (void)widths(any.data(), r);
  r.nused = entered;
  errors(r);
  return FRBCH_OK;
}

}  // namespace

extern "C" int frbch_burstspec_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* par,
                                      const frbch_burst_cand* cands, uint32_t ncand) try {
  PostErr e{nullptr, 0};
  int rc = burst_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  BurstPlan plan;
  rc = burst_build(fil, cands, ncand, &plan, e);
  return rc ? rc : (burst_fast_layout(fil, d_rows) ? 1 : 0);
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

namespace {
// step 1 inside a scope: the sums into d_sums, then host copies of sums, spectra, noise and `used` (all synchronised)
int burst_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* par,
              const frbch_burst_cand* cands, uint32_t ncand, const float* gain, BurstSums* d_sums, PostScope& ps,
              std::vector<frbch_burst_sums>* sums, float* spec, float* noise, uint8_t* used, uint32_t* kernel_used, const PostErr& e) {
  BurstPlan plan;
  int rc = burst_build(fil, cands, ncand, &plan, e);
  if (rc) return rc;
  const bool fastk = burst_fast_layout(fil, d_rows);
  if ((rc = burst_launch(fil, d_rows, nrows, plan, ncand, d_sums, fastk, ps, e)) != 0) return rc;
  const size_t n = (size_t)ncand * fil->nifs * fil->nchan;
  sums->resize(n);
  POST_DEV(dev_d2h(sums->data(), d_sums, n * sizeof(frbch_burst_sums), ps.s), "download sums");
  POST_DEV(dev_sync(ps.s), "sync");
  burst_derive(fil, par->products, sums->data(), ncand, gain, spec, noise, used);
  if (kernel_used) *kernel_used = fastk ? 1 : 0;
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_burstspec_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* par,
                                      const frbch_burst_cand* cands, uint32_t ncand, const float* gain, int device,
                                      frbch_burst_sums* d_sums, float* spec, float* noise, uint8_t* used, uint32_t* kernel_used,
                                      char* err, size_t err_cap) try {
  static_assert(sizeof(BurstSums) == sizeof(frbch_burst_sums) && sizeof(BurstSums) == 32, "frbch_burst_sums");
  PostErr e{err, err_cap};
  int rc = burst_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!d_rows || !d_sums) return e.fail(FRBCH_E_ARG, "null argument");
  const size_t n = (size_t)ncand * fil->nifs * fil->nchan;
  std::vector<frbch_burst_sums> sums;
  std::vector<float> sp(n), nz(n);
  std::vector<uint8_t> us((size_t)ncand * fil->nchan);
  rc = burst_device_call(device, e, [&](PostScope& ps) {
    return burst_run(fil, d_rows, nrows, par, cands, ncand, gain, (BurstSums*)d_sums, ps, &sums, sp.data(), nz.data(), us.data(), kernel_used, e);
  });
  if (rc) return rc;
  deliver(spec, sp);
  deliver(noise, nz);
  deliver(used, us);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstspec_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* par,
                                    const frbch_burst_cand* cands, uint32_t ncand, const float* gain, int device,
                                    frbch_burst_sums* sums, float* spec, float* noise, uint8_t* used, uint32_t* kernel_used,
                                    char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = burst_check(fil, nrows, par, cands, ncand, e);
  if (rc) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  void* d_rows = hs.in(rows, post_rows_bytes(fil, nrows));
  const size_t nb = (size_t)ncand * fil->nifs * fil->nchan * sizeof(frbch_burst_sums);
  frbch_burst_sums* d_sums = sums ? hs.out(sums, nb) : (frbch_burst_sums*)hs.scratch(nb);
  return hs.run(e, "device memory for the rows and the sums", "upload rows", "download sums", [&]() {
    return frbch_burstspec_device(fil, d_rows, nrows, par, cands, ncand, gain, device, d_sums, spec, noise, used, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_rm_table(int32_t* out) {
  if (!out) return FRBCH_E_ARG;
  rm_table_fill(out);
  return FRBCH_OK;
}

// ---- the entry points of the family, each body once; the extern "C" names below only name the member (by its grid record) --
namespace {
static_assert(sizeof(RmdRec) == 32 && sizeof(frbch_rmd_params) == 48 && sizeof(frbch_rmd_result) == 112, "delay x RM records");

// floats of F
template <class Par> size_t rm_nf(uint32_t ncand, const Par* par) { return (size_t)ncand * RmFam<Par>::ntau(par) * par->nphi * 2; }

template <class Par>
int rm_family_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                    uint32_t ncand, const Par* par, typename RmFam<Par>::Res* res) {
  if constexpr (RmFam<Par>::delay) return rmd_peaks_run(fil, F, used, noise_q, noise_u, ncand, par, res);
  else return rm_peaks_run(fil, F, used, noise_q, noise_u, ncand, par, res);
}

template <class Par> int rm_entry_kernel(const frbch_fil_desc* fil, const float* d_F, uint32_t ncand, const Par* par, uint32_t* nsplit) try {
  PostErr e{nullptr, 0};
  const int rc = rm_check(fil, ncand, par, e);
  if (rc) return rc;
  if (!d_F) return FRBCH_E_ARG;
  const RmPlanRule rule = rm_plan_rule(fil->nchan, ncand, par->nphi, RmFam<Par>::ntau(par), d_F);
  if (nsplit) *nsplit = (uint32_t)rule.nsplit;
  return rule.fastk ? 1 : 0;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

template <class Par>
int rm_entry_device(const frbch_fil_desc* fil, const float* d_q, const float* d_u, const uint8_t* d_used, uint32_t ncand, const Par* par,
                    int device, float* d_F, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = rm_check(fil, ncand, par, e);
  if (rc) return rc;
  if (!d_q || !d_u || !d_used || !d_F) return e.fail(FRBCH_E_ARG, "null argument");
  const size_t n = (size_t)ncand * fil->nchan;
  std::vector<float> q(n), u(n);
  std::vector<uint8_t> used(n);
  RmPlan<typename RmFam<Par>::Rec> plan;
  return burst_device_call(device, e, [&](PostScope& ps) {
    int rc;
    POST_DEV(dev_d2h(q.data(), d_q, n * sizeof(float), ps.s), "download q");
    POST_DEV(dev_d2h(u.data(), d_u, n * sizeof(float), ps.s), "download u");
    POST_DEV(dev_d2h(used.data(), d_used, n, ps.s), "download used");
    POST_DEV(dev_sync(ps.s), "sync");
    if ((rc = rm_build(fil, q.data(), u.data(), used.data(), ncand, par, &plan, e)) != 0) return rc;
    if ((rc = rm_launch(fil, ncand, par, plan, d_F, ps, kernel_used, e)) != 0) return rc;
    POST_DEV(dev_sync(ps.s), "sync");       // (the host vectors the uploads read stay alive until here)
    return (int)FRBCH_OK;
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

template <class Par>
int rm_entry_host(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand, const Par* par, int device,
                  float* F, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = rm_check(fil, ncand, par, e);
  if (rc) return rc;
  if (!q || !u || !used || !F) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t n = (size_t)ncand * fil->nchan;
  HostStage hs;
  const float* d_q = hs.in(q, n * sizeof(float));
  const float* d_u = hs.in(u, n * sizeof(float));
  const uint8_t* d_used = hs.in(used, n);
  float* d_F = hs.out(F, rm_nf(ncand, par) * sizeof(float));
  return hs.run(e, "device memory for the spectra and F", "upload spectra", "download F",
                [&]() { return rm_entry_device(fil, d_q, d_u, d_used, ncand, par, device, d_F, kernel_used, err, err_cap); });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

template <class Par>
int rm_entry_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u, uint32_t ncand,
                   const Par* par, typename RmFam<Par>::Res* results, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  const int rc = rm_check(fil, ncand, par, e);
  if (rc) return rc;
  if (!F || !used || !results) return e.fail(FRBCH_E_ARG, "null argument");
  return rm_family_peaks(fil, F, used, noise_q, noise_u, ncand, par, results);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// the composite: rows -> spectra (step 1) -> Q, U and their noises, less the flagged channels -> the transform -> the peaks
template <class Par>
int rm_entry_burst_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                          const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag, const Par* par, int device,
                          float* spec, float* noise, uint8_t* used, float* F, typename RmFam<Par>::Res* results, uint32_t* kernel_used,
                          char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if (fil->nifs != 4) return e.fail(FRBCH_E_ARG, "the composite needs the four products of a full-Stokes file (nifs = 4)");
  if ((rc = rm_check(fil, ncand, par, e)) != 0) return rc;
  if (!d_rows || !spec || !noise || !used || !F || !results) return e.fail(FRBCH_E_ARG, "null argument");
  const size_t nchan = fil->nchan, n = (size_t)ncand * nchan, nF = rm_nf(ncand, par);
  std::vector<frbch_burst_sums> sums;
  std::vector<float> q(n), u(n), nq(n), nu(n);
  RmPlan<typename RmFam<Par>::Rec> plan;
  uint32_t k[3] = {0, 0, 1};
  rc = burst_device_call(device, e, [&](PostScope& ps) {
    int rc;
    BurstSums* d_sums = nullptr;
    float* d_F = nullptr;
    POST_DEV(ps.alloc(&d_sums, n * 4 * sizeof(BurstSums)), "hipMalloc");
    POST_DEV(ps.alloc(&d_F, nF * sizeof(float)), "hipMalloc");
    if ((rc = burst_run(fil, d_rows, nrows, bpar, cands, ncand, gain, d_sums, ps, &sums, spec, noise, used, &k[0], e)) != 0) return rc;
    for (uint32_t i = 0; i < ncand; ++i)
      for (size_t c = 0; c < nchan; ++c) {
        if (flag && flag[c]) used[i * nchan + c] = 0;
        q[i * nchan + c] = spec[((size_t)i * 4 + 1) * nchan + c];
        u[i * nchan + c] = spec[((size_t)i * 4 + 2) * nchan + c];
        nq[i * nchan + c] = noise[((size_t)i * 4 + 1) * nchan + c];
        nu[i * nchan + c] = noise[((size_t)i * 4 + 2) * nchan + c];
      }
    if ((rc = rm_build(fil, q.data(), u.data(), used, ncand, par, &plan, e)) != 0) return rc;
    if ((rc = rm_launch(fil, ncand, par, plan, d_F, ps, &k[1], e)) != 0) return rc;
    POST_DEV(dev_d2h(F, d_F, nF * sizeof(float), ps.s), "download F");
    POST_DEV(dev_sync(ps.s), "sync");
    return (int)FRBCH_OK;
  });
  if (rc) return rc;
  deliver(kernel_used, k);
  return rm_family_peaks(fil, F, used, nq.data(), nu.data(), ncand, par, results);
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

template <class Par>
int rm_entry_burst_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                        const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag, const Par* par, int device,
                        float* spec, float* noise, uint8_t* used, float* F, typename RmFam<Par>::Res* results, uint32_t* kernel_used,
                        char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  const int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return rm_entry_burst_device(fil, d_rows, nrows, bpar, cands, ncand, gain, flag, par, device, spec, noise, used, F, results, kernel_used,
                                 err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }
}  // namespace

extern "C" int frbch_rmsynth_kernel(const frbch_fil_desc* fil, const float* d_F, uint32_t ncand, const frbch_rm_params* par, uint32_t* nsplit) {
  return rm_entry_kernel(fil, d_F, ncand, par, nsplit);
}
extern "C" int frbch_rmdelay_kernel(const frbch_fil_desc* fil, const float* d_F, uint32_t ncand, const frbch_rmd_params* par, uint32_t* nsplit) {
  return rm_entry_kernel(fil, d_F, ncand, par, nsplit);
}

extern "C" int frbch_rmsynth_device(const frbch_fil_desc* fil, const float* d_q, const float* d_u, const uint8_t* d_used, uint32_t ncand,
                                    const frbch_rm_params* par, int device, float* d_F, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_device(fil, d_q, d_u, d_used, ncand, par, device, d_F, kernel_used, err, err_cap);
}
extern "C" int frbch_rmdelay_device(const frbch_fil_desc* fil, const float* d_q, const float* d_u, const uint8_t* d_used, uint32_t ncand,
                                    const frbch_rmd_params* par, int device, float* d_F, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_device(fil, d_q, d_u, d_used, ncand, par, device, d_F, kernel_used, err, err_cap);
}

extern "C" int frbch_rmsynth_host(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand,
                                  const frbch_rm_params* par, int device, float* F, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_host(fil, q, u, used, ncand, par, device, F, kernel_used, err, err_cap);
}
extern "C" int frbch_rmdelay_host(const frbch_fil_desc* fil, const float* q, const float* u, const uint8_t* used, uint32_t ncand,
                                  const frbch_rmd_params* par, int device, float* F, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_host(fil, q, u, used, ncand, par, device, F, kernel_used, err, err_cap);
}

extern "C" int frbch_rm_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                              uint32_t ncand, const frbch_rm_params* par, frbch_rm_result* results, char* err, size_t err_cap) {
  return rm_entry_peaks(fil, F, used, noise_q, noise_u, ncand, par, results, err, err_cap);
}
extern "C" int frbch_rmdelay_peaks(const frbch_fil_desc* fil, const float* F, const uint8_t* used, const float* noise_q, const float* noise_u,
                                   uint32_t ncand, const frbch_rmd_params* par, frbch_rmd_result* results, char* err, size_t err_cap) {
  return rm_entry_peaks(fil, F, used, noise_q, noise_u, ncand, par, results, err, err_cap);
}

extern "C" int frbch_burst_rm_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                     const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                                     const frbch_rm_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                                     frbch_rm_result* results, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_burst_device(fil, d_rows, nrows, bpar, cands, ncand, gain, flag, par, device, spec, noise, used, F, results, kernel_used, err, err_cap);
}
extern "C" int frbch_burst_polcal_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                         const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                                         const frbch_rmd_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                                         frbch_rmd_result* results, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_burst_device(fil, d_rows, nrows, bpar, cands, ncand, gain, flag, par, device, spec, noise, used, F, results, kernel_used, err, err_cap);
}

extern "C" int frbch_burst_rm_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                   const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                                   const frbch_rm_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                                   frbch_rm_result* results, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_burst_host(fil, rows, nrows, bpar, cands, ncand, gain, flag, par, device, spec, noise, used, F, results, kernel_used, err, err_cap);
}
extern "C" int frbch_burst_polcal_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                       const frbch_burst_cand* cands, uint32_t ncand, const float* gain, const uint8_t* flag,
                                       const frbch_rmd_params* par, int device, float* spec, float* noise, uint8_t* used, float* F,
                                       frbch_rmd_result* results, uint32_t* kernel_used, char* err, size_t err_cap) {
  return rm_entry_burst_host(fil, rows, nrows, bpar, cands, ncand, gain, flag, par, device, spec, noise, used, F, results, kernel_used, err, err_cap);
}

// ---------------------------------------------------------------------------------------------------------------------
// polarisation profile of a burst: derotated I, L, V and PA per time bin (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint64_t kPolMaxOut = 1ull << 22, kPolPartCap = 1ull << 30;

const char* pol_bad_ref(const frbch_prof_params& p) {
  return p.ref > FRBCH_PROF_REF_ZERO ? "ref must be 0 (the mean lambda^2) or 1 (lambda^2 = 0)" : nullptr;
}

int pol_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_burst_params* bpar, const frbch_burst_cand* cands,
              uint32_t ncand, const frbch_prof_params* par, const PostErr& e) {
  POST_NO_CONTRACT
  int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if (fil->nifs != 4) return e.fail(FRBCH_E_ARG, "the profile needs the four products of a full-Stokes file (nifs = 4)");
  if ((rc = window_check(fil, par, "the profile", "frbch_prof_params", {nullptr, pol_bad_ref, nullptr}, e)) != 0) return rc;
  if (!(fil->fch1_mhz + (double)(fil->nchan - 1) * fil->foff_mhz > 0)) return e.fail(FRBCH_E_ARG, "a channel frequency that is not positive");
  if ((uint64_t)ncand * par->nbin > kPolMaxOut) return e.fail(FRBCH_E_ARG, "ncand * nbin exceeds 2^22: cut the batch into several calls");
  return FRBCH_OK;
}

int pol_check_rm(const double* rm, uint32_t ncand, const PostErr& e) {
  if (!rm) return e.fail(FRBCH_E_ARG, "null argument");
  for (uint32_t i = 0; i < ncand; ++i)
    if (!(fabs(rm[i]) <= kRmPhiMax)) return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": an rm that is not finite or above 1e7 rad m^-2 in size");
  return FRBCH_OK;
}

int pol_check_tau(const double* tau, uint32_t ncand, const PostErr& e) {
  for (uint32_t i = 0; tau && i < ncand; ++i)
    if (!(fabs(tau[i]) <= kRmdTauLim)) return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": a tau that is not finite or above 100 microseconds in size");
  return FRBCH_OK;
}

// The plan rule of the profile -- the one decision behind frbch_polprof_device's launches, kernel_used[1] and
// frbch_polprof_kernel's answer.  The fast kernel wants the layout of the fast burst-sums kernel (only the ADDRESS of d_rows
// is examined), room in its stage of kPpSpan rows for one bin behind the largest delay spread of any 64-byte tile of any
// candidate (tile_scan, TileScan::brun, which gives the bins of a run as well), and partials of at most 2^30 bytes.  The
// emulator build has no such kernel: generic.
struct PolPlanRule { bool fastk; int brun, ntile; };
PolPlanRule pol_plan_rule(const frbch_fil_desc* fil, const void* d_rows, const std::vector<int32_t>& delays, uint32_t ncand,
                          const frbch_prof_params* par) {
  PolPlanRule r{false, 0, 0};
#ifndef FRBCH_NO_FAST
  if (!burst_fast_layout(fil, d_rows)) return r;
  const TileScan ts = tile_scan(fil, delays);
  const int brun = ts.brun(ncand, 1, 1, (int64_t)fast::kPpSpan, par->nbin, par->tfactor);
  if (!brun || (uint64_t)ncand * ts.ntile * par->nbin * 36ull > kPolPartCap) return r;
  r = PolPlanRule{true, brun, (int)ts.ntile};
#else
  (void)fil; (void)d_rows; (void)delays; (void)ncand; (void)par;
#endif
  return r;
}

struct PolOut {
  std::vector<long long> acc;
  std::vector<uint32_t> hits;
  std::vector<frbch_prof_bin> bins;
  std::vector<frbch_prof_result> res;
  std::vector<uint8_t> used;
  uint32_t k[2] = {0, 0};
};

// floor(a / b), b > 0
long long pol_floordiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// everything of a call inside its scope: the burst sums, the records, the launches, the derivation (all synchronised)
int pol_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
            const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const double* tau, const float* gain,
            const uint8_t* flag, const frbch_prof_params* par, PostScope& ps, PolOut* out, const PostErr& e) {
  POST_NO_CONTRACT
  const size_t nchan = fil->nchan, n = (size_t)ncand * nchan, nbin = par->nbin;
  BurstPlan bplan;
  int rc = burst_build(fil, cands, ncand, &bplan, e);
  if (rc) return rc;
  const PolPlanRule rule = pol_plan_rule(fil, d_rows, bplan.delays, ncand, par);
  std::vector<frbch_burst_sums> sums;
  std::vector<float> spec(n * 4), noise(n * 4);
  out->used.assign(n, 0);
  BurstSums* d_sums = nullptr;
  POST_DEV(ps.alloc(&d_sums, n * 4 * sizeof(BurstSums)), "hipMalloc");
  if ((rc = burst_run(fil, d_rows, nrows, bpar, cands, ncand, gain, d_sums, ps, &sums, spec.data(), noise.data(), out->used.data(), &out->k[0], e)) != 0) return rc;
  ps.drop(d_sums);
  uint8_t* used = out->used.data();
  if (flag)
    for (uint32_t i = 0; i < ncand; ++i)
      for (size_t c = 0; c < nchan; ++c)
        if (flag[c]) used[i * nchan + c] = 0;

  // the records
  const bool coh = bpar->products == FRBCH_BURST_COHERENCY;
  const std::vector<double> l2 = rm_l2(fil);
  std::vector<int32_t> table(kRmTableN);
  rm_table_fill(table.data());
  std::vector<PolRec> rec(n);
  std::vector<PolCand> pc(ncand);
  out->res.assign(ncand, frbch_prof_result{});
  memset((void*)rec.data(), 0, n * sizeof(PolRec));
  for (size_t o = 0; o < n; ++o) rec[o].delay = bplan.delays[o];      // (of unused channels too: the fast kernel sizes its stage by them)
  memset((void*)out->res.data(), 0, (size_t)ncand * sizeof(frbch_prof_result));
  const double tf = (double)par->tfactor;
  for (uint32_t i = 0; i < ncand; ++i) {
    frbch_prof_result& r = out->res[i];
    const uint8_t* us = used + (size_t)i * nchan;
    const long long on_lo = (long long)cands[i].sample - (long long)(cands[i].width / 2);
    const long long t0 = (long long)cands[i].sample - (long long)(par->nbin / 2) * (long long)par->tfactor;
    pc[i].t0 = t0;
    pc[i].scale = 0.0;
    const long long last = (long long)nbin - 1;
    r.on_lo_bin = (uint32_t)std::min(last, std::max(0ll, pol_floordiv(on_lo - t0, (long long)par->tfactor)));
    r.on_hi_bin = (uint32_t)std::min(last, std::max(0ll, pol_floordiv(on_lo + (long long)cands[i].width - 1 - t0, (long long)par->tfactor)));
    uint32_t N = 0;
    double sum = 0.0, fsum = 0.0, gmax = 0.0;
    for (size_t c = 0; c < nchan; ++c)
      if (us[c]) {
        ++N;
        sum = sum + l2[c];
        fsum = fsum + (fil->fch1_mhz + (double)c * fil->foff_mhz);
        for (size_t p = 0; p < 4; ++p) gmax = std::max(gmax, gain ? fabs((double)gain[p * nchan + c]) : 1.0);
      }
    r.nused = N;
    if (N == 0 || gmax == 0.0) continue;                       // every output 0: no used record
    const double lref = par->ref == FRBCH_PROF_REF_MEAN ? sum / (double)N : 0.0;
    const double f0 = fsum / (double)N;                        // (of the delay term: the polarisation calibration section)
    const double M = (tf * ldexp(1.0, fil->nbits)) * gmax;
    int ex = 0;
    (void)frexp(M, &ex);
    r.k = 22 - ex;
    r.lref = lref;
    pc[i].scale = ldexp(1.0, r.k);
    double W[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t c = 0; c < nchan; ++c) {
      PolRec& q = rec[(size_t)i * nchan + c];
      if (!us[c]) continue;
      q.used = 1;
      double w[4];
      for (size_t p = 0; p < 4; ++p) {
        const OffStat off = burst_off_stat(sums[((size_t)i * 4 + p) * nchan + c]);
        const double g = gain ? (double)gain[p * nchan + c] : 1.0;
        q.mean[p] = off.mean;
        q.g[p] = g;
        const double gg = g * g;
        w[p] = gg * off.var;
      }
      if (coh) {
        const double wi = w[0] + w[1];
        W[0] = W[0] + wi; W[1] = W[1] + 4.0 * w[2]; W[2] = W[2] + 4.0 * w[3]; W[3] = W[3] + wi;
      } else {
        for (int p = 0; p < 4; ++p) W[p] = W[p] + w[p];
      }
      const double a = (l2[c] - lref) / kRmPi;
      uint64_t ph = rm_fix(rm[i] * a);
      if (tau) {
        const double b = (fil->fch1_mhz + (double)c * fil->foff_mhz) - f0;
        ph += rm_fix(tau[i] * b);
      }
      const int j = (int)(((ph + (1ull << 49)) >> 50) & 16383ull);
      q.cc = table[j];
      q.sc = table[(j - 4096) & 16383];
    }
    double sg[4];
    const double den = (double)N * tf;
    for (int p = 0; p < 4; ++p) {
      const double t1 = tf * W[p];
      sg[p] = sqrt(t1) / den;
    }
    r.sigma_i = sg[0]; r.sigma_q = sg[1]; r.sigma_u = sg[2]; r.sigma_v = sg[3];
    const double qq = sg[1] * sg[1], uu = sg[2] * sg[2];
    r.sigma_l = sqrt((qq + uu) / 2.0);
  }

  // the launches
  PolRec* d_rec = nullptr;
  PolCand* d_pc = nullptr;
  long long* d_acc = nullptr;
  uint32_t* d_hits = nullptr;
  POST_DEV(ps.alloc(&d_rec, n * sizeof(PolRec)), "hipMalloc");
  POST_DEV(ps.alloc(&d_pc, (size_t)ncand * sizeof(PolCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_acc, (size_t)ncand * nbin * 4 * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_hits, (size_t)ncand * nbin * sizeof(uint32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_rec, rec.data(), n * sizeof(PolRec), ps.s), "upload records");
  POST_DEV(dev_h2d(d_pc, pc.data(), (size_t)ncand * sizeof(PolCand), ps.s), "upload records");
  PolParams p = post_params<PolParams>(fil, d_rows, nrows);
  p.ncand = (int)ncand; p.cand = d_pc; p.rec = d_rec; p.acc = d_acc; p.hits = d_hits;
  p.nbin = (int)par->nbin; p.tfactor = (int)par->tfactor; p.coh = coh ? 1 : 0; p.ntile = rule.ntile; p.brun = rule.brun;
  out->k[1] = rule.fastk ? 1 : 0;
  bool launched = false;
#ifndef FRBCH_NO_FAST
  if (rule.fastk) {
    long long* d_part = nullptr;
    uint32_t* d_hpart = nullptr;
    const size_t np = (size_t)ncand * rule.ntile * nbin;
    POST_DEV(ps.alloc(&d_part, np * 4 * sizeof(long long)), "hipMalloc");
    POST_DEV(ps.alloc(&d_hpart, np * sizeof(uint32_t)), "hipMalloc");
    p.part = d_part; p.hpart = d_hpart;
    const dim3 grid((unsigned)rule.ntile, (unsigned)((par->nbin + rule.brun - 1) / rule.brun), ncand), block(fast::kPpThreads);
    if (fil->nbits == 8) POST_DEV(launch_lds(fast::frbch_post_polprof_fast<1>, grid, block, fast::kPpLds, ps.s, p), "LDS size");
    else POST_DEV(launch_lds(fast::frbch_post_polprof_fast<2>, grid, block, fast::kPpLds, ps.s, p), "LDS size");
    POST_DEV(dev_check_launch(), "launch profile");
    hipLaunchKernelGGL(fast::frbch_post_polprof_join, dim3((par->nbin + fast::kPpThreads - 1) / fast::kPpThreads, ncand), dim3(fast::kPpThreads), 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch profile join");
    launched = true;
  }
#endif
  if (!launched) {
    DEV_LAUNCH(frbch_post_polprof, (par->nbin + 255) / 256, ncand, 256, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch profile");
  }
  out->acc.resize((size_t)ncand * nbin * 4);
  out->hits.resize((size_t)ncand * nbin);
  POST_DEV(dev_d2h(out->acc.data(), d_acc, out->acc.size() * sizeof(long long), ps.s), "download profile");
  POST_DEV(dev_d2h(out->hits.data(), d_hits, out->hits.size() * sizeof(uint32_t), ps.s), "download profile");
  POST_DEV(dev_sync(ps.s), "sync");

  // the derivation
  out->bins.assign((size_t)ncand * nbin, frbch_prof_bin{});
  memset((void*)out->bins.data(), 0, out->bins.size() * sizeof(frbch_prof_bin));
  for (uint32_t i = 0; i < ncand; ++i) {
    const frbch_prof_result& r = out->res[i];
    if (pc[i].scale == 0.0) continue;
    const double inv = ldexp(1.0, -r.k), inv22 = ldexp(1.0, -(r.k + 22)), sl = r.sigma_l;
    for (size_t j = 0; j < nbin; ++j) {
      const long long* a = out->acc.data() + ((size_t)i * nbin + j) * 4;
      frbch_prof_bin& b = out->bins[(size_t)i * nbin + j];
      b.hits = out->hits[(size_t)i * nbin + j];
      if (!b.hits) continue;
      const double h = (double)b.hits;
      b.i = ((double)a[0] * inv) / h;
      b.q = ((double)a[1] * inv22) / h;
      b.u = ((double)a[2] * inv22) / h;
      b.v = ((double)a[3] * inv) / h;
      const double qq = b.q * b.q, uu = b.u * b.u;
      b.l = sqrt(qq + uu);
      if (b.l >= 1.57 * sl) {
        const double ll = b.l * b.l, s2 = sl * sl;
        b.l_db = sqrt(ll - s2);
      }
      b.pa = atan2(b.u, b.q) / 2.0;
      if (b.l_db > 0.0) {
        b.pa_err = sl / (2.0 * b.l_db);
        b.pa_valid = 1;
      }
    }
  }
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_polprof_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                    const frbch_burst_cand* cands, uint32_t ncand, const frbch_prof_params* par) try {
  PostErr e{nullptr, 0};
  int rc = pol_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  BurstPlan plan;
  if ((rc = burst_build(fil, cands, ncand, &plan, e)) != 0) return rc;
  return pol_plan_rule(fil, d_rows, plan.delays, ncand, par).fastk ? 1 : 0;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_polprof_cal_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                        const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const double* tau, const float* gain,
                                        const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                                    frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used,
                                    char* err, size_t err_cap) try {
  static_assert(sizeof(PolRec) == 80 && sizeof(frbch_prof_bin) == 72 && sizeof(frbch_prof_result) == 64 && sizeof(long long) == sizeof(int64_t), "profile records");
  PostErr e{err, err_cap};
  int rc = pol_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if (!d_rows) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = pol_check_rm(rm, ncand, e)) != 0) return rc;
  if ((rc = pol_check_tau(tau, ncand, e)) != 0) return rc;
  PolOut out;
  rc = burst_device_call(device, e, [&](PostScope& ps) { return pol_run(fil, d_rows, nrows, bpar, cands, ncand, rm, tau, gain, flag, par, ps, &out, e); });
  if (rc) return rc;
  deliver(acc, out.acc);
  deliver(hits, out.hits);
  deliver(bins, out.bins);
  deliver(results, out.res);
  deliver(used, out.used);
  deliver(kernel_used, out.k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_polprof_cal_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                      const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const double* tau, const float* gain,
                                      const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                                  frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used,
                                  char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = pol_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  if ((rc = pol_check_rm(rm, ncand, e)) != 0) return rc;
  if ((rc = pol_check_tau(tau, ncand, e)) != 0) return rc;
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return frbch_polprof_cal_device(fil, d_rows, nrows, bpar, cands, ncand, rm, tau, gain, flag, par, device, acc, hits, bins, results, used, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// the calls without a delay: tau = NULL
extern "C" int frbch_polprof_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                    const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const float* gain,
                                    const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                                    frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used,
                                    char* err, size_t err_cap) {
  return frbch_polprof_cal_device(fil, d_rows, nrows, bpar, cands, ncand, rm, nullptr, gain, flag, par, device, acc, hits, bins, results, used, kernel_used, err, err_cap);
}

extern "C" int frbch_polprof_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                  const frbch_burst_cand* cands, uint32_t ncand, const double* rm, const float* gain,
                                  const uint8_t* flag, const frbch_prof_params* par, int device, int64_t* acc, uint32_t* hits,
                                  frbch_prof_bin* bins, frbch_prof_result* results, uint8_t* used, uint32_t* kernel_used,
                                  char* err, size_t err_cap) {
  return frbch_polprof_cal_host(fil, rows, nrows, bpar, cands, ncand, rm, nullptr, gain, flag, par, device, acc, hits, bins, results, used, kernel_used, err, err_cap);
}

// ---------------------------------------------------------------------------------------------------------------------
// DM of a burst: fine DM scan, S/N and structure maxima (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kDmMaxTrial = 4096, kDmMaxWidths = 16;
constexpr uint64_t kDmMaxOut = 1ull << 24, kDmPartCap = 1ull << 30;

const char* dm_bad_ntrial(const frbch_dmscan_params& p) { return p.ntrial < 1 || p.ntrial > kDmMaxTrial ? "ntrial must be 1..4096" : nullptr; }
const char* dm_bad_ddm(const frbch_dmscan_params& p) {
  return p.ntrial > 1 && (!(p.ddm > 0.0) || !rm_finite(p.ddm)) ? "ddm must be finite and above 0" : nullptr;
}

int dm_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_burst_params* bpar, const frbch_burst_cand* cands,
             uint32_t ncand, const frbch_dmscan_params* par, const PostErr& e) {
  int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if ((rc = window_check(fil, par, "the DM scan", "frbch_dmscan_params", {dm_bad_ntrial, dm_bad_ddm, nullptr}, e)) != 0) return rc;
  if ((uint64_t)ncand * par->ntrial * fil->nchan > kCutTableCap) return e.fail(FRBCH_E_ARG, "ncand * ntrial * nchan exceeds 2^26: cut the batch or the scan");
  if ((uint64_t)ncand * par->ntrial * par->nbin > kDmMaxOut) return e.fail(FRBCH_E_ARG, "ncand * ntrial * nbin exceeds 2^24: cut the batch or the scan");
  return FRBCH_OK;
}

int dm_check_peaks(const frbch_dmscan_params* par, const frbch_dmscan_peak_params* pk, const PostErr& e) {
  if (!pk || pk->size != sizeof(frbch_dmscan_peak_params)) return e.fail(FRBCH_E_ARG, "frbch_dmscan_peak_params: wrong size");
  if (pk->nwidth < 1 || pk->nwidth > kDmMaxWidths) return e.fail(FRBCH_E_ARG, "nwidth must be 1..16");
  for (uint32_t i = 0; i < pk->nwidth; ++i)
    if (pk->widths[i] < 1 || pk->widths[i] > par->nbin || (i && pk->widths[i] <= pk->widths[i - 1]))
      return e.fail(FRBCH_E_ARG, "the widths must ascend within 1..nbin");
  if (par->nbin > 1 && (pk->smooth < 1 || pk->smooth > par->nbin - 1)) return e.fail(FRBCH_E_ARG, "smooth must be 1..nbin - 1");
  if (!(pk->fit_frac > 0.0) || !(pk->fit_frac < 1.0)) return e.fail(FRBCH_E_ARG, "fit_frac must lie inside (0, 1)");
  return FRBCH_OK;
}

// dm_k of every candidate, [ncand][ntrial]; a value outside [0, 1e5) is refused
int dm_trials(const frbch_burst_cand* cands, uint32_t ncand, const frbch_dmscan_params* par, std::vector<double>* dms, const PostErr& e) {
  POST_NO_CONTRACT
  dms->resize((size_t)ncand * par->ntrial);
  const double kc = (double)(par->ntrial / 2);
  for (uint32_t i = 0; i < ncand; ++i)
    for (uint32_t k = 0; k < par->ntrial; ++k) {
      double dm = cands[i].dm;
      if (par->ntrial > 1) {
        const double off = ((double)k - kc) * par->ddm;
        dm = cands[i].dm + off;
      }
      if (!(dm >= 0.0) || !(dm < 1.0e5)) return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": a trial DM outside [0, 1e5)");
      (*dms)[(size_t)i * par->ntrial + k] = dm;
    }
  return FRBCH_OK;
}

// the trial DMs and their delay table [ncand][ntrial][nchan]
int dm_build(const frbch_fil_desc* fil, const frbch_burst_cand* cands, uint32_t ncand, const frbch_dmscan_params* par,
             std::vector<double>* dms, std::vector<int32_t>* delays, const PostErr& e) {
  const int rc = dm_trials(cands, ncand, par, dms, e);
  if (rc) return rc;
  int64_t maxd = 0;
  *delays = post_delays(fil, dms->data(), (uint32_t)dms->size(), &maxd);
  if (maxd > (int64_t)1 << 30) return e.fail(FRBCH_E_ARG, "a dispersion delay of more than 2^30 samples");
  return FRBCH_OK;
}

// The plan rule of the scan -- the one decision behind frbch_dmscan_device's launches, kernel_used[1] and
// frbch_dmscan_kernel's answer.  The fast kernel wants the layout of the fast burst-sums kernel (only the ADDRESS of d_rows is
// examined), bins of at most kDmMaxT rows, a trial run -- the largest of 16, 8, 4, 2, 1 within ntrial -- whose delay range
// over any 64-byte tile of any candidate leaves room for one bin in the stage (tile_scan, dm_stage_brun), and partials of at
// most 2^30 bytes.  The emulator build has no such kernel: generic.
struct DmPlanRule { bool fastk; int trun, brun, ntile; };
#ifndef FRBCH_NO_FAST
// the bins of a run of the fast DM scan kernel's stage (kDmLds / (64 products) rows) at a trial run of `trun`; 0: none fits
int dm_stage_brun(const TileScan& ts, uint32_t products, uint32_t ncand, uint32_t ntrial, uint32_t trun, uint32_t nbin, uint32_t tfactor) {
  const int64_t cap = (int64_t)(fast::kDmLds / (64u * (products == FRBCH_BURST_COHERENCY ? 2u : 1u)));
  return ts.brun(ncand, ntrial, trun, cap, nbin, tfactor);
}
#endif
DmPlanRule dm_plan_rule(const frbch_fil_desc* fil, const void* d_rows, uint32_t products, const std::vector<int32_t>& delays,
                        uint32_t ncand, const frbch_dmscan_params* par) {
  DmPlanRule r{false, 0, 0, 0};
#ifndef FRBCH_NO_FAST
  if (!burst_fast_layout(fil, d_rows) || par->tfactor > (uint32_t)fast::kDmMaxT) return r;
  const TileScan ts = tile_scan(fil, delays);
  if ((uint64_t)ncand * ts.ntile * par->ntrial * par->nbin * 12ull > kDmPartCap) return r;
  for (uint32_t trun = (uint32_t)fast::kDmTrun; trun >= 1; trun /= 2) {
    if (trun > par->ntrial && trun > 1) continue;
    const int brun = dm_stage_brun(ts, products, ncand, par->ntrial, trun, par->nbin, par->tfactor);
    if (brun) return DmPlanRule{true, (int)trun, brun, (int)ts.ntile};
  }
#else
  (void)fil; (void)d_rows; (void)products; (void)delays; (void)ncand; (void)par;
#endif
  return r;
}

struct DmCurves {
  std::vector<double> snr, strc;
  std::vector<uint32_t> width, bin;
  std::vector<frbch_dmscan_result> res;
};

// B(w, j) of the header from the prefix sums of a trial
inline double dm_boxcar(const __int128* pa, const uint64_t* ph, uint32_t w, uint32_t j, double inv) {
  POST_NO_CONTRACT
  const uint64_t H = ph[j + w] - ph[j];
  if (!H) return 0.0;
  const double a = (double)(pa[j + w] - pa[j]);
  const double b = a * inv;
  return b / sqrt((double)H);
}

// the fit of one curve: -> the peak's trial, n, fitted, dm and (err != NULL) the half-width at 1 below the vertex
void dm_fit(const double* v, uint32_t nt, double fit_frac, const double* dms, double ddm, uint32_t* kpeak, uint32_t* nfit,
            uint32_t* fitted, double* dm, double* err) {
  POST_NO_CONTRACT
  uint32_t kp = 0;
  for (uint32_t k = 1; k < nt; ++k)
    if (v[k] > v[kp]) kp = k;
  *kpeak = kp; *nfit = 0; *fitted = 0; *dm = dms[kp];
  if (err) *err = 0.0;
  if (!(v[kp] > 0.0)) return;
  const double thr = fit_frac * v[kp];
  uint32_t lo = kp, hi = kp;
  while (lo > 0 && v[lo - 1] >= thr) --lo;
  while (hi + 1 < nt && v[hi + 1] >= thr) ++hi;
  *nfit = hi - lo + 1;
  if (*nfit < 3 || lo == 0 || hi == nt - 1) return;
  long long s[5] = {0, 0, 0, 0, 0};
  double T0 = 0.0, T1 = 0.0, T2 = 0.0;
  for (uint32_t k = lo; k <= hi; ++k) {
    const long long x = (long long)k - (long long)kp;
    s[0] += 1; s[1] += x; s[2] += x * x; s[3] += x * x * x; s[4] += x * x * x * x;
    const double xv = (double)x * v[k], xxv = (double)(x * x) * v[k];
    T0 = T0 + v[k];
    T1 = T1 + xv;
    T2 = T2 + xxv;
  }
  const double S0 = (double)s[0], S1 = (double)s[1], S2 = (double)s[2], S3 = (double)s[3], S4 = (double)s[4];
  const double m0 = S2 * S0 - S1 * S1, m1 = S3 * S0 - S1 * S2, m2 = S3 * S1 - S2 * S2;
  const double D = (S4 * m0 - S3 * m1) + S2 * m2;
  const double p1 = T1 * S0 - S1 * T0, p2 = T1 * S1 - S2 * T0, p3 = S3 * T0 - S2 * T1;
  const double Da = (T2 * m0 - S3 * p1) + S2 * p2;
  const double Db = (S4 * p1 - T2 * m1) + S2 * p3;
  const double a = Da / D, b = Db / D;
  if (!(a < 0.0)) return;
  const double vertex = (-b) / (2.0 * a);
  const double shift = vertex * ddm;
  *dm = dms[kp] + shift;
  *fitted = 1;
  if (err) *err = sqrt(-1.0 / a) * ddm;
}

// the peaks section of the header; every check has been made
void dm_peaks(const frbch_dmscan_params* par, const frbch_dmscan_peak_params* pk, const std::vector<double>& dms, uint32_t ncand,
              const int32_t* kscale, const uint32_t* nused, const int64_t* acc, const uint32_t* hits, DmCurves* out) {
  POST_NO_CONTRACT
  const uint32_t nt = par->ntrial, nb = par->nbin;
  out->snr.assign((size_t)ncand * nt, 0.0);
  out->strc.assign((size_t)ncand * nt, 0.0);
  out->width.assign((size_t)ncand * nt, 0);
  out->bin.assign((size_t)ncand * nt, 0);
  out->res.assign(ncand, frbch_dmscan_result{});
  memset((void*)out->res.data(), 0, (size_t)ncand * sizeof(frbch_dmscan_result));
  std::vector<__int128> pa(nb + 1);
  std::vector<uint64_t> ph(nb + 1);
  std::vector<double> z(nb);
  for (uint32_t i = 0; i < ncand; ++i) {
    if (!nused[i]) continue;
    frbch_dmscan_result& r = out->res[i];
    r.k = kscale[i];
    r.nused = nused[i];
    const double inv = ldexp(1.0, -kscale[i]);
    double* snr = out->snr.data() + (size_t)i * nt;
    double* strc = out->strc.data() + (size_t)i * nt;
    uint32_t* wd = out->width.data() + (size_t)i * nt;
    uint32_t* bn = out->bin.data() + (size_t)i * nt;
    for (uint32_t k = 0; k < nt; ++k) {
      const int64_t* a = acc + ((size_t)i * nt + k) * nb;
      const uint32_t* h = hits + ((size_t)i * nt + k) * nb;
      pa[0] = 0; ph[0] = 0;
      for (uint32_t j = 0; j < nb; ++j) { pa[j + 1] = pa[j] + (__int128)a[j]; ph[j + 1] = ph[j] + h[j]; }
      double best = dm_boxcar(pa.data(), ph.data(), pk->widths[0], 0, inv);
      uint32_t bw = pk->widths[0], bj = 0;
      for (uint32_t wi = 0; wi < pk->nwidth; ++wi) {
        const uint32_t w = pk->widths[wi];
        for (uint32_t j = 0; j + w <= nb; ++j) {
          const double B = dm_boxcar(pa.data(), ph.data(), w, j, inv);
          if (B > best) { best = B; bw = w; bj = j; }
        }
      }
      snr[k] = best; wd[k] = bw; bn[k] = bj;
      if (nb > 1) {
        const uint32_t s = pk->smooth;
        for (uint32_t j = 0; j + s <= nb; ++j) z[j] = dm_boxcar(pa.data(), ph.data(), s, j, inv);
        double sum = 0.0;
        for (uint32_t j = 0; j + s < nb; ++j) {
          const double d = z[j + 1] - z[j];
          const double dd = d * d;
          sum = sum + dd;
        }
        const double ex = (2.0 * (double)(nb - s)) / (double)s;
        strc[k] = sum - ex;
      }
    }
    const double* dm = dms.data() + (size_t)i * nt;
    dm_fit(snr, nt, pk->fit_frac, dm, par->ddm, &r.k_snr, &r.nfit_snr, &r.fitted_snr, &r.dm_snr, &r.dm_snr_err);
    r.snr_peak = snr[r.k_snr]; r.width_snr = wd[r.k_snr]; r.bin_snr = bn[r.k_snr];
    if (nb > 1) {
      dm_fit(strc, nt, pk->fit_frac, dm, par->ddm, &r.k_struct, &r.nfit_struct, &r.fitted_struct, &r.dm_struct, nullptr);
    } else {
      r.k_struct = 0; r.dm_struct = dm[0];
    }
    r.struct_peak = strc[r.k_struct]; r.snr_at_struct = snr[r.k_struct]; r.width_struct = wd[r.k_struct]; r.bin_struct = bn[r.k_struct];
  }
}

struct DmOut {
  std::vector<long long> acc;
  std::vector<uint32_t> hits;
  std::vector<uint8_t> used;
  DmCurves cv;
  uint32_t k[2] = {0, 0};
};

// The host preparation of the header's DM section, inside a scope: the burst sums at cand.dm (synchronised), then per
// candidate the window's first row, the records of the used channels, N_i and k_i.  The DM scan and the burst ACF share it.
struct DmPrep {
  std::vector<DmRec> rec;               // [ncand][nchan]
  std::vector<DmCand> dc;               // [ncand]
  std::vector<int32_t> kscale;          // [ncand]
  std::vector<uint32_t> nused;          // [ncand]
  std::vector<uint8_t> used;            // [ncand][nchan]
  uint32_t p0 = 0, np = 1;              // the first product read and their number
};
int dm_prepare(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
               const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, uint32_t par_nbin, uint32_t par_tfactor,
               PostScope& ps, DmPrep* out, uint32_t* kernel_used, const PostErr& e) {
  POST_NO_CONTRACT
  const size_t nchan = fil->nchan, n = (size_t)ncand * nchan, nifs = fil->nifs;
  int rc;
  std::vector<frbch_burst_sums> sums;
  std::vector<float> spec(n * nifs), noise(n * nifs);
  std::vector<uint8_t> bused(n);
  BurstSums* d_sums = nullptr;
  POST_DEV(ps.alloc(&d_sums, n * nifs * sizeof(BurstSums)), "hipMalloc");
  if ((rc = burst_run(fil, d_rows, nrows, bpar, cands, ncand, nullptr, d_sums, ps, &sums, spec.data(), noise.data(), bused.data(), kernel_used, e)) != 0) return rc;
  ps.drop(d_sums);

  // the records
  const bool coh = bpar->products == FRBCH_BURST_COHERENCY;
  const uint32_t p0 = coh ? 0u : fil->product, np = coh ? 2u : 1u;
  out->p0 = p0; out->np = np;
  out->rec.resize(n);
  out->dc.resize(ncand);
  out->kscale.assign(ncand, 0);
  out->nused.assign(ncand, 0);
  memset((void*)out->rec.data(), 0, n * sizeof(DmRec));
  out->used.assign(n, 0);
  for (uint32_t i = 0; i < ncand; ++i) {
    DmCand& dc = out->dc[i];
    dc.t0 = (long long)cands[i].sample - (long long)(par_nbin / 2) * (long long)par_tfactor;
    dc.scale = 0.0;
    double wmax = 0.0;
    for (size_t c = 0; c < nchan; ++c) {
      bool ok = !(flag && flag[c]);
      double mean = 0.0, var = 0.0;
      for (uint32_t p = p0; p < p0 + np; ++p) {
        const frbch_burst_sums& s = sums[((size_t)i * nifs + p) * nchan + c];
        if (s.on_hits == 0 || s.off_hits < 2) { ok = false; break; }
        const OffStat off = burst_off_stat(s);
        mean = p == p0 ? off.mean : mean + off.mean;
        var = p == p0 ? off.var : var + off.var;
      }
      if (!ok || !(var > 0.0)) continue;
      DmRec& q = out->rec[(size_t)i * nchan + c];
      q.mean = mean;
      q.w = 1.0 / sqrt(var);
      q.used = 1;
      out->used[(size_t)i * nchan + c] = 1;
      ++out->nused[i];
      wmax = std::max(wmax, q.w);
    }
    if (!out->nused[i]) continue;
    double M = ((double)par_tfactor * ldexp(1.0, fil->nbits)) * wmax;
    if (coh) M = 2.0 * M;
    int ex = 0;
    (void)frexp(M, &ex);
    out->kscale[i] = 40 - ex;
    dc.scale = ldexp(1.0, out->kscale[i]);
  }
  return FRBCH_OK;
}

// everything of a call inside its scope: the burst sums, the records, the launches, the peaks (all synchronised)
int dm_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
           const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_dmscan_params* par,
           const frbch_dmscan_peak_params* pk, PostScope& ps, DmOut* out, const PostErr& e) {
  POST_NO_CONTRACT
  const size_t nchan = fil->nchan, n = (size_t)ncand * nchan, nbin = par->nbin, nt = par->ntrial;
  std::vector<double> dms;
  std::vector<int32_t> delays;
  int rc = dm_build(fil, cands, ncand, par, &dms, &delays, e);
  if (rc) return rc;
  const DmPlanRule rule = dm_plan_rule(fil, d_rows, bpar->products, delays, ncand, par);
  DmPrep prep;
  if ((rc = dm_prepare(fil, d_rows, nrows, bpar, cands, ncand, flag, par->nbin, par->tfactor, ps, &prep, &out->k[0], e)) != 0) return rc;
  out->used.swap(prep.used);

  // the launches
  DmRec* d_rec = nullptr;
  DmCand* d_dc = nullptr;
  int32_t* d_dly = nullptr;
  long long* d_acc = nullptr;
  uint32_t* d_hits = nullptr;
  const size_t nout = (size_t)ncand * nt * nbin;
  POST_DEV(ps.alloc(&d_rec, n * sizeof(DmRec)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dc, (size_t)ncand * sizeof(DmCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dly, delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_acc, nout * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_hits, nout * sizeof(uint32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_rec, prep.rec.data(), n * sizeof(DmRec), ps.s), "upload records");
  POST_DEV(dev_h2d(d_dc, prep.dc.data(), (size_t)ncand * sizeof(DmCand), ps.s), "upload records");
  POST_DEV(dev_h2d(d_dly, delays.data(), delays.size() * sizeof(int32_t), ps.s), "upload delays");
  DmParams p = post_params<DmParams>(fil, d_rows, nrows);
  p.ncand = (int)ncand; p.cand = d_dc; p.rec = d_rec; p.delays = d_dly; p.acc = d_acc; p.hits = d_hits;
  p.ntrial = (int)par->ntrial; p.nbin = (int)par->nbin; p.tfactor = (int)par->tfactor; p.p0 = (int)prep.p0; p.np = (int)prep.np;
  p.ntile = rule.ntile; p.trun = rule.trun; p.brun = rule.brun;
  out->k[1] = rule.fastk ? 1 : 0;
  bool launched = false;
#ifndef FRBCH_NO_FAST
  if (rule.fastk) {
    long long* d_part = nullptr;
    uint32_t* d_hpart = nullptr;
    const size_t npart = nout * (size_t)rule.ntile;
    POST_DEV(ps.alloc(&d_part, npart * sizeof(long long)), "hipMalloc");
    POST_DEV(ps.alloc(&d_hpart, npart * sizeof(uint32_t)), "hipMalloc");
    p.part = d_part; p.hpart = d_hpart;
    const bool coh = prep.np == 2;
    const unsigned nbr = (unsigned)((par->nbin + rule.brun - 1) / rule.brun), ntr = (unsigned)((par->ntrial + rule.trun - 1) / rule.trun);
    const dim3 grid((unsigned)rule.ntile * nbr, ntr, ncand), block(fast::kDmThreads);
    int lrc;
    if (fil->nbits == 8) lrc = coh ? launch_lds(fast::frbch_post_dmscan_fast<1, 2>, grid, block, fast::kDmLds, ps.s, p)
                                   : launch_lds(fast::frbch_post_dmscan_fast<1, 1>, grid, block, fast::kDmLds, ps.s, p);
    else lrc = coh ? launch_lds(fast::frbch_post_dmscan_fast<2, 2>, grid, block, fast::kDmLds, ps.s, p)
                   : launch_lds(fast::frbch_post_dmscan_fast<2, 1>, grid, block, fast::kDmLds, ps.s, p);
    POST_DEV(lrc, "LDS size");
    POST_DEV(dev_check_launch(), "launch DM scan");
    hipLaunchKernelGGL(fast::frbch_post_dmscan_join, dim3((unsigned)((nout + fast::kDmThreads - 1) / fast::kDmThreads)), dim3(fast::kDmThreads), 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch DM scan join");
    launched = true;
  }
#endif
  if (!launched) {
    DEV_LAUNCH(frbch_post_dmscan, (nout + 255) / 256, 1, 256, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch DM scan");
  }
  out->acc.resize(nout);
  out->hits.resize(nout);
  POST_DEV(dev_d2h(out->acc.data(), d_acc, nout * sizeof(long long), ps.s), "download DM scan");
  POST_DEV(dev_d2h(out->hits.data(), d_hits, nout * sizeof(uint32_t), ps.s), "download DM scan");
  POST_DEV(dev_sync(ps.s), "sync");
  dm_peaks(par, pk, dms, ncand, prep.kscale.data(), prep.nused.data(), (const int64_t*)out->acc.data(), out->hits.data(), &out->cv);
  return FRBCH_OK;
}
}  // namespace

extern "C" double frbch_dm_sample_step(const frbch_fil_desc* fil) {
  if (!fil || fil->size != sizeof(frbch_fil_desc) || fil->nchan < 2 || !(fil->tsamp_s > 0) || fil->foff_mhz == 0.0) return 0.0;
  const double d = post_delay_s(fil, 1.0, fil->foff_mhz < 0 ? fil->nchan - 1 : 0);
  return d > 0.0 ? fil->tsamp_s / d : 0.0;
}

extern "C" int frbch_dmscan_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                   const frbch_burst_cand* cands, uint32_t ncand, const frbch_dmscan_params* par) try {
  PostErr e{nullptr, 0};
  int rc = dm_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  std::vector<double> dms;
  std::vector<int32_t> delays;
  if ((rc = dm_build(fil, cands, ncand, par, &dms, &delays, e)) != 0) return rc;
  return dm_plan_rule(fil, d_rows, bpar->products, delays, ncand, par).fastk ? 1 : 0;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_dmscan_peaks(const frbch_dmscan_params* par, const frbch_dmscan_peak_params* pk, const frbch_burst_cand* cands,
                                  uint32_t ncand, const int32_t* k, const uint32_t* nused, const int64_t* acc, const uint32_t* hits,
                                  double* snr, double* strc, uint32_t* width, uint32_t* bin, frbch_dmscan_result* results, char* err,
                                  size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!par || par->size != sizeof(frbch_dmscan_params)) return e.fail(FRBCH_E_ARG, "frbch_dmscan_params: wrong size");
  if (dm_bad_ntrial(*par)) return e.fail(FRBCH_E_ARG, dm_bad_ntrial(*par));
  if (par->nbin < 1 || par->nbin > kWinMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 1..1024");
  if (dm_bad_ddm(*par)) return e.fail(FRBCH_E_ARG, dm_bad_ddm(*par));
  if (!cands || ncand < 1 || ncand > kBurstMaxCand) return e.fail(FRBCH_E_ARG, "1..4096 candidates");
  if ((uint64_t)ncand * par->ntrial * par->nbin > kDmMaxOut) return e.fail(FRBCH_E_ARG, "ncand * ntrial * nbin exceeds 2^24: cut the batch or the scan");
  int rc = dm_check_peaks(par, pk, e);
  if (rc) return rc;
  if (!k || !nused || !acc || !hits) return e.fail(FRBCH_E_ARG, "null argument");
  std::vector<double> dms;
  if ((rc = dm_trials(cands, ncand, par, &dms, e)) != 0) return rc;
  DmCurves cv;
  dm_peaks(par, pk, dms, ncand, k, nused, acc, hits, &cv);
  deliver(snr, cv.snr);
  deliver(strc, cv.strc);
  deliver(width, cv.width);
  deliver(bin, cv.bin);
  deliver(results, cv.res);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dmscan_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                   const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_dmscan_params* par,
                                   const frbch_dmscan_peak_params* pk, int device, int64_t* acc, uint32_t* hits, double* snr,
                                   double* strc, frbch_dmscan_result* results, uint8_t* used, uint32_t* kernel_used, char* err,
                                   size_t err_cap) try {
  static_assert(sizeof(DmRec) == 24 && sizeof(frbch_dmscan_result) == 96 && sizeof(frbch_dmscan_params) == 24 &&
                sizeof(frbch_dmscan_peak_params) == 88 && sizeof(long long) == sizeof(int64_t), "DM scan records");
  PostErr e{err, err_cap};
  int rc = dm_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if ((rc = dm_check_peaks(par, pk, e)) != 0) return rc;
  if (!d_rows) return e.fail(FRBCH_E_ARG, "null argument");
  {
    std::vector<double> dms;                                    // (the trial DMs are refused before anything is allocated)
    if ((rc = dm_trials(cands, ncand, par, &dms, e)) != 0) return rc;
  }
  DmOut out;
  rc = burst_device_call(device, e, [&](PostScope& ps) { return dm_run(fil, d_rows, nrows, bpar, cands, ncand, flag, par, pk, ps, &out, e); });
  if (rc) return rc;
  deliver(acc, out.acc);
  deliver(hits, out.hits);
  deliver(snr, out.cv.snr);
  deliver(strc, out.cv.strc);
  deliver(results, out.cv.res);
  deliver(used, out.used);
  deliver(kernel_used, out.k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_dmscan_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                 const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_dmscan_params* par,
                                 const frbch_dmscan_peak_params* pk, int device, int64_t* acc, uint32_t* hits, double* snr,
                                 double* strc, frbch_dmscan_result* results, uint8_t* used, uint32_t* kernel_used, char* err,
                                 size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = dm_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if ((rc = dm_check_peaks(par, pk, e)) != 0) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  {
    std::vector<double> dms;
    if ((rc = dm_trials(cands, ncand, par, &dms, e)) != 0) return rc;
  }
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return frbch_dmscan_device(fil, d_rows, nrows, bpar, cands, ncand, flag, par, pk, device, acc, hits, snr, strc, results, used, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// ---------------------------------------------------------------------------------------------------------------------
// Structure of a burst: dedispersed dynamic spectrum and its two-dimensional ACF (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kAcfMaxLagF = 1024, kAcfMaxLagT = 256;
constexpr uint64_t kAcfMaxPlane = 1ull << 20, kAcfMaxCells = 1ull << 24, kAcfMaxLags = 1ull << 24, kAcfPartCap = 1ull << 30;
constexpr int32_t kAcfMaxY = 1 << 21;

int acf2_check(uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form, const PostErr& e) {
  if (n < 1 || nsub < 1) return e.fail(FRBCH_E_ARG, "at least one plane and one subband");
  if (nbin < 1 || nbin > kWinMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 1..1024");
  if ((uint64_t)nsub * nbin > kAcfMaxPlane) return e.fail(FRBCH_E_ARG, "nsub * nbin exceeds 2^20: raise ffactor or cut the window");
  if ((uint64_t)n * nsub * nbin > kAcfMaxCells) return e.fail(FRBCH_E_ARG, "ncand * nsub * nbin exceeds 2^24: cut the batch");
  if (nlagf < 1 || nlagf > std::min(nsub, kAcfMaxLagF)) return e.fail(FRBCH_E_ARG, "nlagf must be 1..min(nsub, 1024)");
  if (nlagt < 1 || nlagt > std::min(nbin, kAcfMaxLagT)) return e.fail(FRBCH_E_ARG, "nlagt must be 1..min(nbin, 256)");
  if ((uint64_t)n * nlagf * (2ull * nlagt - 1) > kAcfMaxLags) return e.fail(FRBCH_E_ARG, "ncand * nlagf * (2 nlagt - 1) exceeds 2^24: cut the batch or the lags");
  if (form > FRBCH_ACF_GENERIC) return e.fail(FRBCH_E_ARG, "form must be FRBCH_ACF_PLAN or FRBCH_ACF_GENERIC");
  return FRBCH_OK;
}

// The plan rule of the ACF stage -- the one decision behind the launches, kernel_used and frbch_acf2d_kernel's answer.  Every
// thread of the fast kernel owns 8 time lags: nrun = ceil((2 nlagt - 1) / 8) runs, nrunp = the next power of two; a workgroup
// takes dfr = min(256 / nrunp, 8, nlagf rounded up to a power of two) frequency lags.  A b line holds nbin8 + 8 nrun positions
// (nbin8 = nbin rounded up to 8) skewed by one word in eight, and the line stride bw is the next value = 9 nrunp (mod 32).  The
// slab is the largest sb with (sb nbin8 + (sb + dfr - 1) bw) words <= 64 KiB, at most nsub.  Not fast: `form` asks for the
// generic kernel, more than 65535 planes (the third grid dimension), or partials of the slabs above 2^30 bytes.  The emulator
// build has no such kernel: generic.
struct Acf2Plan { bool fastk; int sb, dfr, nrun, nrunp, bw, nslab, threads; size_t lds; };
Acf2Plan acf2_plan_rule(uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form) {
  Acf2Plan r{false, 0, 0, 0, 0, 0, 0, 0, 0};
#ifndef FRBCH_NO_FAST
  if (form == FRBCH_ACF_GENERIC || n > 65535u) return r;
  const int ndt = 2 * (int)nlagt - 1, nrun = (ndt + fast::kAcfRun - 1) / fast::kAcfRun;
  int nrunp = 1, lf = 1;
  while (nrunp < nrun) nrunp <<= 1;
  while (lf < (int)nlagf) lf <<= 1;
  const int dfr = std::min({fast::kAcfThreads / nrunp, fast::kAcfMaxDfr, lf});
  const int nbin8 = ((int)nbin + 7) & ~7, bwl = nbin8 + 8 * nrun, words = (int)(fast::kAcfLds / 4);
  int bw = bwl + bwl / 8;
  while (bw % 32 != (9 * nrunp) % 32) ++bw;
  int sb = (words - (dfr - 1) * bw) / (nbin8 + bw);
  if (sb < 1) return r;
  sb = std::min(sb, (int)nsub);
  const int nslab = ((int)nsub + sb - 1) / sb;
  if ((uint64_t)n * (uint64_t)nslab * nlagf * (uint64_t)ndt * 8ull > kAcfPartCap) return r;
  r = Acf2Plan{true, sb, dfr, nrun, nrunp, bw, nslab, std::max(64, dfr * nrunp), (size_t)(sb * nbin8 + (sb + dfr - 1) * bw) * 4};
#else
  (void)n; (void)nsub; (void)nbin; (void)nlagf; (void)nlagt; (void)form;
#endif
  return r;
}

// the launches of the stage on device planes, inside a scope; not synchronised
int acf2_launch(const int32_t* d_y, uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form,
                long long* d_A, PostScope& ps, uint32_t* kernel_used, const PostErr& e) {
  const Acf2Plan pl = acf2_plan_rule(n, nsub, nbin, nlagf, nlagt, form);
  Acf2Params p;
  memset(&p, 0, sizeof p);
  p.y = d_y; p.A = d_A; p.n = (int)n; p.nsub = (int)nsub; p.nbin = (int)nbin; p.nlagf = (int)nlagf; p.nlagt = (int)nlagt;
  p.sb = pl.sb; p.dfr = pl.dfr; p.nrun = pl.nrun; p.nrunp = pl.nrunp; p.bw = pl.bw; p.nslab = pl.nslab;
  const size_t nout = (size_t)n * nlagf * (2 * (size_t)nlagt - 1);
  if (kernel_used) *kernel_used = pl.fastk ? 1 : 0;
#ifndef FRBCH_NO_FAST
  if (pl.fastk) {
    long long* d_part = nullptr;
    POST_DEV(ps.alloc(&d_part, nout * (size_t)pl.nslab * sizeof(long long)), "hipMalloc");
    p.part = d_part;
    const dim3 grid((unsigned)pl.nslab, (unsigned)((nlagf + pl.dfr - 1) / pl.dfr), n), block((unsigned)pl.threads);
    POST_DEV(launch_lds(fast::frbch_post_acf2d_fast, grid, block, pl.lds, ps.s, p), "LDS size");
    POST_DEV(dev_check_launch(), "launch ACF");
    hipLaunchKernelGGL(fast::frbch_post_acf2d_join, dim3((unsigned)((nout + fast::kAcfThreads - 1) / fast::kAcfThreads)), dim3(fast::kAcfThreads), 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch ACF join");
    return FRBCH_OK;
  }
#endif
  DEV_LAUNCH(frbch_post_acf2d, (nout + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch ACF");
  return FRBCH_OK;
}

int acf_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_burst_params* bpar, const frbch_burst_cand* cands,
              uint32_t ncand, const frbch_acf_params* par, const PostErr& e) {
  int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if ((rc = window_check(fil, par, "the burst ACF", "frbch_acf_params", {nullptr, nullptr, &frbch_acf_params::ffactor}, e)) != 0) return rc;
  return acf2_check(ncand, fil->nchan / par->ffactor, par->nbin, par->nlagf, par->nlagt, FRBCH_ACF_PLAN, e);
}

int acf_check_fit(const frbch_acf_fit_params* fp, const PostErr& e) {
  if (!fp || fp->size != sizeof(frbch_acf_fit_params)) return e.fail(FRBCH_E_ARG, "frbch_acf_fit_params: wrong size");
  if (!(fp->fit_frac > 0.0) || !(fp->fit_frac < 1.0)) return e.fail(FRBCH_E_ARG, "fit_frac must lie inside (0, 1)");
  return FRBCH_OK;
}

// the delays of the candidates at their own DM, [ncand][nchan]: the DM scan's table at one trial
int acf_delays(const frbch_fil_desc* fil, const frbch_burst_cand* cands, uint32_t ncand, const frbch_acf_params* par,
               std::vector<int32_t>* delays, const PostErr& e) {
  const frbch_dmscan_params one{sizeof(frbch_dmscan_params), 1, par->nbin, par->tfactor, 0.0};
  std::vector<double> dms;
  return dm_build(fil, cands, ncand, &one, &dms, delays, e);
}

// The plan rule of the dynamic spectrum -- the one decision behind its launches, kernel_used[1] and frbch_burstacf_kernel's
// answer.  The fast kernel wants what the fast DM scan kernel wants at one trial (the layout of the fast burst-sums kernel, bins
// of at most kDmMaxT rows, a bin that fits the stage: dm_stage_brun with ntrial = trun = 1) and an
// ffactor it can reduce: a power of two of at most the CT channels of a tile (shuffles over ffactor lanes, gl = ffactor), or a
// multiple of CT (shuffles over the tile, gl = CT, and a join over tps = ffactor / CT tiles, whose partials stay within 2^30
// bytes).  The emulator build has no such kernel: generic.
struct DynPlan { bool fastk; int brun, ntile, gl, tps; };
DynPlan dyn_plan_rule(const frbch_fil_desc* fil, const void* d_rows, uint32_t products, const std::vector<int32_t>& delays,
                      uint32_t ncand, const frbch_acf_params* par) {
  DynPlan r{false, 0, 0, 0, 0};
#ifndef FRBCH_NO_FAST
  if (!burst_fast_layout(fil, d_rows) || par->tfactor > (uint32_t)fast::kDmMaxT) return r;
  const uint32_t ct = 64u / (uint32_t)(fil->nbits / 8), ntile = fil->nchan / ct, ff = par->ffactor;
  const bool shuffle = (ff & (ff - 1)) == 0 && ff <= ct, join = ff > ct && ff % ct == 0;
  if (!shuffle && !join) return r;
  if (join && (uint64_t)ncand * ntile * par->nbin * 12ull > kDmPartCap) return r;
  const int brun = dm_stage_brun(tile_scan(fil, delays), products, ncand, 1, 1, par->nbin, par->tfactor);     // the DM scan's stage at one trial
  if (!brun) return r;
  r = DynPlan{true, brun, (int)ntile, (int)std::min(ff, ct), join ? (int)(ff / ct) : 0};
#else
  (void)fil; (void)d_rows; (void)products; (void)delays; (void)ncand; (void)par;
#endif
  return r;
}

// half-width at half maximum of a cut v[0 .. nl - 1] whose lag 0 is left out (the header's rule) -> x, *fitted
double acf_half_width(const double* v, uint32_t nl, uint32_t* fitted) {
  POST_NO_CONTRACT
  *fitted = 0;
  if (nl < 2 || !(v[1] > 0.0)) return 0.0;
  const double h = v[1] / 2.0;
  for (uint32_t d = 2; d < nl; ++d)
    if (v[d] < h) {
      const double a = v[d - 1] - h, b = v[d - 1] - v[d];
      const double q = a / b;
      *fitted = 1;
      return (double)(d - 1) + q;
    }
  return (double)(nl - 1);
}

// step 4 of the header; every check has been made.  norm may be NULL.
void acf_fit(const frbch_fil_desc* fil, const frbch_acf_params* par, double fit_frac, uint32_t ncand, const int32_t* k,
             const uint32_t* r, const uint32_t* nused, const uint32_t* ncomplete, const int64_t* A, const uint32_t* P, double* norm,
             frbch_acf_result* res) {
  POST_NO_CONTRACT
  const uint32_t nlf = par->nlagf, nlt = par->nlagt, ndt = 2 * nlt - 1, L = nlt - 1;
  const size_t per = (size_t)nlf * ndt;
  const double tu = (double)par->tfactor * fil->tsamp_s;
  const double unit_t = tu * 1000.0;
  const double unit_f = (double)par->ffactor * fil->foff_mhz;
  std::vector<double> own(per), cut(std::max(nlf, nlt));
  memset((void*)res, 0, (size_t)ncand * sizeof(frbch_acf_result));
  for (uint32_t i = 0; i < ncand; ++i) {
    double* nm = norm ? norm + (size_t)i * per : own.data();
    if (!nused[i]) {
      std::fill(nm, nm + per, 0.0);
      continue;
    }
    frbch_acf_result& R = res[i];
    R.k = k[i]; R.r = r[i]; R.nused = nused[i]; R.ncomplete = ncomplete[i];
    const double q = ldexp(1.0, -2 * (k[i] - (int32_t)r[i]));
    for (size_t l = 0; l < per; ++l) {
      const uint32_t pv = P[(size_t)i * per + l];
      const double a = (double)A[(size_t)i * per + l] * q;
      nm[l] = pv ? a / (double)pv : 0.0;
    }
    for (uint32_t d = 0; d < nlf; ++d) cut[d] = nm[(size_t)d * ndt + L];
    const double xf = acf_half_width(cut.data(), nlf, &R.fitted_f);
    R.width_f_mhz = xf * fabs(unit_f);
    for (uint32_t d = 0; d < nlt; ++d) cut[d] = nm[L + d];
    const double xt = acf_half_width(cut.data(), nlt, &R.fitted_t);
    R.width_t_ms = xt * unit_t;
    bool any = false;
    double ref = 0.0;
    for (uint32_t df = 0; df < nlf; ++df)
      for (uint32_t x = 0; x < ndt; ++x) {
        if (df == 0 && x == L) continue;
        const double v = nm[(size_t)df * ndt + x];
        if (!any || v > ref) { ref = v; any = true; }
      }
    R.ref = ref;
    if (!(ref > 0.0)) continue;
    const double thr = fit_frac * ref;
    double mff = 0.0, mtf = 0.0, mtt = 0.0;
    for (uint32_t df = 0; df < nlf; ++df)
      for (uint32_t x = 0; x < ndt; ++x) {
        const long long dt = (long long)x - (long long)L;
        if (df == 0 && dt <= 0) continue;
        const double v = nm[(size_t)df * ndt + x];
        if (!(v >= thr)) continue;
        const double tf = v * (double)((long long)df * (long long)df), tx = v * (double)((long long)df * dt), tt = v * (double)(dt * dt);
        mff = mff + tf;
        mtf = mtf + tx;
        mtt = mtt + tt;
      }
    R.mff = 2.0 * mff; R.mtf = 2.0 * mtf; R.mtt = 2.0 * mtt;
    if (!(R.mff > 0.0)) continue;
    const double slope = R.mtf / R.mff;
    const double ms = slope * unit_t;
    R.dt_df = ms / unit_f;
    R.drift = R.dt_df != 0.0 ? 1.0 / R.dt_df : 0.0;
    R.fitted_d = 1;
  }
}

struct AcfOut {
  std::vector<long long> Y, A;
  std::vector<uint32_t> yhits, P;
  std::vector<uint8_t> used;
  std::vector<frbch_acf_result> res;
  uint32_t k[3] = {0, 0, 0};
};

// Steps 1 and 2 of the header inside a scope, launched and not synchronised: the preparation (synchronised), the dynamic
// spectrum, the row maxima, the shift, the quantised plane and the 0 / 1 plane of the complete cells.  Only nbin, tfactor and
// ffactor of `par` are looked at.  The burst ACF and the scattering fit share it.
struct DynOut {
  DmPrep prep;
  std::vector<uint8_t> used;            // [ncand][nchan]
  std::vector<uint32_t> nused_s;        // [ncand][nsub]
  long long* d_Y = nullptr;             // [ncand][nsub][nbin], the scope's
  uint32_t* d_hits = nullptr;
  int32_t *d_shift = nullptr, *d_y = nullptr, *d_mask = nullptr;
};
int dyn_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
            const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par, PostScope& ps,
            DynOut* out, uint32_t* kernel_used, const PostErr& e) {
  const size_t nchan = fil->nchan, n = (size_t)ncand * nchan, nbin = par->nbin, nsub = nchan / par->ffactor;
  const size_t ncell = (size_t)ncand * nsub * nbin;
  std::vector<int32_t> delays;
  int rc = acf_delays(fil, cands, ncand, par, &delays, e);
  if (rc) return rc;
  const DynPlan rule = dyn_plan_rule(fil, d_rows, bpar->products, delays, ncand, par);
  DmPrep& prep = out->prep;
  if ((rc = dm_prepare(fil, d_rows, nrows, bpar, cands, ncand, flag, par->nbin, par->tfactor, ps, &prep, &kernel_used[0], e)) != 0) return rc;
  out->used.swap(prep.used);
  std::vector<uint32_t>& nused_s = out->nused_s;
  nused_s.assign((size_t)ncand * nsub, 0);
  for (size_t i = 0; i < ncand; ++i)
    for (size_t c = 0; c < nchan; ++c) nused_s[i * nsub + c / par->ffactor] += out->used[i * nchan + c];

  DmRec* d_rec = nullptr;
  DmCand* d_dc = nullptr;
  int32_t *d_dly = nullptr, *d_shift = nullptr, *d_y = nullptr, *d_mask = nullptr;
  uint32_t *d_nu = nullptr, *d_hits = nullptr;
  long long *d_Y = nullptr, *d_rowmax = nullptr;
  POST_DEV(ps.alloc(&d_rec, n * sizeof(DmRec)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dc, (size_t)ncand * sizeof(DmCand)), "hipMalloc");
  POST_DEV(ps.alloc(&d_dly, delays.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_nu, nused_s.size() * sizeof(uint32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_Y, ncell * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_hits, ncell * sizeof(uint32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_rowmax, (size_t)ncand * nsub * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_shift, (size_t)ncand * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_y, ncell * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_mask, ncell * sizeof(int32_t)), "hipMalloc");
  POST_DEV(dev_h2d(d_rec, prep.rec.data(), n * sizeof(DmRec), ps.s), "upload records");
  POST_DEV(dev_h2d(d_dc, prep.dc.data(), (size_t)ncand * sizeof(DmCand), ps.s), "upload records");
  POST_DEV(dev_h2d(d_dly, delays.data(), delays.size() * sizeof(int32_t), ps.s), "upload delays");
  POST_DEV(dev_h2d(d_nu, nused_s.data(), nused_s.size() * sizeof(uint32_t), ps.s), "upload records");
  DynParams p = post_params<DynParams>(fil, d_rows, nrows);
  p.ncand = (int)ncand; p.cand = d_dc; p.rec = d_rec; p.delays = d_dly; p.nused_s = d_nu; p.Y = d_Y; p.yhits = d_hits;
  p.rowmax = d_rowmax; p.shift = d_shift; p.y = d_y; p.mask = d_mask;
  p.nsub = (int)nsub; p.nbin = (int)par->nbin; p.tfactor = (int)par->tfactor; p.ffactor = (int)par->ffactor;
  p.p0 = (int)prep.p0; p.np = (int)prep.np; p.ntile = rule.ntile; p.brun = rule.brun; p.gl = rule.gl;
  kernel_used[1] = rule.fastk ? 1 : 0;
  bool launched = false;
#ifndef FRBCH_NO_FAST
  if (rule.fastk) {
    long long* d_part = nullptr;
    uint32_t* d_hpart = nullptr;
    if (rule.tps) {
      const size_t npart = (size_t)ncand * rule.ntile * nbin;
      POST_DEV(ps.alloc(&d_part, npart * sizeof(long long)), "hipMalloc");
      POST_DEV(ps.alloc(&d_hpart, npart * sizeof(uint32_t)), "hipMalloc");
      p.part = d_part; p.hpart = d_hpart;
    }
    const bool coh = prep.np == 2;
    const unsigned nbr = (unsigned)((par->nbin + rule.brun - 1) / rule.brun);
    const dim3 grid((unsigned)rule.ntile * nbr, 1, ncand), block(fast::kDmThreads);
    int lrc;
    if (fil->nbits == 8) lrc = coh ? launch_lds(fast::frbch_post_dynspec_fast<1, 2>, grid, block, fast::kDmLds, ps.s, p)
                                   : launch_lds(fast::frbch_post_dynspec_fast<1, 1>, grid, block, fast::kDmLds, ps.s, p);
    else lrc = coh ? launch_lds(fast::frbch_post_dynspec_fast<2, 2>, grid, block, fast::kDmLds, ps.s, p)
                   : launch_lds(fast::frbch_post_dynspec_fast<2, 1>, grid, block, fast::kDmLds, ps.s, p);
    POST_DEV(lrc, "LDS size");
    POST_DEV(dev_check_launch(), "launch dynamic spectrum");
    if (rule.tps) {
      hipLaunchKernelGGL(fast::frbch_post_dynspec_join, dim3((unsigned)((ncell + fast::kDmThreads - 1) / fast::kDmThreads)), dim3(fast::kDmThreads), 0, ps.s, p, rule.tps);
      POST_DEV(dev_check_launch(), "launch dynamic spectrum join");
    }
    launched = true;
  }
#endif
  if (!launched) {
    DEV_LAUNCH(frbch_post_dynspec, (ncell + 255) / 256, 1, 256, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch dynamic spectrum");
  }
  DEV_LAUNCH(frbch_post_acf_rowmax, ((size_t)ncand * nsub + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch row maxima");
  DEV_LAUNCH(frbch_post_acf_shift, (ncand + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch scale");
  DEV_LAUNCH(frbch_post_acf_quant, (ncell + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch quantisation");
  out->d_Y = d_Y; out->d_hits = d_hits; out->d_shift = d_shift; out->d_y = d_y; out->d_mask = d_mask;
  return FRBCH_OK;
}

// everything of a call inside its scope: the preparation, the dynamic spectrum, the quantised plane, the ACFs, the fit
int acf_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
            const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par,
            const frbch_acf_fit_params* fp, PostScope& ps, AcfOut* out, const PostErr& e) {
  const size_t nbin = par->nbin, nsub = fil->nchan / par->ffactor;
  const size_t ncell = (size_t)ncand * nsub * nbin, ndt = 2 * (size_t)par->nlagt - 1, nlag = (size_t)ncand * par->nlagf * ndt;
  DynOut dyn;
  int rc = dyn_run(fil, d_rows, nrows, bpar, cands, ncand, flag, par, ps, &dyn, out->k, e);
  if (rc) return rc;
  out->used.swap(dyn.used);
  long long* d_A = nullptr;
  POST_DEV(ps.alloc(&d_A, nlag * sizeof(long long)), "hipMalloc");
  if ((rc = acf2_launch(dyn.d_y, ncand, (uint32_t)nsub, par->nbin, par->nlagf, par->nlagt, FRBCH_ACF_PLAN, d_A, ps, &out->k[2], e)) != 0) return rc;
  std::vector<int32_t> shift(ncand);
  out->Y.resize(ncell);
  out->yhits.resize(ncell);
  out->A.resize(nlag);
  POST_DEV(dev_d2h(out->Y.data(), dyn.d_Y, ncell * sizeof(long long), ps.s), "download dynamic spectrum");
  POST_DEV(dev_d2h(out->yhits.data(), dyn.d_hits, ncell * sizeof(uint32_t), ps.s), "download dynamic spectrum");
  POST_DEV(dev_d2h(shift.data(), dyn.d_shift, (size_t)ncand * sizeof(int32_t), ps.s), "download scale");
  POST_DEV(dev_d2h(out->A.data(), d_A, nlag * sizeof(long long), ps.s), "download ACF");
  POST_DEV(dev_sync(ps.s), "sync");

  // the complete cells of every candidate; all of them complete: P in closed form, else the same kernel on the 0 / 1 plane
  std::vector<uint32_t> ncomplete(ncand, 0), ushift(ncand);
  for (size_t i = 0; i < ncand; ++i) {
    ushift[i] = (uint32_t)shift[i];
    for (size_t s = 0; s < nsub; ++s) {
      const uint32_t nu = dyn.nused_s[i * nsub + s];
      if (!nu) continue;
      const uint32_t* h = out->yhits.data() + (i * nsub + s) * nbin;
      for (size_t j = 0; j < nbin; ++j) ncomplete[i] += h[j] == par->tfactor * nu ? 1u : 0u;
    }
  }
  out->P.resize(nlag);
  bool all = true;
  for (size_t i = 0; i < ncand; ++i) all = all && ncomplete[i] == nsub * nbin;
  if (all) {
    for (size_t i = 0; i < ncand; ++i)
      for (size_t df = 0; df < par->nlagf; ++df)
        for (size_t x = 0; x < ndt; ++x) {
          const size_t adt = x >= par->nlagt - 1 ? x - (par->nlagt - 1) : (par->nlagt - 1) - x;
          out->P[(i * par->nlagf + df) * ndt + x] = (uint32_t)((nsub - df) * (nbin - adt));
        }
  } else {
    std::vector<long long> pairs(nlag);
    uint32_t kp = 0;
    if ((rc = acf2_launch(dyn.d_mask, ncand, (uint32_t)nsub, par->nbin, par->nlagf, par->nlagt, FRBCH_ACF_PLAN, d_A, ps, &kp, e)) != 0) return rc;
    POST_DEV(dev_d2h(pairs.data(), d_A, nlag * sizeof(long long), ps.s), "download pair counts");
    POST_DEV(dev_sync(ps.s), "sync");
    for (size_t l = 0; l < nlag; ++l) out->P[l] = (uint32_t)pairs[l];
  }
  out->res.resize(ncand);
  acf_fit(fil, par, fp->fit_frac, ncand, dyn.prep.kscale.data(), ushift.data(), dyn.prep.nused.data(), ncomplete.data(),
          (const int64_t*)out->A.data(), out->P.data(), nullptr, out->res.data());
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_acf2d_kernel(uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt, uint32_t form) try {
  const int rc = acf2_check(n, nsub, nbin, nlagf, nlagt, form, PostErr{nullptr, 0});
  return rc ? rc : (acf2_plan_rule(n, nsub, nbin, nlagf, nlagt, form).fastk ? 1 : 0);
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_acf2d_device(const int32_t* d_y, uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt,
                                  uint32_t form, int device, int64_t* d_A, uint32_t* kernel_used, char* err, size_t err_cap) try {
  static_assert(sizeof(frbch_acf_params) == 32 && sizeof(frbch_acf_fit_params) == 16 && sizeof(frbch_acf_result) == 96, "ACF records");
  PostErr e{err, err_cap};
  int rc = acf2_check(n, nsub, nbin, nlagf, nlagt, form, e);
  if (rc) return rc;
  if (!d_y || !d_A) return e.fail(FRBCH_E_ARG, "null argument");
  uint32_t k[1] = {0};
  rc = burst_device_call(device, e, [&](PostScope& ps) {
    const int rc = acf2_launch(d_y, n, nsub, nbin, nlagf, nlagt, form, (long long*)d_A, ps, k, e);
    if (rc) return rc;
    POST_DEV(dev_sync(ps.s), "sync");
    return (int)FRBCH_OK;
  });
  if (rc) return rc;
  deliver(kernel_used, k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_acf2d_host(const int32_t* y, uint32_t n, uint32_t nsub, uint32_t nbin, uint32_t nlagf, uint32_t nlagt,
                                uint32_t form, int device, int64_t* A, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = acf2_check(n, nsub, nbin, nlagf, nlagt, form, e);
  if (rc) return rc;
  if (!y || !A) return e.fail(FRBCH_E_ARG, "null argument");
  const size_t ncell = (size_t)n * nsub * nbin, nlag = (size_t)n * nlagf * (2 * (size_t)nlagt - 1);
  for (size_t i = 0; i < ncell; ++i)
    if (y[i] > kAcfMaxY || y[i] < -kAcfMaxY) return e.fail(FRBCH_E_ARG, "a value of the plane lies outside -2^21 .. 2^21: the int64 sums are not safe");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  int32_t* d_y = hs.in(y, ncell * sizeof(int32_t));
  int64_t* d_A = hs.out(A, nlag * sizeof(int64_t));
  return hs.run(e, "device memory for the plane", "upload plane", "download ACF", [&]() {
    return frbch_acf2d_device(d_y, n, nsub, nbin, nlagf, nlagt, form, device, d_A, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstacf_fit(const frbch_fil_desc* fil, const frbch_acf_params* par, const frbch_acf_fit_params* fp, uint32_t ncand,
                                  const int32_t* k, const uint32_t* r, const uint32_t* nused, const uint32_t* ncomplete, const int64_t* A,
                                  const uint32_t* P, double* norm, frbch_acf_result* results, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!fil || fil->size != sizeof(frbch_fil_desc) || fil->nchan < 1 || !(fil->tsamp_s > 0) || fil->foff_mhz == 0.0) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size, or bad nchan / tsamp / foff");
  if (!par || par->size != sizeof(frbch_acf_params)) return e.fail(FRBCH_E_ARG, "frbch_acf_params: wrong size");
  if (par->tfactor < 1 || par->tfactor > kWinMaxT) return e.fail(FRBCH_E_ARG, "tfactor must be 1..512");
  if (par->ffactor < 1 || par->ffactor > fil->nchan || fil->nchan % par->ffactor) return e.fail(FRBCH_E_ARG, "ffactor must be 1..nchan and divide nchan");
  int rc = acf2_check(ncand, fil->nchan / par->ffactor, par->nbin, par->nlagf, par->nlagt, FRBCH_ACF_PLAN, e);
  if (rc) return rc;
  if ((rc = acf_check_fit(fp, e)) != 0) return rc;
  if (!k || !r || !nused || !ncomplete || !A || !P) return e.fail(FRBCH_E_ARG, "null argument");
  for (uint32_t i = 0; i < ncand; ++i)
    if (r[i] > 40 || k[i] < -1024 || k[i] > 1024) return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": k or r out of range");
  std::vector<frbch_acf_result> res(ncand);
  std::vector<double> nm(norm ? (size_t)ncand * par->nlagf * (2 * (size_t)par->nlagt - 1) : 0);
  acf_fit(fil, par, fp->fit_frac, ncand, k, r, nused, ncomplete, A, P, norm ? nm.data() : nullptr, res.data());
  deliver(norm, nm);
  deliver(results, res);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstacf_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                     const frbch_burst_cand* cands, uint32_t ncand, const frbch_acf_params* par, uint32_t* kernel_used) try {
  PostErr e{nullptr, 0};
  int rc = acf_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  std::vector<int32_t> delays;
  if ((rc = acf_delays(fil, cands, ncand, par, &delays, e)) != 0) return rc;
  if (kernel_used) {
    kernel_used[0] = burst_fast_layout(fil, d_rows) ? 1 : 0;
    kernel_used[1] = dyn_plan_rule(fil, d_rows, bpar->products, delays, ncand, par).fastk ? 1 : 0;
    kernel_used[2] = acf2_plan_rule(ncand, fil->nchan / par->ffactor, par->nbin, par->nlagf, par->nlagt, FRBCH_ACF_PLAN).fastk ? 1 : 0;
  }
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_burstacf_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                     const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par,
                                     const frbch_acf_fit_params* fp, int device, int64_t* Y, uint32_t* yhits, int64_t* A, uint32_t* P,
                                     frbch_acf_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = acf_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if ((rc = acf_check_fit(fp, e)) != 0) return rc;
  if (!d_rows) return e.fail(FRBCH_E_ARG, "null argument");
  AcfOut out;
  rc = burst_device_call(device, e, [&](PostScope& ps) { return acf_run(fil, d_rows, nrows, bpar, cands, ncand, flag, par, fp, ps, &out, e); });
  if (rc) return rc;
  deliver(Y, out.Y);
  deliver(yhits, out.yhits);
  deliver(A, out.A);
  deliver(P, out.P);
  deliver(results, out.res);
  deliver(used, out.used);
  deliver(kernel_used, out.k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstacf_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                   const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_acf_params* par,
                                   const frbch_acf_fit_params* fp, int device, int64_t* Y, uint32_t* yhits, int64_t* A, uint32_t* P,
                                   frbch_acf_result* results, uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = acf_check(fil, nrows, bpar, cands, ncand, par, e);
  if (rc) return rc;
  if ((rc = acf_check_fit(fp, e)) != 0) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return frbch_burstacf_device(fil, d_rows, nrows, bpar, cands, ncand, flag, par, fp, device, Y, yhits, A, P, results, used, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// ---------------------------------------------------------------------------------------------------------------------
// Scattering of a burst: a bank of scattered Gaussians per subband, tau(nu) across the band (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kTbMaxTap = 1024, kTbMaxTemp = 4096, kScatMaxAlpha = 32;
constexpr uint64_t kTbMaxCells = 1ull << 24, kTbMaxOut = 1ull << 24;
constexpr int32_t kTbMaxY = 1 << 21, kTbMaxP = 1 << 30;

int tbank_check(uint32_t n, const frbch_tbank_shape* sh, uint32_t form, const PostErr& e) {
  if (!sh || sh->size != sizeof(frbch_tbank_shape)) return e.fail(FRBCH_E_ARG, "frbch_tbank_shape: wrong size");
  if (n < 1 || sh->nsub < 1) return e.fail(FRBCH_E_ARG, "at least one plane and one subband");
  if (sh->nbin < 1 || sh->nbin > kWinMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 1..1024");
  if (sh->ntap < 1 || sh->ntap > kTbMaxTap) return e.fail(FRBCH_E_ARG, "ntap must be 1..1024");
  if (sh->lead >= sh->ntap) return e.fail(FRBCH_E_ARG, "lead must lie below ntap");
  if (sh->ntemp < 1 || sh->ntemp > kTbMaxTemp) return e.fail(FRBCH_E_ARG, "1..4096 templates");
  if (sh->nshift < 1 || sh->shift0 > sh->nbin || sh->nshift > sh->nbin - sh->shift0) return e.fail(FRBCH_E_ARG, "nshift must be at least 1 and shift0 + nshift at most nbin");
  if ((uint64_t)n * sh->nsub * sh->nbin > kTbMaxCells) return e.fail(FRBCH_E_ARG, "n * nsub * nbin exceeds 2^24: cut the batch");
  if ((uint64_t)n * sh->nsub * sh->ntemp * sh->nshift > kTbMaxOut) return e.fail(FRBCH_E_ARG, "n * nsub * templates * nshift exceeds 2^24: cut the batch, the bank or the shifts");
  if (form > FRBCH_TBANK_GENERIC) return e.fail(FRBCH_E_ARG, "form must be FRBCH_TBANK_PLAN or FRBCH_TBANK_GENERIC");
  return FRBCH_OK;
}

// The plan rule of the template-bank stage -- the one decision behind the launches, kernel_used and frbch_tbank_kernel's
// answer.  Every thread of the fast kernel owns 8 shifts: nrun = ceil(nshift / 8) runs, nrunp = the next power of two; a
// workgroup takes sw = min(max(1, 64 / nrunp), 8, nsub rounded up to a power of two) subbands, so that sw nrunp lanes -- a whole
// wave where the shape allows -- share a template.  A line holds 8 nrun + ntap8 positions (ntap8 = ntap rounded up to 8) skewed
// by one word in eight, and the line stride lw is the next value = 9 nrunp (mod 32).  sw is halved while the lines leave no room
// for one template in 64 KiB (sw = 1 always does); the templates are cut into the fewest runs that fit, of equal length kr.
// Not fast: `form` asks for the generic kernel, or more than 65535 planes (the third grid dimension).  The emulator build
// has no such kernel: generic.
struct TbankPlan { bool fastk; int sw, kr, nrun, nrunp, lw, ntap8; size_t lds; };
TbankPlan tbank_plan_rule(uint32_t n, const frbch_tbank_shape* sh, uint32_t form) {
  TbankPlan r{false, 0, 0, 0, 0, 0, 0, 0};
#ifndef FRBCH_NO_FAST
  if (form == FRBCH_TBANK_GENERIC || n > 65535u) return r;
  const int nrun = ((int)sh->nshift + fast::kTbRun - 1) / fast::kTbRun, ntap8 = ((int)sh->ntap + 7) & ~7;
  int nrunp = 1, ls = 1;
  while (nrunp < nrun) nrunp <<= 1;
  while (ls < (int)sh->nsub) ls <<= 1;
  int sw = std::min({std::max(1, 64 / nrunp), fast::kTbMaxSw, ls});
  const int lwl = 8 * nrun + ntap8, words = (int)(fast::kTbLds / 4);
  int lw = lwl + lwl / 8;
  while (lw % 32 != (9 * nrunp) % 32) ++lw;
  while (sw > 1 && words - sw * lw < ntap8) sw >>= 1;
  const int krmax = (words - sw * lw) / ntap8;
  if (krmax < 1) return r;
  const int nkr = ((int)sh->ntemp + krmax - 1) / krmax, kr = ((int)sh->ntemp + nkr - 1) / nkr;
  r = TbankPlan{true, sw, kr, nrun, nrunp, lw, ntap8, (size_t)(kr * ntap8 + sw * lw) * 4};
#else
  (void)n; (void)sh; (void)form;
#endif
  return r;
}

// the launch of the stage on device planes, inside a scope; not synchronised
int tbank_launch(const int32_t* d_y, const int32_t* d_P, uint32_t n, const frbch_tbank_shape* sh, uint32_t form, long long* d_C,
                 PostScope& ps, uint32_t* kernel_used, const PostErr& e) {
  const TbankPlan pl = tbank_plan_rule(n, sh, form);
  TbankParams p;
  memset(&p, 0, sizeof p);
  p.y = d_y; p.P = d_P; p.C = d_C; p.n = (int)n; p.nsub = (int)sh->nsub; p.nbin = (int)sh->nbin; p.ntemp = (int)sh->ntemp;
  p.ntap = (int)sh->ntap; p.lead = (int)sh->lead; p.shift0 = (int)sh->shift0; p.nshift = (int)sh->nshift;
  p.sw = pl.sw; p.kr = pl.kr; p.nrun = pl.nrun; p.nrunp = pl.nrunp; p.lw = pl.lw; p.ntap8 = pl.ntap8;
  if (kernel_used) *kernel_used = pl.fastk ? 1 : 0;
#ifndef FRBCH_NO_FAST
  if (pl.fastk) {
    const dim3 grid((unsigned)((sh->nsub + pl.sw - 1) / pl.sw), (unsigned)((sh->ntemp + pl.kr - 1) / pl.kr), n), block(fast::kTbThreads);
    POST_DEV(launch_lds(fast::frbch_post_tbank_fast, grid, block, pl.lds, ps.s, p), "LDS size");
    POST_DEV(dev_check_launch(), "launch template bank");
    return FRBCH_OK;
  }
#endif
  const size_t nout = (size_t)n * sh->nsub * sh->ntemp * sh->nshift;
  DEV_LAUNCH(frbch_post_tbank, (nout + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch template bank");
  return FRBCH_OK;
}

int scat_check_bank(const frbch_scat_bank_params* bp, const PostErr& e) {
  if (!bp || bp->size != sizeof(frbch_scat_bank_params)) return e.fail(FRBCH_E_ARG, "frbch_scat_bank_params: wrong size");
  if (bp->ntap < 1 || bp->ntap > kTbMaxTap) return e.fail(FRBCH_E_ARG, "ntap must be 1..1024");
  if (bp->lead >= bp->ntap) return e.fail(FRBCH_E_ARG, "lead must lie below ntap");
  if (bp->nsig < 1 || bp->ntau < 1 || (uint64_t)bp->nsig * bp->ntau > kTbMaxTemp) return e.fail(FRBCH_E_ARG, "nsig * ntau must be 1..4096 templates");
  if (!rm_finite(bp->sigma0) || !rm_finite(bp->rsig) || !rm_finite(bp->tau0) || !rm_finite(bp->rtau)) return e.fail(FRBCH_E_ARG, "the grid of the bank must be finite");
  if (!(bp->sigma0 >= 0.25) || !(bp->tau0 >= 0.25)) return e.fail(FRBCH_E_ARG, "sigma0 and tau0 must be at least 0.25 bins");
  if (!(bp->rsig > 1.0) || !(bp->rtau > 1.0)) return e.fail(FRBCH_E_ARG, "rsig and rtau must be above 1");
  double s = bp->sigma0, t = bp->tau0;
  for (uint32_t a = 1; a < bp->nsig; ++a) s = s * bp->rsig;
  for (uint32_t b = 1; b < bp->ntau; ++b) t = t * bp->rtau;
  if (!rm_finite(s) || !rm_finite(t) || !rm_finite(s * s)) return e.fail(FRBCH_E_ARG, "the grid of the bank must be finite");
  return FRBCH_OK;
}

// the bank of the header; every check has been made
struct ScatBank {
  std::vector<int32_t> p, psq;          // [K][ntap]
  std::vector<int64_t> s1, cum;         // [K], [K][ntap + 1]
  std::vector<double> tail, sigma, tau; // [K], [nsig], [ntau]
};
void scat_bank(const frbch_scat_bank_params* bp, ScatBank* out) {
  POST_NO_CONTRACT
  const size_t ntap = bp->ntap, nsig = bp->nsig, ntau = bp->ntau, K = nsig * ntau;
  out->p.assign(K * ntap, 0); out->psq.assign(K * ntap, 0); out->s1.assign(K, 0); out->cum.assign(K * (ntap + 1), 0);
  out->tail.assign(K, 0.0); out->sigma.resize(nsig); out->tau.resize(ntau);
  for (size_t a = 0; a < nsig; ++a) out->sigma[a] = a ? out->sigma[a - 1] * bp->rsig : bp->sigma0;
  for (size_t b = 0; b < ntau; ++b) out->tau[b] = b ? out->tau[b - 1] * bp->rtau : bp->tau0;
  std::vector<double> g(ntap), ex(ntap), f(ntap);
  for (size_t a = 0; a < nsig; ++a) {
    const double sg = out->sigma[a];
    const double den = 2.0 * (sg * sg);
    for (size_t j = 0; j < ntap; ++j) {
      const double d = (double)((long long)j - (long long)bp->lead);
      const double dd = d * d;
      g[j] = exp(-dd / den);
    }
    for (size_t b = 0; b < ntau; ++b) {
      const size_t k = a * ntau + b;
      const double tau = out->tau[b];
      for (size_t n = 0; n < ntap; ++n) ex[n] = exp(-(double)n / tau);
      double fmax = 0.0;
      for (size_t m = 0; m < ntap; ++m) {
        double acc = 0.0;
        for (size_t n = 0; n <= m; ++n) {
          const double t = g[m - n] * ex[n];
          acc = acc + t;
        }
        f[m] = acc;
        if (acc > fmax) fmax = acc;
      }
      int64_t s1 = 0, c = 0;
      for (size_t m = 0; m < ntap; ++m) {
        const double u = f[m] / fmax;
        const int32_t pv = (int32_t)rint(u * 32768.0);
        out->p[k * ntap + m] = pv;
        out->psq[k * ntap + m] = pv * pv;
        s1 += pv;
        out->cum[k * (ntap + 1) + m] = c;
        c += (int64_t)pv * pv;
      }
      out->cum[k * (ntap + 1) + ntap] = c;
      out->s1[k] = s1;
      out->tail[k] = f[ntap - 1] / fmax;
    }
  }
}

int scat_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_burst_params* bpar, const frbch_burst_cand* cands,
               uint32_t ncand, const frbch_scat_params* par, const frbch_scat_bank_params* bp, frbch_acf_params* apar,
               frbch_tbank_shape* sh, const PostErr& e) {
  int rc = burst_check(fil, nrows, bpar, cands, ncand, e);
  if (rc) return rc;
  if ((rc = window_check(fil, par, "the scattering fit", "frbch_scat_params", {nullptr, nullptr, &frbch_scat_params::ffactor}, e)) != 0) return rc;
  if ((rc = scat_check_bank(bp, e)) != 0) return rc;
  *apar = frbch_acf_params{sizeof(frbch_acf_params), par->nbin, par->tfactor, par->ffactor, 1, 1, {0, 0}};
  *sh = frbch_tbank_shape{sizeof(frbch_tbank_shape), fil->nchan / par->ffactor, par->nbin, bp->nsig * bp->ntau, bp->ntap, bp->lead, par->shift0, par->nshift};
  return tbank_check(ncand, sh, FRBCH_TBANK_PLAN, e);
}

int scat_check_fit(const frbch_scat_fit_params* fp, const PostErr& e) {
  if (!fp || fp->size != sizeof(frbch_scat_fit_params)) return e.fail(FRBCH_E_ARG, "frbch_scat_fit_params: wrong size");
  if (fp->nalpha < 1 || fp->nalpha > kScatMaxAlpha) return e.fail(FRBCH_E_ARG, "nalpha must be 1..32");
  if (!rm_finite(fp->snr_min)) return e.fail(FRBCH_E_ARG, "snr_min must be finite");
  for (uint32_t i = 0; i < fp->nalpha; ++i)
    if (!rm_finite(fp->alpha[i])) return e.fail(FRBCH_E_ARG, "every alpha must be finite");
  return FRBCH_OK;
}

// step 3 of the header; every check has been made.  q may be NULL.
void scat_fit(const frbch_fil_desc* fil, const frbch_scat_params* par, const frbch_scat_bank_params* bp, const ScatBank& bank,
              const frbch_scat_fit_params* fp, uint32_t ncand, const int32_t* k, const uint32_t* r, const uint32_t* nused,
              const uint32_t* nused_s, const int64_t* C, const int64_t* N, double* qout, frbch_scat_sub* sub, frbch_scat_band* band) {
  POST_NO_CONTRACT
  const size_t nsub = fil->nchan / par->ffactor, nsig = bp->nsig, ntau = bp->ntau, K = nsig * ntau, nsh = par->nshift;
  const size_t per = nsub * K * nsh;
  const double tu = (double)par->tfactor * fil->tsamp_s;
  const double unit = tu * 1000.0;
  const double nu_ref = fil->fch1_mhz + ((double)(fil->nchan - 1) / 2.0) * fil->foff_mhz;
  const double lrt = log(bp->rtau);
  std::vector<double> own(qout ? 0 : per), prof(std::max<size_t>(ntau, fp->nalpha)), profa(fp->nalpha), Qrow(nsh);
  std::vector<long long> ds(nsub);
  std::vector<size_t> part;
  memset((void*)sub, 0, (size_t)ncand * nsub * sizeof(frbch_scat_sub));
  memset((void*)band, 0, (size_t)ncand * sizeof(frbch_scat_band));
  for (uint32_t i = 0; i < ncand; ++i) {
    double* q = qout ? qout + (size_t)i * per : own.data();
    const int64_t *Ci = C + (size_t)i * per, *Ni = N + (size_t)i * per;
    frbch_scat_band& B = band[i];
    B.k = k[i]; B.r = r[i]; B.nused = nused[i]; B.nu_ref_mhz = nu_ref;
    const int kr = k[i] - (int32_t)r[i];
    part.clear();
    for (size_t s = 0; s < nsub; ++s) {
      frbch_scat_sub& R = sub[(size_t)i * nsub + s];
      const uint32_t nu = nused_s[(size_t)i * nsub + s];
      R.nused = nu;
      R.freq_mhz = fil->fch1_mhz + ((double)(s * par->ffactor) + (double)(par->ffactor - 1) / 2.0) * fil->foff_mhz;
      double* qs = q + s * K * nsh;
      const double cells = (double)par->tfactor * (double)nu;
      const double vs = ldexp(cells, 2 * kr);
      size_t best = 0;
      double qb = 0.0;
      for (size_t l = 0; l < K * nsh; ++l) {
        const int64_t c = Ci[s * K * nsh + l], nn = Ni[s * K * nsh + l];
        double v = 0.0;
        if (nu && nn > 0 && c > 0) {
          const double cc = (double)c * (double)c;
          const double x = cc / (double)nn;
          v = x / vs;
        }
        qs[l] = v;
        if (v > qb) { qb = v; best = l; }
      }
      if (!(qb > 0.0)) continue;
      const size_t kb = best / nsh, ub = best % nsh, ab = kb / ntau, bb = kb % ntau;
      R.k = (uint32_t)kb; R.u = (uint32_t)ub; R.q = qb; R.snr = sqrt(qb);
      R.sigma = bank.sigma[ab]; R.tau = bank.tau[bb]; R.arrival = (double)(par->shift0 + ub);
      R.sigma_ms = R.sigma * unit; R.tau_ms = R.tau * unit; R.arrival_ms = R.arrival * unit;
      const double amp = (double)Ci[s * K * nsh + best] / (double)Ni[s * K * nsh + best];
      R.amp = ldexp(amp, 15 - kr);
      const double ar = amp * (double)bank.s1[kb];
      R.area = ldexp(ar, -kr);
      for (size_t b = 0; b < ntau; ++b) {
        double m = 0.0;
        for (size_t a = 0; a < nsig; ++a)
          for (size_t u = 0; u < nsh; ++u) m = std::max(m, qs[(a * ntau + b) * nsh + u]);
        prof[b] = m;
      }
      size_t lo = bb, hi = bb;
      const double thr = qb - 1.0;
      for (size_t b = 0; b < ntau; ++b)
        if (prof[b] >= thr) { lo = std::min(lo, b); hi = std::max(hi, b); }
      R.tau_lo = bank.tau[lo] * unit; R.tau_hi = bank.tau[hi] * unit;
      R.bounded_lo = lo > 0 ? 1 : 0; R.bounded_hi = hi + 1 < ntau ? 1 : 0;
      R.dq_unscattered = qb - prof[0];
      if (R.snr >= fp->snr_min) part.push_back(s);
    }
    B.nfit = (uint32_t)part.size();
    if (part.empty()) continue;
    // the band: Q over (alpha, b_ref, a, u)
    double Qb = -1.0;
    size_t bia = 0, bbr = 0, ba = 0, bu = 0;
    std::fill(prof.begin(), prof.end(), 0.0);
    std::fill(profa.begin(), profa.end(), 0.0);
    for (uint32_t ia = 0; ia < fp->nalpha; ++ia) {
      for (size_t s : part) {
        const double nus = sub[(size_t)i * nsub + s].freq_mhz;
        const double lg = log(nus / nu_ref);
        const double t = (-fp->alpha[ia]) * lg;
        ds[s] = (long long)rint(t / lrt);
      }
      for (size_t br = 0; br < ntau; ++br)
        for (size_t a = 0; a < nsig; ++a) {
          std::fill(Qrow.begin(), Qrow.end(), 0.0);
          for (size_t s : part) {
            const long long bs = std::min<long long>(std::max<long long>((long long)br + ds[s], 0), (long long)ntau - 1);
            const double* qs = q + (s * K + a * ntau + (size_t)bs) * nsh;
            for (size_t u = 0; u < nsh; ++u) Qrow[u] = Qrow[u] + qs[u];
          }
          for (size_t u = 0; u < nsh; ++u) {
            const double v = Qrow[u];
            if (v > Qb) { Qb = v; bia = ia; bbr = br; ba = a; bu = u; }
            if (v > prof[br]) prof[br] = v;
            if (v > profa[ia]) profa[ia] = v;
          }
        }
    }
    B.q = Qb; B.ialpha = (uint32_t)bia; B.b_ref = (uint32_t)bbr; B.a = (uint32_t)ba; B.u = (uint32_t)bu;
    B.alpha = fp->alpha[bia]; B.tau_ref = bank.tau[bbr]; B.tau_ref_ms = B.tau_ref * unit;
    B.sigma = bank.sigma[ba]; B.sigma_ms = B.sigma * unit; B.arrival = (double)(par->shift0 + bu); B.arrival_ms = B.arrival * unit;
    for (size_t s : part) {
      const double lg = log(sub[(size_t)i * nsub + s].freq_mhz / nu_ref);
      const double t = (-fp->alpha[bia]) * lg;
      const long long bs = (long long)bbr + (long long)rint(t / lrt);
      if (bs < 0 || bs > (long long)ntau - 1) ++B.nclipped;
    }
    const double thr = Qb - 1.0;
    size_t lo = bbr, hi = bbr;
    for (size_t b = 0; b < ntau; ++b)
      if (prof[b] >= thr) { lo = std::min(lo, b); hi = std::max(hi, b); }
    B.tau_ref_lo = bank.tau[lo] * unit; B.tau_ref_hi = bank.tau[hi] * unit;
    B.bounded_lo = lo > 0 ? 1 : 0; B.bounded_hi = hi + 1 < ntau ? 1 : 0;
    B.alpha_lo = B.alpha_hi = B.alpha;
    for (uint32_t ia = 0; ia < fp->nalpha; ++ia)
      if (profa[ia] >= thr) { B.alpha_lo = std::min(B.alpha_lo, fp->alpha[ia]); B.alpha_hi = std::max(B.alpha_hi, fp->alpha[ia]); }
  }
}

struct ScatOut {
  std::vector<long long> Y, C, N;
  std::vector<uint32_t> yhits;
  std::vector<int32_t> y;
  std::vector<uint8_t> used;
  std::vector<frbch_scat_sub> sub;
  std::vector<frbch_scat_band> band;
  uint32_t k[3] = {0, 0, 0};
};

// everything of a call inside its scope: the preparation, the dynamic spectrum, the quantised plane, C, N, the fit
int scat_run(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
             const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_scat_params* par,
             const frbch_acf_params* apar, const frbch_tbank_shape* sh, const frbch_scat_bank_params* bp,
             const frbch_scat_fit_params* fp, PostScope& ps, ScatOut* out, const PostErr& e) {
  const size_t nbin = par->nbin, nsub = sh->nsub, K = sh->ntemp, ntap = sh->ntap, nsh = sh->nshift;
  const size_t ncell = (size_t)ncand * nsub * nbin, nout = (size_t)ncand * nsub * K * nsh;
  ScatBank bank;
  scat_bank(bp, &bank);
  DynOut dyn;
  int rc = dyn_run(fil, d_rows, nrows, bpar, cands, ncand, flag, apar, ps, &dyn, out->k, e);
  if (rc) return rc;
  out->used.swap(dyn.used);
  int32_t* d_P = nullptr;
  long long* d_C = nullptr;
  POST_DEV(ps.alloc(&d_P, K * ntap * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_C, nout * sizeof(long long)), "hipMalloc");
  POST_DEV(dev_h2d(d_P, bank.p.data(), K * ntap * sizeof(int32_t), ps.s), "upload bank");
  if ((rc = tbank_launch(dyn.d_y, d_P, ncand, sh, FRBCH_TBANK_PLAN, d_C, ps, &out->k[2], e)) != 0) return rc;
  std::vector<int32_t> shift(ncand);
  out->Y.resize(ncell); out->yhits.resize(ncell); out->y.resize(ncell); out->C.resize(nout); out->N.resize(nout);
  POST_DEV(dev_d2h(out->Y.data(), dyn.d_Y, ncell * sizeof(long long), ps.s), "download dynamic spectrum");
  POST_DEV(dev_d2h(out->yhits.data(), dyn.d_hits, ncell * sizeof(uint32_t), ps.s), "download dynamic spectrum");
  POST_DEV(dev_d2h(out->y.data(), dyn.d_y, ncell * sizeof(int32_t), ps.s), "download quantised plane");
  POST_DEV(dev_d2h(shift.data(), dyn.d_shift, (size_t)ncand * sizeof(int32_t), ps.s), "download scale");
  POST_DEV(dev_d2h(out->C.data(), d_C, nout * sizeof(long long), ps.s), "download correlations");
  POST_DEV(dev_sync(ps.s), "sync");

  // all cells complete: N in closed form from the prefix sums, else the same kernel on the 0 / 1 plane with the squared bank
  bool all = true;
  for (size_t i = 0; i < ncand && all; ++i)
    for (size_t s = 0; s < nsub && all; ++s) {
      const uint32_t nu = dyn.nused_s[i * nsub + s];
      const uint32_t* h = out->yhits.data() + (i * nsub + s) * nbin;
      for (size_t j = 0; j < nbin && all; ++j) all = nu > 0 && h[j] == par->tfactor * nu;
    }
  if (all) {
    for (size_t k = 0; k < K; ++k) {
      const int64_t* cum = bank.cum.data() + k * (ntap + 1);
      for (size_t u = 0; u < nsh; ++u) {
        const long long j0 = (long long)par->shift0 + (long long)u - (long long)sh->lead;
        const long long lo = std::max<long long>(0, -j0), hi = std::min<long long>((long long)ntap, (long long)nbin - j0);
        out->N[k * nsh + u] = cum[hi] - cum[lo];
      }
    }
    for (size_t is = 1; is < (size_t)ncand * nsub; ++is) memcpy(out->N.data() + is * K * nsh, out->N.data(), K * nsh * sizeof(long long));
  } else {
    uint32_t kn = 0;
    POST_DEV(dev_h2d(d_P, bank.psq.data(), K * ntap * sizeof(int32_t), ps.s), "upload bank");
    if ((rc = tbank_launch(dyn.d_mask, d_P, ncand, sh, FRBCH_TBANK_PLAN, d_C, ps, &kn, e)) != 0) return rc;
    POST_DEV(dev_d2h(out->N.data(), d_C, nout * sizeof(long long), ps.s), "download template energies");
    POST_DEV(dev_sync(ps.s), "sync");
  }
  std::vector<uint32_t> ushift(ncand);
  for (size_t i = 0; i < ncand; ++i) ushift[i] = (uint32_t)shift[i];
  out->sub.resize((size_t)ncand * nsub);
  out->band.resize(ncand);
  scat_fit(fil, par, bp, bank, fp, ncand, dyn.prep.kscale.data(), ushift.data(), dyn.prep.nused.data(), dyn.nused_s.data(),
           (const int64_t*)out->C.data(), (const int64_t*)out->N.data(), nullptr, out->sub.data(), out->band.data());
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_scat_bank(const frbch_scat_bank_params* bp, int32_t* p, int64_t* s1, int64_t* cum, double* tail, double* sigma,
                               double* tau, char* err, size_t err_cap) try {
  static_assert(sizeof(frbch_scat_bank_params) == 64 && sizeof(frbch_tbank_shape) == 32 && sizeof(frbch_scat_params) == 32 &&
                sizeof(frbch_scat_fit_params) == 272 && sizeof(frbch_scat_sub) == 136 && sizeof(frbch_scat_band) == 152, "scattering records");
  PostErr e{err, err_cap};
  const int rc = scat_check_bank(bp, e);
  if (rc) return rc;
  ScatBank b;
  scat_bank(bp, &b);
  deliver(p, b.p);
  deliver(s1, b.s1);
  deliver(cum, b.cum);
  deliver(tail, b.tail);
  deliver(sigma, b.sigma);
  deliver(tau, b.tau);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_tbank_kernel(uint32_t n, const frbch_tbank_shape* sh, uint32_t form) try {
  const int rc = tbank_check(n, sh, form, PostErr{nullptr, 0});
  return rc ? rc : (tbank_plan_rule(n, sh, form).fastk ? 1 : 0);
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_tbank_device(const int32_t* d_y, const int32_t* d_P, uint32_t n, const frbch_tbank_shape* sh, uint32_t form,
                                  int device, int64_t* d_C, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = tbank_check(n, sh, form, e);
  if (rc) return rc;
  if (!d_y || !d_P || !d_C) return e.fail(FRBCH_E_ARG, "null argument");
  uint32_t k[1] = {0};
  rc = burst_device_call(device, e, [&](PostScope& ps) {
    const int rc = tbank_launch(d_y, d_P, n, sh, form, (long long*)d_C, ps, k, e);
    if (rc) return rc;
    POST_DEV(dev_sync(ps.s), "sync");
    return (int)FRBCH_OK;
  });
  if (rc) return rc;
  deliver(kernel_used, k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_tbank_host(const int32_t* y, const int32_t* P, uint32_t n, const frbch_tbank_shape* sh, uint32_t form, int device,
                                int64_t* C, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = tbank_check(n, sh, form, e);
  if (rc) return rc;
  if (!y || !P || !C) return e.fail(FRBCH_E_ARG, "null argument");
  const size_t ncell = (size_t)n * sh->nsub * sh->nbin, nbank = (size_t)sh->ntemp * sh->ntap, nout = (size_t)n * sh->nsub * sh->ntemp * sh->nshift;
  for (size_t i = 0; i < ncell; ++i)
    if (y[i] > kTbMaxY || y[i] < -kTbMaxY) return e.fail(FRBCH_E_ARG, "a value of the plane lies outside -2^21 .. 2^21: the int64 sums are not safe");
  for (size_t i = 0; i < nbank; ++i)
    if (P[i] > kTbMaxP || P[i] < -kTbMaxP) return e.fail(FRBCH_E_ARG, "a tap of the bank lies outside -2^30 .. 2^30: the int64 sums are not safe");
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  HostStage hs;
  int32_t* d_y = hs.in(y, ncell * sizeof(int32_t));
  int32_t* d_P = hs.in(P, nbank * sizeof(int32_t));
  int64_t* d_C = hs.out(C, nout * sizeof(int64_t));
  return hs.run(e, "device memory for the plane", "upload plane", "download correlations", [&]() {
    return frbch_tbank_device(d_y, d_P, n, sh, form, device, d_C, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstscat_fit(const frbch_fil_desc* fil, const frbch_scat_params* par, const frbch_scat_bank_params* bp,
                                   const frbch_scat_fit_params* fp, uint32_t ncand, const int32_t* k, const uint32_t* r,
                                   const uint32_t* nused, const uint32_t* nused_s, const int64_t* C, const int64_t* N, double* q,
                                   frbch_scat_sub* sub, frbch_scat_band* band, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!fil || fil->size != sizeof(frbch_fil_desc) || fil->nchan < 1 || !(fil->tsamp_s > 0) || fil->foff_mhz == 0.0) return e.fail(FRBCH_E_ARG, "frbch_fil_desc: wrong size, or bad nchan / tsamp / foff");
  if (!par || par->size != sizeof(frbch_scat_params)) return e.fail(FRBCH_E_ARG, "frbch_scat_params: wrong size");
  if (par->tfactor < 1 || par->tfactor > kWinMaxT) return e.fail(FRBCH_E_ARG, "tfactor must be 1..512");
  if (par->ffactor < 1 || par->ffactor > fil->nchan || fil->nchan % par->ffactor) return e.fail(FRBCH_E_ARG, "ffactor must be 1..nchan and divide nchan");
  int rc = scat_check_bank(bp, e);
  if (rc) return rc;
  const frbch_tbank_shape sh{sizeof(frbch_tbank_shape), fil->nchan / par->ffactor, par->nbin, bp->nsig * bp->ntau, bp->ntap, bp->lead, par->shift0, par->nshift};
  if ((rc = tbank_check(ncand, &sh, FRBCH_TBANK_PLAN, e)) != 0) return rc;
  if ((rc = scat_check_fit(fp, e)) != 0) return rc;
  if (!k || !r || !nused || !nused_s || !C || !N) return e.fail(FRBCH_E_ARG, "null argument");
  for (uint32_t i = 0; i < ncand; ++i)
    if (r[i] > 40 || k[i] < -1024 || k[i] > 1024) return e.fail(FRBCH_E_ARG, "candidate " + std::to_string(i) + ": k or r out of range");
  ScatBank bank;
  scat_bank(bp, &bank);
  const size_t nout = (size_t)ncand * sh.nsub * sh.ntemp * sh.nshift;
  std::vector<double> qv(q ? nout : 0);
  std::vector<frbch_scat_sub> sv((size_t)ncand * sh.nsub);
  std::vector<frbch_scat_band> bv(ncand);
  scat_fit(fil, par, bp, bank, fp, ncand, k, r, nused, nused_s, C, N, q ? qv.data() : nullptr, sv.data(), bv.data());
  deliver(q, qv);
  deliver(sub, sv);
  deliver(band, bv);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstscat_kernel(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                      const frbch_burst_cand* cands, uint32_t ncand, const frbch_scat_params* par,
                                      const frbch_scat_bank_params* bp, uint32_t* kernel_used) try {
  PostErr e{nullptr, 0};
  frbch_acf_params apar;
  frbch_tbank_shape sh;
  int rc = scat_check(fil, nrows, bpar, cands, ncand, par, bp, &apar, &sh, e);
  if (rc) return rc;
  if (!d_rows) return FRBCH_E_ARG;
  std::vector<int32_t> delays;
  if ((rc = acf_delays(fil, cands, ncand, &apar, &delays, e)) != 0) return rc;
  if (kernel_used) {
    kernel_used[0] = burst_fast_layout(fil, d_rows) ? 1 : 0;
    kernel_used[1] = dyn_plan_rule(fil, d_rows, bpar->products, delays, ncand, &apar).fastk ? 1 : 0;
    kernel_used[2] = tbank_plan_rule(ncand, &sh, FRBCH_TBANK_PLAN).fastk ? 1 : 0;
  }
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return FRBCH_E_NOMEM; }

extern "C" int frbch_burstscat_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_burst_params* bpar,
                                      const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_scat_params* par,
                                      const frbch_scat_bank_params* bp, const frbch_scat_fit_params* fp, int device, int64_t* Y,
                                      uint32_t* yhits, int32_t* y, int64_t* C, int64_t* N, frbch_scat_sub* sub, frbch_scat_band* band,
                                      uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  frbch_acf_params apar;
  frbch_tbank_shape sh;
  int rc = scat_check(fil, nrows, bpar, cands, ncand, par, bp, &apar, &sh, e);
  if (rc) return rc;
  if ((rc = scat_check_fit(fp, e)) != 0) return rc;
  if (!d_rows) return e.fail(FRBCH_E_ARG, "null argument");
  ScatOut out;
  rc = burst_device_call(device, e, [&](PostScope& ps) { return scat_run(fil, d_rows, nrows, bpar, cands, ncand, flag, par, &apar, &sh, bp, fp, ps, &out, e); });
  if (rc) return rc;
  deliver(Y, out.Y);
  deliver(yhits, out.yhits);
  deliver(y, out.y);
  deliver(C, out.C);
  deliver(N, out.N);
  deliver(sub, out.sub);
  deliver(band, out.band);
  deliver(used, out.used);
  deliver(kernel_used, out.k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_burstscat_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_burst_params* bpar,
                                    const frbch_burst_cand* cands, uint32_t ncand, const uint8_t* flag, const frbch_scat_params* par,
                                    const frbch_scat_bank_params* bp, const frbch_scat_fit_params* fp, int device, int64_t* Y,
                                    uint32_t* yhits, int32_t* y, int64_t* C, int64_t* N, frbch_scat_sub* sub, frbch_scat_band* band,
                                    uint8_t* used, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  frbch_acf_params apar;
  frbch_tbank_shape sh;
  int rc = scat_check(fil, nrows, bpar, cands, ncand, par, bp, &apar, &sh, e);
  if (rc) return rc;
  if ((rc = scat_check_fit(fp, e)) != 0) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return frbch_burstscat_device(fil, d_rows, nrows, bpar, cands, ncand, flag, par, bp, fp, device, Y, yhits, y, C, N, sub, band, used, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

// ---------------------------------------------------------------------------------------------------------------------
// refinement of a fold: DM, spin frequency and frequency derivative (include/frbch.h states the arithmetic)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kFfMaxBin = 4096, kFfMaxSub = 4096, kFfMaxChan = 16384;
constexpr uint64_t kFfMaxTrial = 1ull << 22, kFfMaxProf = 1ull << 24, kFfMaxPlane = 1ull << 31;

inline uint64_t ff_rows_per_sub(const frbch_fil_desc* fil, double subint_s) {
  return std::max<uint64_t>(1, (uint64_t)llround(subint_s / fil->tsamp_s));
}
inline uint32_t ff_popcount(uint32_t m) { uint32_t n = 0; for (; m; m &= m - 1) ++n; return n; }
inline uint64_t ff_ntrial(const frbch_foldfit_params* par) { return (uint64_t)par->ndm * par->nfdot * par->nfreq; }

// every refusal that needs neither the flag nor a table
int ff_check(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const PostErr& e) {
  POST_NO_CONTRACT
  if (!par || par->size != sizeof(frbch_foldfit_params)) return e.fail(FRBCH_E_ARG, "frbch_foldfit_params: wrong size");
  const int rc = post_check_fil(fil, nrows, e);
  if (rc) return rc;
  if (fil->nbits == 32) return e.fail(FRBCH_E_ARG, "float rows: the search adds exact integers, 8- or 16-bit rows only");
  if (fil->nifs > 4) return e.fail(FRBCH_E_ARG, "nifs must be 1..4");
  if (fil->nchan > kFfMaxChan) return e.fail(FRBCH_E_ARG, "more than 16384 channels");
  if (par->nbin < 2 || par->nbin > kFfMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 2..4096");
  if (par->nsub < 1 || par->nsub > kFfMaxSub) return e.fail(FRBCH_E_ARG, "nsub must be 1..4096");
  const uint32_t n[3] = {par->ndm, par->nfreq, par->nfdot};
  const char* const name[3] = {"ndm", "nfreq", "nfdot"};
  for (int a = 0; a < 3; ++a)
    if (n[a] < 1 || (n[a] > 1 && n[a] % 2 == 0)) return e.fail(FRBCH_E_ARG, std::string(name[a]) + " must be odd or 1");
  if (ff_ntrial(par) > kFfMaxTrial) return e.fail(FRBCH_E_ARG, "ndm * nfdot * nfreq exceeds 2^22");
  if ((uint64_t)par->ndm * par->nsub * par->nbin > kFfMaxPlane) return e.fail(FRBCH_E_ARG, "ndm * nsub * nbin exceeds 2^31: cut the DM axis");
  if (!par->products) return e.fail(FRBCH_E_ARG, "products: an empty mask");
  if (par->products >> fil->nifs) return e.fail(FRBCH_E_ARG, "products: a product beyond nifs");
  if (!(par->f0_fold > 0) || !std::isfinite(par->f0_fold)) return e.fail(FRBCH_E_ARG, "f0_fold must be positive and finite");
  const double step[3] = {par->ddm, par->dfreq, par->dfdot};
  const char* const sname[3] = {"ddm", "dfreq", "dfdot"};
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(step[a])) return e.fail(FRBCH_E_ARG, std::string(sname[a]) + " is not finite");
    if (n[a] > 1 && !(step[a] > 0)) return e.fail(FRBCH_E_ARG, std::string(sname[a]) + " must be positive where its axis has more than one trial");
  }
  if (!std::isfinite(par->dm0)) return e.fail(FRBCH_E_ARG, "dm0 is not finite");
  if (!(par->fit_frac > 0) || !(par->fit_frac <= 1)) return e.fail(FRBCH_E_ARG, "fit_frac must lie in (0, 1]");
  if (par->nwidth < 1 || par->nwidth > 8) return e.fail(FRBCH_E_ARG, "nwidth must be 1..8");
  for (uint32_t w = 0; w < par->nwidth; ++w)
    if (par->widths[w] < 1 || par->widths[w] > par->nbin / 2) return e.fail(FRBCH_E_ARG, "a width outside 1..nbin / 2");
  const unsigned __int128 big = (unsigned __int128)((1ull << fil->nbits) - 1) * nrows * fil->nchan * ff_popcount(par->products);
  if (big >= ((unsigned __int128)1 << 53)) return e.fail(FRBCH_E_ARG, "(2^nbits - 1) * nrows * nchan * products reaches 2^53: the sums would not be exact doubles");
  if (!(par->subint_s > 0)) return e.fail(FRBCH_E_ARG, "subint_s must be positive");
  const long want = frbch_fold_nsub(fil, nrows, par->subint_s);
  if (want <= 0 || (uint32_t)want != par->nsub) return e.fail(FRBCH_E_ARG, "nsub must be frbch_fold_nsub()");
  return FRBCH_OK;
}

struct FfPlan {
  uint64_t L = 0;
  std::vector<int32_t> shd;        // [ndm][nchan]
  std::vector<int32_t> shp;        // [nfdot][nfreq][nsub]: (-shP) mod nbin, which the kernels add
  std::vector<uint8_t> use;        // [nchan]
};

inline double ff_axis(uint32_t i, uint32_t n, double step) {
  POST_NO_CONTRACT
  return (double)((long long)i - (long long)(n / 2)) * step;
}

// y bins -> 0 .. nbin - 1; false: beyond 2^52
inline bool ff_reduce(double y, uint32_t nbin, int32_t* out) {
  if (!(fabs(y) <= 4503599627370496.0)) return false;
  long long m = (long long)rint(y) % (long long)nbin;
  if (m < 0) m += nbin;
  *out = (int32_t)m;
  return true;
}

// the tables of the header; `flag` may be NULL
int ff_build(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const uint8_t* flag, FfPlan* plan,
             const PostErr& e) {
  POST_NO_CONTRACT
  const uint32_t nchan = fil->nchan, nbin = par->nbin, nsub = par->nsub;
  plan->L = ff_rows_per_sub(fil, par->subint_s);
  plan->use.assign(nchan, 1);
  for (uint32_t c = 0; flag && c < nchan; ++c)
    if (flag[c]) plan->use[c] = 0;
  plan->shd.resize((size_t)par->ndm * nchan);
  for (uint32_t k = 0; k < par->ndm; ++k) {
    const double dm = par->dm0 + ff_axis(k, par->ndm, par->ddm);
    if (!(dm >= 0.0) || !(dm < 1.0e5)) return e.fail(FRBCH_E_ARG, "DM trial " + std::to_string(k) + " lies outside [0, 1e5)");
    for (uint32_t c = 0; c < nchan; ++c) {
      const double turns = post_delay_s(fil, dm, c) * par->f0_fold;
      if (!ff_reduce(turns * (double)nbin, nbin, &plan->shd[(size_t)k * nchan + c])) return e.fail(FRBCH_E_ARG, "a DM shift beyond 2^52 bins");
    }
  }
  std::vector<double> tau(nsub);
  for (uint32_t s = 0; s < nsub; ++s) {
    const uint64_t first = (uint64_t)s * plan->L, r = std::min<uint64_t>(plan->L, nrows - first);
    const double mid = ((double)first + 0.5 * (double)r) - 0.5 * (double)nrows;
    tau[s] = mid * fil->tsamp_s;
  }
  plan->shp.resize((size_t)par->nfdot * par->nfreq * nsub);
  for (uint32_t j = 0; j < par->nfdot; ++j) {
    const double hd = 0.5 * ff_axis(j, par->nfdot, par->dfdot);
    for (uint32_t i = 0; i < par->nfreq; ++i) {
      const double df = ff_axis(i, par->nfreq, par->dfreq);
      for (uint32_t s = 0; s < nsub; ++s) {
        const double lin = df * tau[s];
        const double quad = (hd * tau[s]) * tau[s];
        const double turns = lin + quad;                       // (bin b reads b - shP: the table holds the shift negated)
        if (!ff_reduce(-(turns * (double)nbin), nbin, &plan->shp[((size_t)j * par->nfreq + i) * nsub + s])) return e.fail(FRBCH_E_ARG, "a spin shift beyond 2^52 bins");
      }
    }
  }
  return FRBCH_OK;
}

// The plan rule of the fold refinement -- the one decision behind frbch_foldfit_device's launches, kernel_used and
// frbch_foldfit_kernel's answer.  The fast forms (kernels_post_fast.inc) want the cube and its hits 16-byte aligned (only the
// ADDRESSES are examined; a call that fails this runs the generic form in BOTH stages, so that every shape has a complete
// generic run next to its fast one) and the sums of a sub-integration in 32 bits.  Stage 1: whole tiles of 8 channels and a
// tile of all bins in the LDS (nbin <= 1024); the channel tiles are cut into runs of kFfTileRun, joined when there are
// several.  Stage 2: at least two spin trials a DM (one trial has nothing to share a staged chunk with); sc sub-integrations
// of 12 bytes a bin fill the 64 KiB stage.  The emulator build has no such kernels: generic.
struct FfPlanRule { bool fast1 = false, fast2 = false; int ngrp = 1, bpt1 = 1, bpt2 = 1, sc = 1, lstride = 0, nrun = 1; };
FfPlanRule ff_plan_rule(const frbch_fil_desc* fil, const frbch_foldfit_params* par, const double* d_cube, const uint32_t* d_hits) {
  FfPlanRule r;
#ifndef FRBCH_NO_FAST
  const uint64_t L = ff_rows_per_sub(fil, par->subint_s);
  const unsigned __int128 vmax = (unsigned __int128)((1ull << fil->nbits) - 1) * ff_popcount(par->products) * L;
  const unsigned __int128 hmax = (unsigned __int128)L * fil->nchan;
  const unsigned __int128 lim = (unsigned __int128)1 << 32;
  if (((uintptr_t)d_cube % 16) != 0 || ((uintptr_t)d_hits % 16) != 0 || vmax >= lim || hmax >= lim) return r;
  auto bpt = [](uint32_t nbin) { int b = 1; while ((uint32_t)(b * fast::kFfThreads) < nbin) b *= 2; return b; };
  if (fil->nchan % fast::kFfCT == 0 && par->nbin <= (uint32_t)fast::kFfMaxBin1) {
    r.fast1 = true;
    r.bpt1 = bpt(par->nbin);
    r.lstride = (int)((par->nbin + 31) / 32 * 32 + 4);
    r.ngrp = (int)((fil->nchan / fast::kFfCT + fast::kFfTileRun - 1) / fast::kFfTileRun);
  }
  if ((uint64_t)par->nfdot * par->nfreq >= 2) {
    r.fast2 = true;
    r.bpt2 = bpt(par->nbin);
    r.sc = (int)std::min<uint64_t>(par->nsub, fast::kFfStage2 / (12ull * par->nbin));
    const uint32_t run = (uint32_t)(fast::kFfElems / r.bpt2);
    r.nrun = (int)((par->nfdot * par->nfreq + run - 1) / run);
  }
#else
  (void)fil; (void)par; (void)d_cube; (void)d_hits;
#endif
  return r;
}

// S/N of a profile (the header's rule) -> *snr, *width, *bin
void ff_snr(const int64_t* B, const uint64_t* H, const frbch_foldfit_params* par, double* snr, uint32_t* width, uint32_t* bin) {
  POST_NO_CONTRACT
  const uint32_t nb = par->nbin, nw = nb / 2;
  std::vector<double> x(nb);
  for (uint32_t b = 0; b < nb; ++b) x[b] = H[b] ? (double)B[b] / (double)H[b] : 0.0;
  auto window = [&](uint32_t j, uint32_t w) {
    double s = 0.0;
    for (uint32_t i = 0; i < w; ++i) s = s + x[(j + i) % nb];
    return s;
  };
  uint32_t off = 0;
  double best = window(0, nw);
  for (uint32_t j = 1; j < nb; ++j) {
    const double s = window(j, nw);
    if (s < best) { best = s; off = j; }
  }
  const double base = best / (double)nw;
  double ss = 0.0;
  for (uint32_t i = 0; i < nw; ++i) {
    const double d = x[(off + i) % nb] - base;
    const double dd = d * d;
    ss = ss + dd;
  }
  const double rms = sqrt(ss / (double)nw);
  *snr = 0.0; *width = par->widths[0]; *bin = 0;
  if (!(rms > 0.0)) return;
  bool first = true;
  for (uint32_t wi = 0; wi < par->nwidth; ++wi) {
    const uint32_t w = par->widths[wi];
    const double rw = sqrt((double)w);
    for (uint32_t j = 0; j < nb; ++j) {
      const double m = window(j, w) / (double)w;
      const double v = ((m - base) * rw) / rms;
      if (first || v > *snr) { *snr = v; *width = w; *bin = j; first = false; }
    }
  }
}

// the peaks section of the header; every check has been made
void ff_peaks(const frbch_foldfit_params* par, const double* score, const int64_t* pacc, const uint64_t* phits, frbch_foldfit_result* r) {
  POST_NO_CONTRACT
  memset(r, 0, sizeof *r);
  const uint32_t n[3] = {par->ndm, par->nfdot, par->nfreq};                 // in memory order
  const uint64_t nt = ff_ntrial(par);
  uint64_t at = 0;
  for (uint64_t t = 1; t < nt; ++t)
    if (score[t] > score[at]) at = t;
  const uint32_t kp = (uint32_t)(at / ((uint64_t)n[1] * n[2])), jp = (uint32_t)((at / n[2]) % n[1]), ip = (uint32_t)(at % n[2]);
  r->kpeak = kp; r->jpeak = jp; r->ipeak = ip;
  r->score_peak = score[at];
  r->score_nominal = score[((uint64_t)(n[0] / 2) * n[1] + n[1] / 2) * n[2] + n[2] / 2];
  std::vector<double> border;
  for (uint64_t t = 0; t < nt; ++t) {
    const uint32_t idx[3] = {(uint32_t)(t / ((uint64_t)n[1] * n[2])), (uint32_t)((t / n[2]) % n[1]), (uint32_t)(t % n[2])};
    bool edge = false;
    for (int a = 0; a < 3; ++a)
      if (n[a] > 1 && (idx[a] == 0 || idx[a] == n[a] - 1)) edge = true;
    if (edge) border.push_back(score[t]);
  }
  if (!border.empty()) {
    std::sort(border.begin(), border.end());
    const size_t m = border.size();
    r->border_median = m % 2 ? border[m / 2] : 0.5 * (border[m / 2 - 1] + border[m / 2]);
  }
  const double wide = r->border_median > 0.0 ? sqrt(r->border_median) : 0.0;
  // the three cuts through the peak: values of the axis, the scores along it, then the parabola of frbch_dmscan_peaks
  const double step[3] = {par->ddm, par->dfdot, par->dfreq}, origin[3] = {par->dm0, 0.0, 0.0};
  const uint64_t stride[3] = {(uint64_t)n[1] * n[2], n[2], 1};
  const uint32_t peak[3] = {kp, jp, ip};
  double* value[3] = {&r->dm, &r->dfdot, &r->dfreq};
  double* res[3] = {&r->dm_res, &r->dfdot_res, &r->dfreq_res};
  uint32_t* fitted[3] = {&r->fitted_dm, &r->fitted_fdot, &r->fitted_freq};
  uint32_t* nfit[3] = {&r->nfit_dm, &r->nfit_fdot, &r->nfit_freq};
  for (int a = 0; a < 3; ++a) {
    std::vector<double> v(n[a]), x(n[a]);
    for (uint32_t i = 0; i < n[a]; ++i) {
      v[i] = score[at - (uint64_t)peak[a] * stride[a] + (uint64_t)i * stride[a]];
      x[i] = origin[a] + ff_axis(i, n[a], step[a]);
    }
    uint32_t where = 0;
    double unit = 0.0;
    dm_fit(v.data(), n[a], par->fit_frac, x.data(), step[a], &where, nfit[a], fitted[a], value[a], &unit);
    *res[a] = *fitted[a] ? unit * wide : 0.0;
  }
  ff_snr(pacc, phits, par, &r->snr_nominal, &r->width_nominal, &r->bin_nominal);
  ff_snr(pacc + par->nbin, phits + par->nbin, par, &r->snr_best, &r->width_best, &r->bin_best);
}

struct FfOut {
  std::vector<double> score;
  std::vector<long long> prof, tacc, plane;
  std::vector<unsigned long long> prof_hits, thits, plane_hits;
  frbch_foldfit_result res;
  uint32_t k[2] = {0, 0};
};

// everything of a call inside its scope: the tables up, stage 1, the totals, stage 2, the two profiles, the peaks
int ff_run(const frbch_fil_desc* fil, const frbch_foldfit_params* par, const FfPlan& plan, const double* d_cube, const uint32_t* d_hits,
           bool want_trials, bool want_plane, PostScope& ps, FfOut* out, const PostErr& e) {
  const size_t nchan = fil->nchan, nbin = par->nbin, nsub = par->nsub, ndm = par->ndm, nspin = (size_t)par->nfdot * par->nfreq;
  const size_t nt = ndm * nspin, nplane = ndm * nsub * nbin;
  const FfPlanRule rule = ff_plan_rule(fil, par, d_cube, d_hits);
  out->k[0] = rule.fast1 ? 1 : 0;
  out->k[1] = rule.fast2 ? 1 : 0;
  uint8_t* d_use = nullptr;
  int32_t *d_shd = nullptr, *d_shp = nullptr, *d_shp2 = nullptr;
  uint32_t* d_trial = nullptr;
  long long *d_A = nullptr, *d_totA = nullptr, *d_tacc = nullptr, *d_prof = nullptr;
  unsigned long long *d_HA = nullptr, *d_totH = nullptr, *d_thits = nullptr, *d_prof_hits = nullptr;
  double* d_score = nullptr;
  POST_DEV(ps.alloc(&d_use, nchan), "hipMalloc");
  POST_DEV(ps.alloc(&d_shd, plan.shd.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_shp, plan.shp.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_A, nplane * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_HA, nplane * sizeof(unsigned long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_totA, ndm * nsub * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_totH, ndm * nsub * sizeof(unsigned long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_score, nt * sizeof(double)), "hipMalloc");
  POST_DEV(dev_h2d(d_use, plan.use.data(), nchan, ps.s), "upload the channel mask");
  POST_DEV(dev_h2d(d_shd, plan.shd.data(), plan.shd.size() * sizeof(int32_t), ps.s), "upload the DM shifts");
  POST_DEV(dev_h2d(d_shp, plan.shp.data(), plan.shp.size() * sizeof(int32_t), ps.s), "upload the spin shifts");
  if (want_trials) {
    POST_DEV(ps.alloc(&d_tacc, nt * nbin * sizeof(long long)), "hipMalloc");
    POST_DEV(ps.alloc(&d_thits, nt * nbin * sizeof(unsigned long long)), "hipMalloc");
  }
  FfParams p;
  memset(&p, 0, sizeof p);
  p.cube = d_cube; p.chits = d_hits; p.use = d_use; p.shd = d_shd; p.shp = d_shp;
  p.A = d_A; p.HA = d_HA; p.totA = d_totA; p.totH = d_totH; p.score = d_score; p.pacc = d_tacc; p.phits = d_thits;
  p.nchan = (int)nchan; p.nifs = (int)fil->nifs; p.nbin = (int)nbin; p.nsub = (int)nsub; p.ndm = (int)ndm; p.nspin = (int)nspin;
  p.ntrial = (int)nt; p.products = (int)par->products;
  p.ngrp = rule.ngrp; p.sc = rule.sc; p.lstride = rule.lstride; p.nrun = rule.nrun;
  // stage 1
  bool launched = false;
#ifndef FRBCH_NO_FAST
  if (rule.fast1) {
    if (rule.ngrp > 1) {
      long long* d_part = nullptr;
      uint32_t* d_hpart = nullptr;
      POST_DEV(ps.alloc(&d_part, (size_t)rule.ngrp * nplane * sizeof(long long)), "hipMalloc");
      POST_DEV(ps.alloc(&d_hpart, (size_t)rule.ngrp * nplane * sizeof(uint32_t)), "hipMalloc");
      p.part = d_part; p.hpart = d_hpart;
    }
    const dim3 grid((unsigned)((ndm + fast::kFfND - 1) / fast::kFfND), (unsigned)rule.ngrp, (unsigned)nsub), block(fast::kFfThreads);
    const size_t lds = (size_t)2 * fast::kFfCT * rule.lstride * sizeof(uint32_t);
    int lrc;
    switch (rule.bpt1) {
      case 1: lrc = launch_lds(fast::frbch_post_ff_dm_fast<1>, grid, block, lds, ps.s, p); break;
      case 2: lrc = launch_lds(fast::frbch_post_ff_dm_fast<2>, grid, block, lds, ps.s, p); break;
      default: lrc = launch_lds(fast::frbch_post_ff_dm_fast<4>, grid, block, lds, ps.s, p); break;
    }
    POST_DEV(lrc, "LDS size");
    POST_DEV(dev_check_launch(), "launch fold refinement, stage 1");
    if (rule.ngrp > 1) {
      hipLaunchKernelGGL(fast::frbch_post_ff_dm_join, dim3((unsigned)((nplane + fast::kFfThreads - 1) / fast::kFfThreads)), dim3(fast::kFfThreads), 0, ps.s, p);
      POST_DEV(dev_check_launch(), "launch fold refinement, join");
    }
    launched = true;
  }
#endif
  if (!launched) {
    DEV_LAUNCH(frbch_post_ff_dm, (nplane + 255) / 256, 1, 256, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch fold refinement, stage 1");
  }
  DEV_LAUNCH(frbch_post_ff_tot, (ndm * nsub + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch fold refinement, totals");
  // stage 2
  launched = false;
#ifndef FRBCH_NO_FAST
  if (rule.fast2) {
    const dim3 grid((unsigned)(ndm * (size_t)rule.nrun)), block(fast::kFfThreads);
    int lrc;
    switch (rule.bpt2) {
      case 1: lrc = launch_lds(fast::frbch_post_ff_spin_fast<1>, grid, block, fast::kFfLds2, ps.s, p); break;
      case 2: lrc = launch_lds(fast::frbch_post_ff_spin_fast<2>, grid, block, fast::kFfLds2, ps.s, p); break;
      case 4: lrc = launch_lds(fast::frbch_post_ff_spin_fast<4>, grid, block, fast::kFfLds2, ps.s, p); break;
      case 8: lrc = launch_lds(fast::frbch_post_ff_spin_fast<8>, grid, block, fast::kFfLds2, ps.s, p); break;
      default: lrc = launch_lds(fast::frbch_post_ff_spin_fast<16>, grid, block, fast::kFfLds2, ps.s, p); break;
    }
    POST_DEV(lrc, "LDS size");
    POST_DEV(dev_check_launch(), "launch fold refinement, stage 2");
    launched = true;
  }
#endif
  if (!launched) {
    DEV_LAUNCH(frbch_post_ff_spin, (nt + 255) / 256, 1, 256, 0, ps.s, p);
    POST_DEV(dev_check_launch(), "launch fold refinement, stage 2");
  }
  out->score.resize(nt);
  POST_DEV(dev_d2h(out->score.data(), d_score, nt * sizeof(double), ps.s), "download the scores");
  if (want_trials) {
    out->tacc.resize(nt * nbin);
    out->thits.resize(nt * nbin);
    POST_DEV(dev_d2h(out->tacc.data(), d_tacc, nt * nbin * sizeof(long long), ps.s), "download the trial profiles");
    POST_DEV(dev_d2h(out->thits.data(), d_thits, nt * nbin * sizeof(unsigned long long), ps.s), "download the trial profiles");
  }
  if (want_plane) {
    out->plane.resize(nsub * nbin);
    out->plane_hits.resize(nsub * nbin);
    const size_t at = (ndm / 2) * nsub * nbin;
    POST_DEV(dev_d2h(out->plane.data(), d_A + at, nsub * nbin * sizeof(long long), ps.s), "download the phase-time plane");
    POST_DEV(dev_d2h(out->plane_hits.data(), d_HA + at, nsub * nbin * sizeof(unsigned long long), ps.s), "download the phase-time plane");
  }
  POST_DEV(dev_sync(ps.s), "sync");
  // the profiles of the nominal and of the peak trial
  size_t best = 0;
  for (size_t t = 1; t < nt; ++t)
    if (out->score[t] > out->score[best]) best = t;
  const uint32_t two[2] = {(uint32_t)((ndm / 2) * nspin + ((size_t)(par->nfdot / 2) * par->nfreq + par->nfreq / 2)), (uint32_t)best};
  std::vector<int32_t> shp2(2 * nsub);
  for (int t = 0; t < 2; ++t)
    memcpy(shp2.data() + (size_t)t * nsub, plan.shp.data() + (size_t)(two[t] % nspin) * nsub, nsub * sizeof(int32_t));
  POST_DEV(ps.alloc(&d_shp2, shp2.size() * sizeof(int32_t)), "hipMalloc");
  POST_DEV(ps.alloc(&d_trial, sizeof two), "hipMalloc");
  POST_DEV(ps.alloc(&d_prof, 2 * nbin * sizeof(long long)), "hipMalloc");
  POST_DEV(ps.alloc(&d_prof_hits, 2 * nbin * sizeof(unsigned long long)), "hipMalloc");
  POST_DEV(dev_h2d(d_shp2, shp2.data(), shp2.size() * sizeof(int32_t), ps.s), "upload the spin shifts");
  POST_DEV(dev_h2d(d_trial, two, sizeof two, ps.s), "upload the trial list");
  p.shp = d_shp2; p.trial = d_trial; p.ntrial = 2; p.score = nullptr; p.pacc = d_prof; p.phits = d_prof_hits;
  DEV_LAUNCH(frbch_post_ff_prof, (2 * nbin + 255) / 256, 1, 256, 0, ps.s, p);
  POST_DEV(dev_check_launch(), "launch fold refinement, profiles");
  out->prof.resize(2 * nbin);
  out->prof_hits.resize(2 * nbin);
  POST_DEV(dev_d2h(out->prof.data(), d_prof, 2 * nbin * sizeof(long long), ps.s), "download the profiles");
  POST_DEV(dev_d2h(out->prof_hits.data(), d_prof_hits, 2 * nbin * sizeof(unsigned long long), ps.s), "download the profiles");
  POST_DEV(dev_sync(ps.s), "sync");
  ff_peaks(par, out->score.data(), (const int64_t*)out->prof.data(), (const uint64_t*)out->prof_hits.data(), &out->res);
  return FRBCH_OK;
}

// the arguments of frbch_foldfit_device / _host behind the cube
int ff_check_outputs(const frbch_foldfit_params* par, const void* cube, const void* hits, const void* score, const void* pacc, const void* phits,
                     const void* result, const void* tacc, const void* thits, const void* plane, const void* plane_hits, const PostErr& e) {
  if (!cube || !hits || !score || !pacc || !phits || !result) return e.fail(FRBCH_E_ARG, "null argument");
  if ((tacc == nullptr) != (thits == nullptr)) return e.fail(FRBCH_E_ARG, "trial_acc and trial_hits come together");
  if ((plane == nullptr) != (plane_hits == nullptr)) return e.fail(FRBCH_E_ARG, "plane_acc and plane_hits come together");
  if (tacc && ff_ntrial(par) * par->nbin > kFfMaxProf) return e.fail(FRBCH_E_ARG, "the trial profiles exceed 2^24 elements: ask for the scores alone");
  return FRBCH_OK;
}
}  // namespace

extern "C" int frbch_foldfit_steps(const frbch_fil_desc* fil, uint64_t nrows, uint32_t nbin, double f0_fold, double* ddm, double* dfreq,
                                   double* dfdot) {
  POST_NO_CONTRACT
  PostErr e{nullptr, 0};
  if (post_check_fil(fil, nrows, e) || nbin < 2 || !(f0_fold > 0)) return FRBCH_E_ARG;
  const double T = (double)nrows * fil->tsamp_s;
  if (dfreq) *dfreq = 1.0 / ((double)nbin * T);
  if (dfdot) *dfdot = 8.0 / (((double)nbin * T) * T);
  if (ddm) {
    const double d = post_delay_s(fil, 1.0, fil->foff_mhz < 0 ? fil->nchan - 1 : 0);     // seconds per unit DM across the band
    *ddm = d > 0.0 ? 1.0 / (((double)nbin * f0_fold) * d) : 0.0;
  }
  return FRBCH_OK;
}

extern "C" int frbch_foldfit_kernel(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* d_cube,
                                    const uint32_t* d_hits, uint32_t* kernel) {
  PostErr e{nullptr, 0};
  const int rc = ff_check(fil, nrows, par, e);
  if (rc) return rc;
  if (!d_cube || !d_hits || !kernel) return FRBCH_E_ARG;
  const FfPlanRule rule = ff_plan_rule(fil, par, d_cube, d_hits);
  kernel[0] = rule.fast1 ? 1 : 0;
  kernel[1] = rule.fast2 ? 1 : 0;
  return FRBCH_OK;
}

extern "C" int frbch_foldfit_device(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* d_cube,
                                    const uint32_t* d_hits, const uint8_t* flag, int device, double* score, int64_t* prof_acc,
                                    uint64_t* prof_hits, frbch_foldfit_result* result, int64_t* trial_acc, uint64_t* trial_hits,
                                    int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap) try {
  static_assert(sizeof(frbch_foldfit_params) == 120 && sizeof(frbch_foldfit_result) == 144 && sizeof(long long) == sizeof(int64_t), "fold refinement records");
  PostErr e{err, err_cap};
  int rc = ff_check(fil, nrows, par, e);
  if (rc) return rc;
  if ((rc = ff_check_outputs(par, d_cube, d_hits, score, prof_acc, prof_hits, result, trial_acc, trial_hits, plane_acc, plane_hits, e)) != 0) return rc;
  FfPlan plan;
  if ((rc = ff_build(fil, nrows, par, flag, &plan, e)) != 0) return rc;
  FfOut out;
  rc = burst_device_call(device, e, [&](PostScope& ps) { return ff_run(fil, par, plan, d_cube, d_hits, trial_acc != nullptr, plane_acc != nullptr, ps, &out, e); });
  if (rc) return rc;
  deliver(score, out.score);
  deliver(prof_acc, out.prof);
  deliver(prof_hits, out.prof_hits);
  deliver(trial_acc, out.tacc);
  deliver(trial_hits, out.thits);
  deliver(plane_acc, out.plane);
  deliver(plane_hits, out.plane_hits);
  *result = out.res;
  deliver(kernel_used, out.k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_foldfit_host(const frbch_fil_desc* fil, uint64_t nrows, const frbch_foldfit_params* par, const double* cube,
                                  const uint32_t* hits, const uint8_t* flag, int device, double* score, int64_t* prof_acc,
                                  uint64_t* prof_hits, frbch_foldfit_result* result, int64_t* trial_acc, uint64_t* trial_hits,
                                  int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = ff_check(fil, nrows, par, e);
  if (rc) return rc;
  if ((rc = ff_check_outputs(par, cube, hits, score, prof_acc, prof_hits, result, trial_acc, trial_hits, plane_acc, plane_hits, e)) != 0) return rc;
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  const size_t nslot = (size_t)par->nsub * par->nbin * fil->nchan;
  HostStage hs;
  const double* d_cube = hs.in(cube, nslot * fil->nifs * sizeof(double));
  const uint32_t* d_hits = hs.in(hits, nslot * sizeof(uint32_t));
  return hs.run(e, "device memory for the cube", "upload the cube", "download", [&]() {
    return frbch_foldfit_device(fil, nrows, par, d_cube, d_hits, flag, device, score, prof_acc, prof_hits, result, trial_acc, trial_hits, plane_acc,
                                plane_hits, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_foldfit_peaks(const frbch_foldfit_params* par, const double* score, const int64_t* prof_acc, const uint64_t* prof_hits,
                                   frbch_foldfit_result* result, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  if (!par || par->size != sizeof(frbch_foldfit_params)) return e.fail(FRBCH_E_ARG, "frbch_foldfit_params: wrong size");
  if (par->nbin < 2 || par->nbin > kFfMaxBin) return e.fail(FRBCH_E_ARG, "nbin must be 2..4096");
  if (par->ndm < 1 || par->nfreq < 1 || par->nfdot < 1 || ff_ntrial(par) > kFfMaxTrial) return e.fail(FRBCH_E_ARG, "ndm * nfdot * nfreq exceeds 2^22");
  if (!(par->fit_frac > 0) || !(par->fit_frac <= 1)) return e.fail(FRBCH_E_ARG, "fit_frac must lie in (0, 1]");
  if (par->nwidth < 1 || par->nwidth > 8) return e.fail(FRBCH_E_ARG, "nwidth must be 1..8");
  for (uint32_t w = 0; w < par->nwidth; ++w)
    if (par->widths[w] < 1 || par->widths[w] > par->nbin / 2) return e.fail(FRBCH_E_ARG, "a width outside 1..nbin / 2");
  if (!score || !prof_acc || !prof_hits || !result) return e.fail(FRBCH_E_ARG, "null argument");
  frbch_foldfit_result r;
  ff_peaks(par, score, prof_acc, prof_hits, &r);
  *result = r;
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_fold_refine_device(const frbch_fil_desc* fil, const void* d_rows, uint64_t nrows, const frbch_fold_model* model,
                                        const frbch_foldfit_params* par, const uint8_t* flag, int device, double* cube, uint32_t* cube_hits,
                                        double* score, int64_t* prof_acc, uint64_t* prof_hits, frbch_foldfit_result* result,
                                        int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  int rc = ff_check(fil, nrows, par, e);
  if (rc) return rc;
  if (!model || model->size != sizeof(frbch_fold_model)) return e.fail(FRBCH_E_ARG, "frbch_fold_model: wrong size");
  if (model->apply_delays) return e.fail(FRBCH_E_ARG, "a fold with apply_delays: the search shifts the channels itself, fold without per-channel delays");
  if (model->nbin != par->nbin || model->subint_s != par->subint_s) return e.fail(FRBCH_E_ARG, "the model and the search differ in nbin or subint_s");
  if (!d_rows || !score || !prof_acc || !prof_hits || !result) return e.fail(FRBCH_E_ARG, "null argument");
  if ((plane_acc == nullptr) != (plane_hits == nullptr)) return e.fail(FRBCH_E_ARG, "plane_acc and plane_hits come together");
  {                                                        // the refusals that only the tables show, before anything is written
    FfPlan probe;
    if ((rc = ff_build(fil, nrows, par, flag, &probe, e)) != 0) return rc;
  }
  if ((rc = post_check_device(device, e)) != 0) return rc;
  DeviceGuard dg(device);
  PostScope ps(false);                                     // holds the cube between the two stages
  if (!ps.s) return e.fail(FRBCH_E_DEVICE, "hipStreamCreate");
  const size_t nslot = (size_t)par->nsub * par->nbin * fil->nchan;
  double* d_cube = nullptr;
  uint32_t* d_chits = nullptr;
  POST_DEV(ps.alloc(&d_cube, nslot * fil->nifs * sizeof(double)), "hipMalloc");
  POST_DEV(ps.alloc(&d_chits, nslot * sizeof(uint32_t)), "hipMalloc");
  uint32_t k[3] = {0, 0, 0};
  if ((rc = frbch_foldp_device(fil, d_rows, nrows, model, device, d_cube, d_chits, par->nsub, &k[0], err, err_cap)) != 0) return rc;
  if (cube) POST_DEV(dev_d2h(cube, d_cube, nslot * fil->nifs * sizeof(double), ps.s), "download the cube");
  if (cube_hits) POST_DEV(dev_d2h(cube_hits, d_chits, nslot * sizeof(uint32_t), ps.s), "download the cube");
  POST_DEV(dev_sync(ps.s), "sync");                        // (the results below are written last, and only by a call that succeeds)
  if ((rc = frbch_foldfit_device(fil, nrows, par, d_cube, d_chits, flag, device, score, prof_acc, prof_hits, result, nullptr, nullptr, plane_acc,
                                 plane_hits, &k[1], err, err_cap)) != 0) return rc;
  deliver(kernel_used, k);
  return FRBCH_OK;
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }

extern "C" int frbch_fold_refine_host(const frbch_fil_desc* fil, const void* rows, uint64_t nrows, const frbch_fold_model* model,
                                      const frbch_foldfit_params* par, const uint8_t* flag, int device, double* cube, uint32_t* cube_hits,
                                      double* score, int64_t* prof_acc, uint64_t* prof_hits, frbch_foldfit_result* result,
                                      int64_t* plane_acc, uint64_t* plane_hits, uint32_t* kernel_used, char* err, size_t err_cap) try {
  PostErr e{err, err_cap};
  const int rc = ff_check(fil, nrows, par, e);
  if (rc) return rc;
  if (!rows) return e.fail(FRBCH_E_ARG, "null argument");
  return burst_host_twin(fil, rows, nrows, device, e, [&](void* d_rows) {
    return frbch_fold_refine_device(fil, d_rows, nrows, model, par, flag, device, cube, cube_hits, score, prof_acc, prof_hits, result, plane_acc,
                                    plane_hits, kernel_used, err, err_cap);
  });
} catch (const std::bad_alloc&) { return PostErr{err, err_cap}.fail(FRBCH_E_NOMEM, "host memory"); }
