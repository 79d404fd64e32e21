// TEST INFRASTRUCTURE ONLY: calls frbch_candidates_host (interference cases: 8-, 16-bit and float rows, two products, foff > 0,
// with and without planes, no candidate, argument errors) and frbch_rfi_cleanp_host (2 and 4 products, the three sample widths,
// a short last block) on the emulator build and frees every result.  Then the failure walk of tests/test_post_failures.py over
// frbch_candidates_host, frbch_rfi_cleanp_host, frbch_cutout_host and frbch_foldp_host: the n-th fallible device-layer call fails,
// n = 1, 2, ... until the call succeeds; here only "not 0" is asked of a failed call -- AddressSanitizer, UBSan and LeakSanitizer
// give the verdict on what it left behind.  Built with -fsanitize=address,undefined (Makefile).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "frbch.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

template <class T>
static std::vector<T> make_rows(uint64_t nrows, uint32_t nifs, uint32_t nchan, uint32_t product, const frbch_fil_desc& fil, double dm,
                                double scale, double offset) {
  std::vector<T> x((size_t)nrows * nifs * nchan);
  const double ftop = fil.foff_mhz < 0 ? fil.fch1_mhz : fil.fch1_mhz + (nchan - 1) * fil.foff_mhz;
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t p = 0; p < nifs; ++p)
      for (uint32_t c = 0; c < nchan; ++c) {
        double v = 96.0 + (double)(rnd() % 64);
        if (p == product) {
          const double f = fil.fch1_mhz + c * fil.foff_mhz;
          const long d = (long)(dm / 2.41e-4 * (1.0 / (f * f) - 1.0 / (ftop * ftop)) / fil.tsamp_s + 0.5);
          if ((long)t >= 3000 + d && (long)t < 3005 + d) v += 30.0;
          if (c == 20) v = 100.0;                                         // dead
          if (c == 50 && t >= 5 * 256 + 30 && t < 5 * 256 + 200) v += 90.0;   // loud inside one block
        }
        x[((size_t)t * nifs + p) * nchan + c] = (T)(v * scale + offset);
      }
  return x;
}

static int fails = 0;
#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++fails; } } while (0)

// the emulator's test hooks (tests/emu/emu_hooks.cpp)
extern "C" void frbch_test_emu_fail_at(long n);
extern "C" uint64_t frbch_test_emu_live(void);

// call() -> return code, with the n-th fallible device-layer call failing, until it returns 0; nothing stays alive on the device
template <class F>
static void failure_walk(const char* name, F call) {
  const uint64_t live = frbch_test_emu_live();
  long n = 1;
  for (; n < 1000; ++n) {
    frbch_test_emu_fail_at(n);
    const int rc = call();
    frbch_test_emu_fail_at(0);
    EXPECT(frbch_test_emu_live() == live);
    if (rc == FRBCH_OK) break;
  }
  EXPECT(n > 3 && n < 1000);
  printf("  %s: %ld failure returns walked\n", name, n - 1);
}

template <class T>
static void candidates_case(int nbits, uint32_t nifs, uint32_t product, double foff, double scale, double offset, uint32_t nt, double threshold,
                            bool walk = false) {
  const uint32_t nchan = 64;
  const uint64_t nrows = 9000;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = nbits; fil.product = product;
  fil.fch1_mhz = foff < 0 ? 1400.0 : 1400.0 - 63 * 0.5;
  fil.foff_mhz = foff; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.25;
  std::vector<T> rows = make_rows<T>(nrows, nifs, nchan, product, fil, 56.7, scale, offset);
  const std::vector<T> before = rows;
  double dms[9];
  for (int i = 0; i < 9; ++i) dms[i] = 36.7 + 5.0 * i;
  std::vector<uint8_t> zap(nchan, 0);
  zap[41] = 1;
  frbch_cand_params par;
  memset(&par, 0, sizeof par);
  par.size = sizeof par;
  par.flags = FRBCH_CAND_RFI | FRBCH_CAND_SERIES;
  par.rfi.size = sizeof par.rfi;
  par.rfi.block_rows = 256; par.rfi.t_cell = 5.0; par.rfi.t_chan = 5.0; par.rfi.chan_frac = 0.3; par.rfi.block_frac = 0.3;
  par.zap = zap.data();
  par.zerodm = 1; par.clip_sigma = 5.0;
  par.sp.size = sizeof par.sp;
  const uint32_t widths[] = {1, 2, 3, 4, 6, 9, 14, 20, 30};
  par.sp.nwidth = 9;
  memcpy(par.sp.widths, widths, sizeof widths);
  par.sp.threshold = threshold;
  par.dm_gap = 2; par.min_members = 1; par.max_cands = 0;
  par.cut.size = sizeof par.cut;
  par.cut.nt = nt; par.cut.nf = 16; par.cut.ndm = 16;
  par.dm_span = foff > 0 ? 30.0 : 0.0;
  char err[1024] = "";
  frbch_cand_result* res = nullptr;
  const int rc = frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, &par, 0, &res, err, sizeof err);
  EXPECT(rc == FRBCH_OK);
  if (rc != FRBCH_OK) { fprintf(stderr, "  %s\n", err); return; }
  EXPECT(rows == before);
  frbch_cand_view v;
  memset(&v, 0, sizeof v);
  v.size = sizeof v;
  EXPECT(frbch_cand_result_view(res, &v) == FRBCH_OK);
  EXPECT(v.row_uploads == 1 && v.nblk == 36 && v.mask && v.series);
  uint64_t masked = 0, touched = 0;
  for (size_t i = 0; i < (size_t)v.nblk * nchan; ++i) masked += v.mask[i];
  EXPECT(masked >= 2 * 36 + 1 && v.mask[5 * nchan + 50] && v.chan_flag[20] && v.chan_flag[41] && !v.chan_flag[50]);
  if (threshold < 100.0) {
    EXPECT(v.ncand >= 9 && v.ngroup >= 1);
    for (uint64_t i = 0; i < v.ncand; ++i) touched += v.cands[i].sample;            // every record is readable
    for (uint64_t i = 0; i < v.ngroup; ++i) touched += v.groups[i].nmember + v.cut_cands[i].tfactor;
    if (nt) {
      EXPECT(v.ft && v.ft_hits && v.dt && v.dt_hits && v.cutout_calls == 1);
      for (size_t i = 0; i < (size_t)v.ngroup * 16 * nt; ++i) touched += v.ft_hits[i] + v.dt_hits[i] + (v.ft[i] > 0) + (v.dt[i] > 0);
    } else {
      EXPECT(!v.ft && !v.dt && v.cutout_calls == 0);
    }
  } else {
    EXPECT(v.ncand == 0 && v.ngroup == 0 && !v.cands && !v.groups && !v.ft && !v.dt_hits);
  }
  for (size_t i = 0; i < (size_t)9 * v.nout; ++i) touched += v.series[i] > 0;
  EXPECT(touched > 0);
  frbch_cand_result_free(res);
  // refused calls leave nothing behind
  par.min_members = 0;
  res = (frbch_cand_result*)(uintptr_t)1;
  EXPECT(frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, &par, 0, &res, err, sizeof err) == FRBCH_E_ARG && !res && err[0]);
  par.min_members = 1;
  par.cut.nt = 3;
  EXPECT(frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, &par, 0, &res, err, sizeof err) == FRBCH_E_ARG && !res);
  par.cut.nt = nt;
  par.size -= 4;
  EXPECT(frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, &par, 0, &res, err, sizeof err) == FRBCH_E_ARG && !res);
  EXPECT(frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, nullptr, 0, nullptr, err, sizeof err) == FRBCH_E_ARG);
  frbch_cand_result_free(nullptr);
  par.size = sizeof par;
  if (walk)
    failure_walk("frbch_candidates_host", [&]() {
      frbch_cand_result* r = (frbch_cand_result*)(uintptr_t)1;
      const int code = frbch_candidates_host(&fil, rows.data(), nrows, dms, 9, &par, 0, &r, err, sizeof err);
      EXPECT((code == FRBCH_OK) == (r != nullptr) && rows == before);
      frbch_cand_result_free(r);
      return code;
    });
}

template <class T>
static void cleanp_case(int nbits, uint32_t nifs, uint32_t nchan, uint64_t nrows, double scale, double offset, bool want_stats, bool walk = false) {
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = nbits; fil.product = 7;            // ignored
  fil.fch1_mhz = 1416.0; fil.foff_mhz = -0.03125; fil.tsamp_s = 32e-6; fil.tstart_mjd = 59000.25;
  std::vector<T> rows((size_t)nrows * nifs * nchan);
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t p = 0; p < nifs; ++p)
      for (uint32_t c = 0; c < nchan; ++c) {
        double v = 40.0 + 15.0 * p + (double)(rnd() % (24 + 8 * p));
        if (c == (7 + 5 * p) % nchan) v += 30.0 + p;
        if (t >= nrows / 3 && t < nrows / 3 + 2 + p) v += 50.0;
        rows[((size_t)t * nifs + p) * nchan + c] = (T)(v * scale + offset);
      }
  const std::vector<T> before = rows;
  frbch_rfi_params par;
  memset(&par, 0, sizeof par);
  par.size = sizeof par;
  par.block_rows = 256; par.t_cell = 3.0; par.t_chan = 5.0; par.chan_frac = 0.3; par.block_frac = 0.3;
  const long nblk = frbch_rfi_nblk(nrows, par.block_rows);
  EXPECT(nblk > 0 && nrows % 256 != 0);
  std::vector<uint8_t> zap(nchan, 0), mask((size_t)nblk * nchan), cf(nchan), bf((size_t)nblk);
  zap[3] = 1;
  std::vector<double> repl((size_t)nifs * nchan);
  std::vector<uint64_t> stats(want_stats ? (size_t)nifs * nblk * nchan * 2 : 0);
  uint32_t used = 9;
  char err[512] = "";
  const int rc = frbch_rfi_cleanp_host(&fil, rows.data(), nrows, &par, zap.data(), 0, mask.data(), repl.data(), cf.data(), bf.data(),
                                       want_stats ? stats.data() : nullptr, &used, err, sizeof err);
  EXPECT(rc == FRBCH_OK && used == 0);
  if (rc != FRBCH_OK) fprintf(stderr, "  %s\n", err);
  EXPECT(cf[3] == 1 && rows != before);
  par.block_rows = 0;
  EXPECT(frbch_rfi_cleanp_host(&fil, rows.data(), nrows, &par, zap.data(), 0, mask.data(), repl.data(), cf.data(), bf.data(), nullptr,
                               &used, err, sizeof err) == FRBCH_E_ARG);
  par.block_rows = 256;
  if (walk)
    failure_walk("frbch_rfi_cleanp_host", [&]() {
      rows = before;
      return frbch_rfi_cleanp_host(&fil, rows.data(), nrows, &par, zap.data(), 0, mask.data(), repl.data(), cf.data(), bf.data(),
                                   want_stats ? stats.data() : nullptr, &used, err, sizeof err);
    });
}

// 8-bit rows of 64 channels: the planes of two candidates, one of them over the end of the data; the fold of both products
static void cutout_and_fold_walk() {
  const uint32_t nchan = 64, nifs = 2;
  const uint64_t nrows = 3000;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8; fil.product = 1;
  fil.fch1_mhz = 1400.0; fil.foff_mhz = -0.5; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.25;
  const std::vector<uint8_t> rows = make_rows<uint8_t>(nrows, nifs, nchan, 1, fil, 56.7, 1.0, 0.0);
  char err[512] = "";
  uint32_t used = 9;
  frbch_cutout_params cut = {sizeof cut, 6, 16, 9};
  frbch_cutout_cand cands[2];
  memset(cands, 0, sizeof cands);
  cands[0].dm = 56.7; cands[0].dm_hi = 113.4; cands[0].sample = 1500; cands[0].tfactor = 3;
  cands[1].dm = 30.0; cands[1].dm_hi = 60.0; cands[1].sample = 2995; cands[1].tfactor = 2;
  std::vector<float> ft(2 * 16 * 6), dt(2 * 9 * 6);
  std::vector<uint32_t> fth(ft.size()), dth(dt.size());
  failure_walk("frbch_cutout_host", [&]() {
    return frbch_cutout_host(&fil, rows.data(), nrows, &cut, cands, 2, 0, ft.data(), fth.data(), dt.data(), dth.data(), &used, err, sizeof err);
  });
  EXPECT(used == 0 && fth[0] > 0);
  frbch_fold_model m;
  memset(&m, 0, sizeof m);
  m.size = sizeof m;
  m.f0_hz = 29.9; m.f1 = -2.5e-9; m.pepoch_mjd = 59000.0; m.dm = 56.7; m.apply_delays = 1; m.nbin = 16; m.subint_s = 0.07;
  const long nsub = frbch_fold_nsub(&fil, nrows, m.subint_s);
  EXPECT(nsub > 1);
  std::vector<double> prof((size_t)nsub * nifs * m.nbin * nchan);
  std::vector<uint32_t> hits((size_t)nsub * m.nbin * nchan);
  failure_walk("frbch_foldp_host", [&]() {
    return frbch_foldp_host(&fil, rows.data(), nrows, &m, 0, prof.data(), hits.data(), (uint32_t)nsub, &used, err, sizeof err);
  });
  uint64_t total = 0;
  for (uint32_t h : hits) total += h;
  EXPECT(used == 0 && total == nrows * nchan);
}

int main() {
  candidates_case<uint8_t>(8, 1, 0, -0.5, 1.0, 0.0, 32, 6.0);
  candidates_case<uint16_t>(16, 1, 0, -0.5, 201.0, 0.0, 32, 6.0);
  candidates_case<float>(32, 1, 0, -0.5, 0.37, -3.0, 32, 6.0);
  candidates_case<uint8_t>(8, 2, 1, -0.5, 1.0, 0.0, 32, 6.0, true);
  candidates_case<uint8_t>(8, 1, 0, +0.5, 1.0, 0.0, 32, 6.0);
  candidates_case<uint8_t>(8, 1, 0, -0.5, 1.0, 0.0, 0, 6.0);          // no planes
  candidates_case<uint8_t>(8, 1, 0, -0.5, 1.0, 0.0, 32, 1000.0);      // no candidate
  cleanp_case<uint8_t>(8, 2, 64, 24 * 256 - 100, 1.0, 0.0, true, true);
  cleanp_case<uint8_t>(8, 4, 64, 2100, 1.0, 0.0, false);
  cleanp_case<uint16_t>(16, 2, 48, 1500, 201.0, 0.0, true);
  cleanp_case<uint16_t>(16, 4, 64, 1025, 201.0, 0.0, true);
  cleanp_case<float>(32, 2, 64, 1500, 0.37, -3.0, true);
  cleanp_case<float>(32, 4, 48, 2049, 0.37, -3.0, false);
  cutout_and_fold_walk();
  printf(fails ? "FAILED: %d expectation(s)\n" : "resident_sanitize: all expectations hold, no sanitizer report\n", fails);
  return fails ? 1 : 0;
}
