// TEST INFRASTRUCTURE ONLY: the DM scan under AddressSanitizer and UBSan, as a stand-alone program linked against the emulator
// sources (CPU only; never loaded into python, never run on a GPU): one small call through the generic kernel (8-bit rows of 96
// channels, bins partly in front of the data and behind it, a candidate wholly outside, a flagged and a constant channel, both
// product orders, a one-product file, 16-bit rows), the peaks alone, the refusals, and a failure walk of frbch_dmscan_host.
//   make -C tests/sanitize -f dmscan.mk run
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "frbch.h"

extern "C" void frbch_test_emu_fail_at(long n);
extern "C" uint64_t frbch_test_emu_live();

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

int main() {
  char err[512];
  const uint32_t nchan = 96, nifs = 4, nbin = 40, ntrial = 9, ncand = 4;
  const uint64_t nrows = 1500;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1415.0; fil.foff_mhz = -1.0; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  frbch_burst_params bpar = {sizeof(frbch_burst_params), FRBCH_BURST_STOKES};
  const double step = frbch_dm_sample_step(&fil);
  CHECK(step > 0.2 && step < 0.3);
  frbch_dmscan_params par = {sizeof(frbch_dmscan_params), ntrial, nbin, 3, step / 2.0};
  frbch_dmscan_peak_params pk;
  memset(&pk, 0, sizeof pk);
  pk.size = sizeof pk;
  pk.nwidth = 3; pk.widths[0] = 1; pk.widths[1] = 2; pk.widths[2] = 4;
  pk.smooth = 3; pk.fit_frac = 0.5;

  // rows: a floor with noise, a burst of 5 rows at DM 60 in every product; channel 20 is constant
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(100 + rnd() % 7);
  const double kdm = 1.0 / 2.41e-4;
  for (uint32_t c = 0; c < nchan; ++c) {
    const double f = fil.fch1_mhz + c * fil.foff_mhz;
    const long d = (long)(60.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz)) / fil.tsamp_s + 0.5);
    for (long t = 698; t < 703; ++t)
      for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)(t + d) * nifs + p) * nchan + c] += 60;
  }
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)t * nifs + p) * nchan + 20] = 100;
  const std::vector<uint8_t> rows0 = rows;
  // the burst; one whose bins begin in front of the data; one wholly outside; one whose bins run off the end
  frbch_burst_cand cands[ncand] = {{60.0, 700, 5, 8, 100, 0}, {60.0, 40, 6, 8, 100, 0}, {60.0, 5000, 4, 8, 100, 0}, {10.0, 1460, 9, 2, 50, 0}};
  std::vector<uint8_t> flag(nchan, 0);
  flag[3] = flag[95] = 1;
  const size_t nout = (size_t)ncand * ntrial * nbin;
  std::vector<int64_t> acc(nout, 7);
  std::vector<uint32_t> hits(nout, 7);
  std::vector<double> snr((size_t)ncand * ntrial, 7.0), strc((size_t)ncand * ntrial, 7.0);
  std::vector<frbch_dmscan_result> res(ncand);
  std::vector<uint8_t> used((size_t)ncand * nchan, 7);
  uint32_t k[2] = {9, 9};

  CHECK(frbch_dmscan_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par) == 0);
  CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                          res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(k[0] == 0 && k[1] == 0 && rows == rows0);
  CHECK(res[0].nused == nchan - 3 && used[3] == 0 && used[95] == 0 && used[20] == 0 && used[9] == 1);
  CHECK(res[0].k_snr + 1 >= ntrial / 2 && res[0].k_snr <= ntrial / 2 + 1 && res[0].snr_peak > 100.0 && fabs(res[0].dm_snr - 60.0) < 2.0 * step);
  CHECK(res[0].nfit_snr >= 3 && res[0].nfit_snr <= ntrial && (res[0].fitted_snr == 1) == (res[0].dm_snr_err > 0.0));
  for (uint32_t j = 0; j < nbin; ++j) {
    CHECK(hits[(size_t)(ntrial / 2) * nbin + j] == 3 * (nchan - 3));
    CHECK(hits[((size_t)2 * ntrial + 1) * nbin + j] == 0 && acc[((size_t)2 * ntrial + 1) * nbin + j] == 0);
  }
  CHECK(res[2].nused == 0 && res[2].k == 0 && res[2].dm_snr == 0.0 && snr[(size_t)2 * ntrial] == 0.0);
  CHECK(hits[(size_t)1 * ntrial * nbin] > 0 && hits[(size_t)1 * ntrial * nbin] < 3 * res[1].nused);       // (only the delayed channels reach row 0)
  CHECK(hits[((size_t)3 * ntrial + ntrial - 1) * nbin + nbin - 1] < 3 * res[3].nused);
  const std::vector<int64_t> want = acc;
  const std::vector<double> want_snr = snr, want_strc = strc;

  // the peaks alone give the same curves and results
  {
    int32_t ks[ncand];
    uint32_t nu[ncand];
    for (uint32_t i = 0; i < ncand; ++i) { ks[i] = res[i].k; nu[i] = res[i].nused; }
    std::vector<double> s2((size_t)ncand * ntrial), t2((size_t)ncand * ntrial);
    std::vector<uint32_t> wd((size_t)ncand * ntrial), bn((size_t)ncand * ntrial);
    std::vector<frbch_dmscan_result> r2(ncand);
    CHECK(frbch_dmscan_peaks(&par, &pk, cands, ncand, ks, nu, acc.data(), hits.data(), s2.data(), t2.data(), wd.data(), bn.data(), r2.data(), err,
                             sizeof err) == FRBCH_OK);
    CHECK(s2 == snr && t2 == strc && memcmp(r2.data(), res.data(), ncand * sizeof(frbch_dmscan_result)) == 0);
    CHECK(wd[ntrial / 2] == res[0].width_snr && bn[ntrial / 2] == res[0].bin_snr);
    CHECK(frbch_dmscan_peaks(&par, &pk, cands, ncand, ks, nu, acc.data(), hits.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == FRBCH_OK);
    CHECK(frbch_dmscan_peaks(&par, &pk, cands, ncand, nullptr, nu, acc.data(), hits.data(), nullptr, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
  }

  // every output optional; coherency order; another product; one trial, one bin of 512 rows; a one-product file; 16-bit rows
  CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &pk, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, 0) == FRBCH_OK);
  frbch_burst_params cpar = {sizeof(frbch_burst_params), FRBCH_BURST_COHERENCY};
  CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &cpar, cands, ncand, nullptr, &par, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                          res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(res[0].nused == nchan - 1 && res[0].snr_peak > 100.0);
  {
    frbch_fil_desc f2 = fil;
    f2.product = 3;
    CHECK(frbch_dmscan_host(&f2, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                            res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(res[0].nused == nchan - 1);
    frbch_dmscan_params one = {sizeof(frbch_dmscan_params), 1, 1, 512, NAN};
    frbch_dmscan_peak_params pk1 = pk;
    pk1.nwidth = 1;
    CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &one, &pk1, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                            res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(hits[0] > 500 * (nchan - 1) && hits[0] <= 512 * (nchan - 1) && res[0].fitted_snr == 0 && res[0].dm_struct == 60.0 && strc[0] == 0.0);
    std::vector<uint8_t> single((size_t)nrows * nchan);
    for (uint64_t t = 0; t < nrows; ++t) memcpy(&single[(size_t)t * nchan], &rows[(size_t)t * nifs * nchan], nchan);
    frbch_fil_desc f1 = fil;
    f1.nifs = 1;
    CHECK(frbch_dmscan_host(&f1, single.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                            res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(acc == want && snr == want_snr && strc == want_strc);              // product 0 of the four-product file
    std::vector<uint16_t> rows16(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows16[i] = (uint16_t)(rows[i] * 200);
    frbch_fil_desc f16 = fil;
    f16.nbits = 16;
    CHECK(frbch_dmscan_host(&f16, rows16.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                            res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(fabs(snr[ntrial / 2] - want_snr[ntrial / 2]) < 1e-6 * want_snr[ntrial / 2]);
  }

  // the refusals
  {
    const frbch_dmscan_params bads[] = {{8, ntrial, nbin, 3, 0.1}, {sizeof(frbch_dmscan_params), 0, nbin, 3, 0.1}, {sizeof(frbch_dmscan_params), 4097, nbin, 3, 0.1},
                                        {sizeof(frbch_dmscan_params), ntrial, 0, 3, 0.1}, {sizeof(frbch_dmscan_params), ntrial, 1025, 3, 0.1},
                                        {sizeof(frbch_dmscan_params), ntrial, nbin, 0, 0.1}, {sizeof(frbch_dmscan_params), ntrial, nbin, 513, 0.1},
                                        {sizeof(frbch_dmscan_params), ntrial, nbin, 3, 0.0}, {sizeof(frbch_dmscan_params), ntrial, nbin, 3, NAN},
                                        {sizeof(frbch_dmscan_params), ntrial, nbin, 3, INFINITY}, {sizeof(frbch_dmscan_params), ntrial, nbin, 3, 3.0}};
    for (const frbch_dmscan_params& b : bads) {
      err[0] = 0;
      std::fill(acc.begin(), acc.end(), 7);
      CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &b, &pk, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                              res.data(), used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && acc[0] == 7);
      CHECK(frbch_dmscan_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &b) == FRBCH_E_ARG);
    }
    frbch_dmscan_peak_params bp[6] = {pk, pk, pk, pk, pk, pk};
    bp[0].size = 80; bp[1].nwidth = 17; bp[2].widths[1] = 1; bp[3].widths[2] = nbin + 1; bp[4].smooth = nbin; bp[5].fit_frac = 1.0;
    for (const frbch_dmscan_peak_params& b : bp) {
      err[0] = 0;
      CHECK(frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &b, 0, acc.data(), hits.data(), snr.data(), strc.data(),
                              res.data(), used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && acc[0] == 7);
    }
    frbch_fil_desc two = fil, flt = fil, manych = fil;
    two.nifs = 2;
    flt.nbits = 32;
    manych.nchan = 16385;
    manych.foff_mhz = -0.01;
    CHECK(frbch_dmscan_kernel(&two, rows.data(), nrows, &cpar, cands, ncand, &par) == FRBCH_E_ARG);
    CHECK(frbch_dmscan_kernel(&flt, rows.data(), nrows, &bpar, cands, ncand, &par) == FRBCH_E_ARG);
    CHECK(frbch_dmscan_kernel(&manych, rows.data(), nrows, &bpar, cands, ncand, &par) == FRBCH_E_ARG);
    CHECK(frbch_dmscan_kernel(&fil, nullptr, nrows, &bpar, cands, ncand, &par) == FRBCH_E_ARG);
    CHECK(frbch_dmscan_kernel(&fil, rows.data(), nrows, &bpar, cands, 0, &par) == FRBCH_E_ARG);
    CHECK(frbch_dmscan_kernel(&fil, rows.data(), nrows, &bpar, cands, 4097, &par) == FRBCH_E_ARG);
    frbch_burst_cand c = cands[0];
    c.width = 0;
    CHECK(frbch_dmscan_kernel(&fil, rows.data(), nrows, &bpar, &c, 1, &par) == FRBCH_E_ARG);
    CHECK(frbch_dm_sample_step(nullptr) == 0.0);
  }

  // the failure walk: every fallible device-layer call fails once; nothing is left behind and nothing is written
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long n = 1; n < 200; ++n, ++steps) {
      std::fill(acc.begin(), acc.end(), 7);
      frbch_test_emu_fail_at(n);
      err[0] = 0;
      const int rc = frbch_dmscan_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &pk, 0, acc.data(), hits.data(), snr.data(),
                                       strc.data(), res.data(), used.data(), k, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0] && acc[0] == 7 && acc.back() == 7);
    }
    CHECK(steps > 15 && steps < 199 && rows == rows0 && acc == want);
  }
  printf("dmscan_sanitize: ok\n");
  return 0;
}
