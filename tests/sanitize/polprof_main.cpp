// TEST INFRASTRUCTURE ONLY: the polarisation profile under AddressSanitizer and UBSan, as a stand-alone program linked against
// the emulator sources (CPU only; never loaded into python, never run on a GPU): one small call through the generic kernel
// (8-bit rows of 96 channels, bins partly in front of the data and behind it, a candidate wholly outside, a flagged channel,
// gains with a zero and an infinite entry, both product orders and both reference wavelengths), the refusals, and a failure
// walk of frbch_polprof_host.
//   make -C tests/sanitize -f polprof.mk run
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
  const uint32_t nchan = 96, nifs = 4, nbin = 40, ncand = 4;
  const uint64_t nrows = 1500;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1415.0; fil.foff_mhz = -1.0; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  frbch_burst_params bpar = {sizeof(frbch_burst_params), FRBCH_BURST_STOKES};
  frbch_prof_params ppar = {sizeof(frbch_prof_params), nbin, 3, FRBCH_PROF_REF_MEAN, 0};

  // rows: a floor with noise, a burst of 5 rows at DM 60 with a linear polarisation rotating at 1500 rad m^-2
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(100 + rnd() % 7);
  const double kdm = 1.0 / 2.41e-4;
  for (uint32_t c = 0; c < nchan; ++c) {
    const double f = fil.fch1_mhz + c * fil.foff_mhz, l2 = (299.792458 / f) * (299.792458 / f);
    const long d = (long)(60.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz)) / fil.tsamp_s + 0.5);
    const double amp[4] = {60.0, 40.0 * cos(2.0 * 1500.0 * l2), 40.0 * sin(2.0 * 1500.0 * l2), 10.0};
    for (long t = 698; t < 703; ++t)
      for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)(t + d) * nifs + p) * nchan + c] = (uint8_t)(rows[((size_t)(t + d) * nifs + p) * nchan + c] + (int)lrint(amp[p]));
  }
  const std::vector<uint8_t> rows0 = rows;
  // the burst; one whose bins begin in front of the data; one wholly outside; one whose bins run off the end
  frbch_burst_cand cands[ncand] = {{60.0, 700, 5, 8, 100, 0}, {60.0, 40, 6, 8, 100, 0}, {60.0, 5000, 4, 8, 100, 0}, {10.0, 1460, 9, 2, 50, 0}};
  const double rm[ncand] = {1500.0, 0.0, -2500.0, 1.0e7};
  std::vector<float> gain((size_t)nifs * nchan, 1.5f);
  gain[1 * nchan + 7] = -0.5f;
  gain[2 * nchan + 9] = 0.f;
  gain[3 * nchan + 11] = INFINITY;
  std::vector<uint8_t> flag(nchan, 0);
  flag[3] = flag[95] = 1;
  std::vector<int64_t> acc((size_t)ncand * nbin * 4, 7);
  std::vector<uint32_t> hits((size_t)ncand * nbin, 7);
  std::vector<frbch_prof_bin> bins((size_t)ncand * nbin);
  std::vector<frbch_prof_result> res(ncand);
  std::vector<uint8_t> used((size_t)ncand * nchan, 7);
  uint32_t k[2] = {9, 9};

  CHECK(frbch_polprof_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &ppar) == 0);
  CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, rm, gain.data(), flag.data(), &ppar, 0, acc.data(), hits.data(),
                           bins.data(), res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(k[0] == 0 && k[1] == 0 && rows == rows0);
  CHECK(res[0].nused == nchan - 3 && used[3] == 0 && used[95] == 0 && used[11] == 0 && used[9] == 1 && used[7] == 1);
  CHECK(res[0].on_lo_bin == 19 && res[0].on_hi_bin == 20 && res[0].sigma_l > 0.0 && res[0].lref > 0.04);
  for (uint32_t j = 0; j < nbin; ++j) {
    CHECK(hits[j] == 3 * (nchan - 3));
    CHECK(hits[(size_t)2 * nbin + j] == 0 && acc[((size_t)2 * nbin + j) * 4 + 1] == 0 && bins[(size_t)2 * nbin + j].pa_valid == 0);
  }
  CHECK(res[2].nused == 0 && res[2].k == 0 && hits[(size_t)1 * nbin] > 0 && hits[(size_t)1 * nbin] < 3 * res[1].nused);   // (only the delayed channels reach row 0)
  CHECK(hits[(size_t)1 * nbin + nbin - 1] == 3 * res[1].nused && hits[(size_t)3 * nbin + nbin - 1] < 3 * res[3].nused);
  const frbch_prof_bin& peak = bins[20];
  CHECK(peak.pa_valid == 1 && peak.i > 50.0 && peak.l_db > 30.0 && peak.l_db < peak.i && peak.pa_err > 0.0 && fabs(peak.pa) <= 1.5707963267948968);
  const std::vector<int64_t> want = acc;

  // every output optional; coherency order; the other reference wavelength; one bin of 512 rows; 16-bit rows
  CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, rm, nullptr, nullptr, &ppar, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                           nullptr, 0) == FRBCH_OK);
  frbch_burst_params cpar = {sizeof(frbch_burst_params), FRBCH_BURST_COHERENCY};
  frbch_prof_params zpar = {sizeof(frbch_prof_params), nbin, 3, FRBCH_PROF_REF_ZERO, 0};
  CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &cpar, cands, ncand, rm, gain.data(), nullptr, &zpar, 0, acc.data(), hits.data(), bins.data(),
                           res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(res[0].lref == 0.0 && res[0].nused == nchan - 1);
  frbch_prof_params wide = {sizeof(frbch_prof_params), 1, 512, FRBCH_PROF_REF_MEAN, 0};
  CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, rm, nullptr, nullptr, &wide, 0, acc.data(), hits.data(), bins.data(), res.data(),
                           used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(hits[0] > 500 * nchan && hits[0] <= 512 * nchan);                 // (the most delayed channels run off the end)
  {
    std::vector<uint16_t> rows16(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows16[i] = (uint16_t)(rows[i] * 200);
    frbch_fil_desc f16 = fil;
    f16.nbits = 16;
    CHECK(frbch_polprof_host(&f16, rows16.data(), nrows, &bpar, cands, ncand, rm, nullptr, nullptr, &ppar, 0, acc.data(), hits.data(), bins.data(),
                             res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(bins[20].i > 50.0 * 200 && res[0].k == 4);                        // 3 x 2^16 = 0.75 x 2^18
  }

  // the refusals
  {
    const frbch_prof_params bads[] = {{8, nbin, 3, 0, 0}, {sizeof(frbch_prof_params), 0, 3, 0, 0}, {sizeof(frbch_prof_params), 1025, 3, 0, 0},
                                      {sizeof(frbch_prof_params), nbin, 0, 0, 0}, {sizeof(frbch_prof_params), nbin, 513, 0, 0},
                                      {sizeof(frbch_prof_params), nbin, 3, 2, 0}};
    for (const frbch_prof_params& b : bads) {
      err[0] = 0;
      CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, rm, nullptr, nullptr, &b, 0, acc.data(), hits.data(), bins.data(), res.data(),
                               used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0]);
      CHECK(frbch_polprof_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &b) == FRBCH_E_ARG);
    }
    frbch_fil_desc two = fil, flt = fil, manych = fil;
    two.nifs = 2;
    flt.nbits = 32;
    manych.nchan = 16385;
    manych.foff_mhz = -0.01;
    CHECK(frbch_polprof_kernel(&two, rows.data(), nrows, &bpar, cands, ncand, &ppar) == FRBCH_E_ARG);
    CHECK(frbch_polprof_kernel(&flt, rows.data(), nrows, &bpar, cands, ncand, &ppar) == FRBCH_E_ARG);
    CHECK(frbch_polprof_kernel(&manych, rows.data(), nrows, &bpar, cands, ncand, &ppar) == FRBCH_E_ARG);
    CHECK(frbch_polprof_kernel(&fil, nullptr, nrows, &bpar, cands, ncand, &ppar) == FRBCH_E_ARG);
    CHECK(frbch_polprof_kernel(&fil, rows.data(), nrows, &bpar, cands, 0, &ppar) == FRBCH_E_ARG);
    CHECK(frbch_polprof_kernel(&fil, rows.data(), nrows, &bpar, cands, 4097, &ppar) == FRBCH_E_ARG);
    const double bad_rm[3] = {NAN, INFINITY, -1.0001e7};
    for (double v : bad_rm) {
      double r2[ncand] = {0.0, 0.0, v, 0.0};
      err[0] = 0;
      CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, r2, nullptr, nullptr, &ppar, 0, acc.data(), hits.data(), bins.data(), res.data(),
                               used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0]);
    }
    CHECK(frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, nullptr, nullptr, &ppar, 0, acc.data(), hits.data(), bins.data(), res.data(),
                             used.data(), k, err, sizeof err) == FRBCH_E_ARG);
    frbch_burst_cand c = cands[0];
    c.width = 0;
    CHECK(frbch_polprof_kernel(&fil, rows.data(), nrows, &bpar, &c, 1, &ppar) == FRBCH_E_ARG);
  }

  // the failure walk: every fallible device-layer call fails once; nothing is left behind and nothing is written
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long n = 1; n < 200; ++n, ++steps) {
      std::fill(acc.begin(), acc.end(), 7);
      frbch_test_emu_fail_at(n);
      err[0] = 0;
      const int rc = frbch_polprof_host(&fil, rows.data(), nrows, &bpar, cands, ncand, rm, gain.data(), flag.data(), &ppar, 0, acc.data(), hits.data(),
                                        bins.data(), res.data(), used.data(), k, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0] && acc[0] == 7 && acc.back() == 7);
    }
    CHECK(steps > 15 && steps < 199 && rows == rows0 && acc == want);
  }
  printf("polprof_sanitize: ok\n");
  return 0;
}
