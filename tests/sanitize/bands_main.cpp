// TEST INFRASTRUCTURE ONLY: the band-limited single-pulse search under AddressSanitizer and UBSan, as a stand-alone program
// linked against the emulator sources (CPU only; never loaded into python, never run on a GPU): the band list, the bands
// dedispersion through the generic kernel (8-bit rows with clip and zero-DM, float rows, cut widths, nsub 1 and 16) with band
// [0, nsub) held against frbch_dedisperse_host, the composite with two batches against one, the grouping, the refusals, and a
// failure walk of the composite.
//   make -C tests/sanitize -f bands.mk run
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
  const uint32_t nchan = 64, nifs = 2, ndm = 5;
  const uint64_t nrows = 3000;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8; fil.product = 1;
  fil.fch1_mhz = 1415.75; fil.foff_mhz = -0.5; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  const double dms[ndm] = {40.0, 41.0, 42.0, 43.0, 44.0};

  // rows: noise, a broadband spike that clips, a 4-row burst at DM 42 in channels 16..31 (sub-bands 2 and 3 of 8) of product 1
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(90 + rnd() % 13);
  for (uint32_t c = 0; c < nchan; ++c) rows[((size_t)2500 * nifs + 1) * nchan + c] = 250;
  const double kdm = 1.0 / 2.41e-4;
  for (uint32_t c = 16; c < 32; ++c) {
    const double f = fil.fch1_mhz + c * fil.foff_mhz;
    const long d = (long)(42.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz)) / fil.tsamp_s + 0.5);
    for (long t = 1000; t < 1004; ++t) rows[((size_t)(t + d) * nifs + 1) * nchan + c] += 8;
  }
  const std::vector<uint8_t> rows0 = rows;
  const long nout_l = frbch_dedisperse_nout(&fil, nrows, dms, ndm);
  CHECK(nout_l > 2000);
  const uint64_t nout = (uint64_t)nout_l;

  // the band list
  frbch_band_params bp = {sizeof(frbch_band_params), 8, 0, 0};
  uint16_t lo[136], hi[136];
  uint32_t nband = 0;
  CHECK(frbch_band_list(nchan, &bp, nullptr, nullptr, 0, &nband, err, sizeof err) == FRBCH_E_CAPACITY && nband == 36);
  CHECK(frbch_band_list(nchan, &bp, lo, hi, 136, &nband, err, sizeof err) == FRBCH_OK && nband == 36);
  CHECK(lo[0] == 0 && hi[0] == 1 && lo[7] == 0 && hi[7] == 8 && lo[8] == 1 && hi[8] == 2 && lo[35] == 7 && hi[35] == 8);
  frbch_band_params cut = {sizeof(frbch_band_params), 8, 2, 3};
  CHECK(frbch_band_list(nchan, &cut, lo, hi, 136, &nband, err, sizeof err) == FRBCH_OK && nband == 13 && hi[0] == 2 && hi[1] == 3 && lo[2] == 1);
  frbch_band_params sixteen = {sizeof(frbch_band_params), 16, 0, 0};
  CHECK(frbch_band_list(nchan, &sixteen, lo, hi, 136, &nband, err, sizeof err) == FRBCH_OK && nband == 136);

  // the bands dedispersion: band [0, nsub) is frbch_dedisperse_host's series, the ranges add up on integer rows without zero-DM
  std::vector<float> full((size_t)ndm * nout), plane((size_t)ndm * 36 * nout);
  uint64_t nclip = 0, nclip2 = 0;
  uint32_t used = 9;
  CHECK(frbch_dedisperse_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, 0, full.data(), nout, &nclip, err, sizeof err) == FRBCH_OK);
  CHECK(frbch_dedisperse_bands_kernel(&fil, rows.data(), nrows, dms, ndm, &bp) == 0);
  CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, 0, plane.data(), nout, &nclip2, &used, err, sizeof err) == FRBCH_OK);
  CHECK(used == 0 && nclip == nclip2 && nclip >= 1 && rows == rows0);
  for (uint32_t d = 0; d < ndm; ++d)
    CHECK(memcmp(&plane[((size_t)d * 36 + 7) * nout], &full[(size_t)d * nout], nout * sizeof(float)) == 0);
  CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 0, 0.0, &bp, 0, plane.data(), nout, nullptr, nullptr, err, sizeof err) == FRBCH_OK);
  for (uint64_t t = 0; t < nout; t += 97)                     // [0, 2) + [2, 8) = [0, 8): bands 1, 20 and 7
    CHECK(plane[((size_t)2 * 36 + 1) * nout + t] + plane[((size_t)2 * 36 + 20) * nout + t] == plane[((size_t)2 * 36 + 7) * nout + t]);
  {
    const uint64_t nout1 = (uint64_t)frbch_dedisperse_nout(&fil, nrows, dms, 1);              // one DM: a longer series
    std::vector<float> p13((size_t)ndm * 13 * nout), p1((size_t)ndm * nout), p136((size_t)136 * nout1);
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &cut, 0, p13.data(), nout, nullptr, &used, err, sizeof err) == FRBCH_OK);
    frbch_band_params one = {sizeof(frbch_band_params), 1, 0, 0};
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &one, 0, p1.data(), nout, nullptr, &used, err, sizeof err) == FRBCH_OK);
    CHECK(memcmp(p1.data(), full.data(), p1.size() * sizeof(float)) == 0);
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, 1, 1, 5.0, &sixteen, 0, p136.data(), nout1,
                                      nullptr, &used, err, sizeof err) == FRBCH_OK);
    // float rows
    std::vector<float> frows(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) frows[i] = 0.37f * rows[i] - 3.f;
    frbch_fil_desc ff = fil;
    ff.nbits = 32;
    CHECK(frbch_dedisperse_host(&ff, frows.data(), nrows, dms, ndm, 1, 5.0, 0, full.data(), nout, nullptr, err, sizeof err) == FRBCH_OK);
    CHECK(frbch_dedisperse_bands_host(&ff, frows.data(), nrows, dms, ndm, 1, 5.0, &bp, 0, plane.data(), nout, nullptr, &used, err, sizeof err) == FRBCH_OK);
    for (uint32_t d = 0; d < ndm; ++d)
      CHECK(memcmp(&plane[((size_t)d * 36 + 7) * nout], &full[(size_t)d * nout], nout * sizeof(float)) == 0);
  }

  // the composite: two batches (3 + 2 DMs) give the list of one; the burst is found in band [2, 4)
  frbch_sp_params sp;
  memset(&sp, 0, sizeof sp);
  sp.size = sizeof sp;
  sp.nwidth = 4;
  sp.widths[0] = 1; sp.widths[1] = 2; sp.widths[2] = 4; sp.widths[3] = 8;
  sp.detrend_len = 500;
  sp.threshold = 6.0;
  const uint64_t one_dm = (uint64_t)36 * nout * sizeof(float);
  std::vector<frbch_spb_cand> a(4096), b(4096);
  uint64_t na = 0, nb = 0;
  uint32_t ku[2] = {9, 9}, nbatch = 0;
  double ms[3];
  CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &sp, 0, 0, nout, &nclip2, a.data(), a.size(), &na, ku, &nbatch, ms, err,
                              sizeof err) == FRBCH_OK);
  CHECK(nbatch == 1 && ku[0] == 0 && ku[1] == 0 && nclip2 == nclip && na > 0 && na < a.size());
  CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &sp, 3 * one_dm + 17, 0, nout, nullptr, b.data(), b.size(), &nb, nullptr,
                              &nbatch, nullptr, err, sizeof err) == FRBCH_OK);
  CHECK(nbatch == 2 && na == nb && memcmp(a.data(), b.data(), (size_t)na * sizeof(frbch_spb_cand)) == 0 && rows == rows0);
  CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &sp, 0, 0, nout, nullptr, nullptr, 0, &nb, nullptr, nullptr, nullptr, err,
                              sizeof err) == FRBCH_E_CAPACITY && nb == na);
  CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &sp, one_dm - 1, 0, nout, nullptr, b.data(), b.size(), &nb, nullptr, nullptr,
                              nullptr, err, sizeof err) == FRBCH_E_ARG && strstr(err, "holds no DM"));

  // the grouping
  {
    std::vector<frbch_spb_group> g((size_t)na);
    uint64_t ng = 0;
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 8, a.data(), na, 2, g.data(), g.size(), &ng, err, sizeof err) == FRBCH_OK && ng >= 1 && ng <= na);
    const frbch_spb_group* top = &g[0];
    for (uint64_t i = 1; i < ng; ++i)
      if (g[i].best.sigma > top->best.sigma) top = &g[i];
    CHECK(top->best.sub_lo == 2 && top->best.sub_hi == 4 && top->best.width == 4 && top->best.sample >= 1000 && top->best.sample <= 1004);
    CHECK(top->sub_lo_min <= 2 && top->sub_hi_max >= 4 && top->nmember >= 1 && top->full_sigma < top->best.sigma);
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 8, a.data(), na, 2, nullptr, 0, &ng, err, sizeof err) == FRBCH_E_CAPACITY && ng >= 1);
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 8, a.data(), 0, 2, nullptr, 0, &ng, err, sizeof err) == FRBCH_OK && ng == 0);
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 3, a.data(), na, 2, g.data(), g.size(), &ng, err, sizeof err) == FRBCH_E_ARG);   // sub_hi > nsub
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 17, a.data(), na, 2, g.data(), g.size(), &ng, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_spb_group_cands(&fil, dms, ndm, 8, a.data(), na, 0, g.data(), g.size(), &ng, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_spb_group_cands(&fil, dms, 2, 8, a.data(), na, 2, g.data(), g.size(), &ng, err, sizeof err) == FRBCH_E_ARG);     // dm_index >= ndm
  }

  // the refusals
  {
    const frbch_band_params bads[] = {{8, 8, 0, 0}, {sizeof(frbch_band_params), 0, 0, 0}, {sizeof(frbch_band_params), 17, 0, 0},
                                      {sizeof(frbch_band_params), 3, 0, 0}, {sizeof(frbch_band_params), 8, 3, 2}, {sizeof(frbch_band_params), 8, 1, 9},
                                      {sizeof(frbch_band_params), 8, 9, 0}};
    for (const frbch_band_params& bad : bads) {
      err[0] = 0;
      CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bad, 0, plane.data(), nout, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG && err[0]);
      CHECK(frbch_dedisperse_bands_kernel(&fil, rows.data(), nrows, dms, ndm, &bad) == FRBCH_E_ARG);
      CHECK(frbch_band_list(nchan, &bad, lo, hi, 136, &nband, err, sizeof err) == FRBCH_E_ARG);
      CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bad, &sp, 0, 0, nout, nullptr, b.data(), b.size(), &nb, nullptr, nullptr, nullptr,
                                  err, sizeof err) == FRBCH_E_ARG);
    }
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, nullptr, 0, plane.data(), nout, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_dedisperse_bands_host(&fil, nullptr, nrows, dms, ndm, 1, 5.0, &bp, 0, plane.data(), nout, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, 0, plane.data(), nout + 1, nullptr, nullptr, err, sizeof err) == FRBCH_E_CAPACITY);
    const double far[1] = {9.0e4};
    CHECK(frbch_dedisperse_bands_host(&fil, rows.data(), nrows, far, 1, 1, 5.0, &bp, 0, plane.data(), nout, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    std::vector<double> many(1821, 1.0);                        // 1821 x 36 = 65556 series
    CHECK(frbch_dedisperse_bands_kernel(&fil, rows.data(), nrows, many.data(), 1821, &bp) == FRBCH_E_ARG);
    CHECK(frbch_dedisperse_bands_kernel(&fil, rows.data(), nrows, many.data(), 1820, &bp) == 0);
    frbch_sp_params badsp = sp;
    badsp.threshold = 0.0;
    CHECK(frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &badsp, 0, 0, nout, nullptr, b.data(), b.size(), &nb, nullptr, nullptr, nullptr,
                                err, sizeof err) == FRBCH_E_ARG);
  }

  // the failure walk of the composite with two batches: every fallible device-layer call fails once; nothing is left behind
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long k = 1; k < 400; ++k, ++steps) {
      frbch_test_emu_fail_at(k);
      err[0] = 0;
      const int rc = frbch_bandsearch_host(&fil, rows.data(), nrows, dms, ndm, 1, 5.0, &bp, &sp, 3 * one_dm, 0, nout, nullptr, b.data(), b.size(), &nb, nullptr,
                                           &nbatch, nullptr, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0]);
    }
    CHECK(steps > 20 && steps < 399 && rows == rows0 && nb == na && memcmp(a.data(), b.data(), (size_t)na * sizeof(frbch_spb_cand)) == 0);
  }
  printf("bands_sanitize: ok\n");
  return 0;
}
