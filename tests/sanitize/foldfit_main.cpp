// TEST INFRASTRUCTURE ONLY: the fold refinement under AddressSanitizer and UBSan, as a stand-alone program linked against the
// emulator sources (CPU only; never loaded into python, never run on a GPU): the generic kernels on a cube that frbch_foldp_host
// made of 8-bit rows with two products (a short last sub-integration, a flagged channel, nbin no power of two, trial profiles
// and the phase-time plane asked for), the host twin against the composite, the peaks alone, the refusals, and a failure walk
// of frbch_fold_refine_host.
//   make -C tests/sanitize -f foldfit.mk run
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
  const uint32_t nchan = 24, nifs = 2, nbin = 50, ndm = 5, nfreq = 7, nfdot = 3;
  const uint64_t nrows = 2300;
  const double f0 = 9.7, subint = 0.5;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1500.0; fil.foff_mhz = -12.5; fil.tsamp_s = 1e-3; fil.tstart_mjd = 59000.0;
  const long nsub_l = frbch_fold_nsub(&fil, nrows, subint);
  CHECK(nsub_l == 5);
  const uint32_t nsub = (uint32_t)nsub_l;

  // rows: noise and a pulse train of the fold frequency plus two bins of drift over the span, dispersed by DM 40
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(90 + rnd() % 13);
  const double kdm = 1.0 / 2.41e-4, T = (double)nrows * fil.tsamp_s;
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t c = 0; c < nchan; ++c) {
      const double f = fil.fch1_mhz + c * fil.foff_mhz;
      const double tt = (double)t * fil.tsamp_s - 40.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz));
      const double ph = (f0 + 2.0 / (nbin * T)) * tt;
      if (ph - floor(ph) < 0.06)
        for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)t * nifs + p) * nchan + c] += 40;
    }
  const std::vector<uint8_t> rows0 = rows;

  frbch_fold_model model;
  memset(&model, 0, sizeof model);
  model.size = sizeof model;
  model.f0_hz = f0; model.pepoch_mjd = fil.tstart_mjd; model.dm = 40.0; model.nbin = nbin; model.subint_s = subint;
  frbch_foldfit_params par;
  memset(&par, 0, sizeof par);
  par.size = sizeof par;
  par.nbin = nbin; par.nsub = nsub; par.products = 3; par.ndm = ndm; par.nfreq = nfreq; par.nfdot = nfdot;
  par.nwidth = 3; par.widths[0] = 1; par.widths[1] = 3; par.widths[2] = 25;
  par.f0_fold = f0; par.subint_s = subint; par.dm0 = 40.0; par.fit_frac = 0.5;
  CHECK(frbch_foldfit_steps(&fil, nrows, nbin, f0, &par.ddm, &par.dfreq, &par.dfdot) == FRBCH_OK);
  CHECK(par.ddm > 0 && par.dfreq > 0 && par.dfdot > 0 && fabs(par.dfreq * nbin * T - 1.0) < 1e-12);
  std::vector<uint8_t> flag(nchan, 0);
  flag[7] = 1;

  const size_t nslot = (size_t)nsub * nbin * nchan, nt = (size_t)ndm * nfdot * nfreq;
  std::vector<double> cube(nslot * nifs), score(nt), score2(nt, 7.0);
  std::vector<uint32_t> chits(nslot);
  std::vector<int64_t> prof(2 * nbin), prof2(2 * nbin), tacc(nt * nbin), plane((size_t)nsub * nbin), plane2((size_t)nsub * nbin);
  std::vector<uint64_t> phits(2 * nbin), phits2(2 * nbin), thits(nt * nbin), plane_hits((size_t)nsub * nbin), plane_hits2((size_t)nsub * nbin);
  frbch_foldfit_result res, res2;
  uint32_t k[3] = {9, 9, 9}, kf = 9;

  // fold, then the search with everything asked for
  CHECK(frbch_foldp_host(&fil, rows.data(), nrows, &model, 0, cube.data(), chits.data(), nsub, &kf, err, sizeof err) == FRBCH_OK && kf == 0);
  CHECK(frbch_foldfit_kernel(&fil, nrows, &par, cube.data(), chits.data(), k) == FRBCH_OK && k[0] == 0 && k[1] == 0);
  CHECK(frbch_foldfit_host(&fil, nrows, &par, cube.data(), chits.data(), flag.data(), 0, score.data(), prof.data(), phits.data(), &res, tacc.data(),
                           thits.data(), plane.data(), plane_hits.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(k[0] == 0 && k[1] == 0);
  // the two profiles are among the trial profiles; the totals of every trial are those of the plane
  const size_t nominal = ((size_t)(ndm / 2) * nfdot + nfdot / 2) * nfreq + nfreq / 2;
  const size_t best = ((size_t)res.kpeak * nfdot + res.jpeak) * nfreq + res.ipeak;
  CHECK(!memcmp(prof.data(), tacc.data() + nominal * nbin, nbin * 8) && !memcmp(prof.data() + nbin, tacc.data() + best * nbin, nbin * 8));
  CHECK(!memcmp(phits.data(), thits.data() + nominal * nbin, nbin * 8) && !memcmp(phits.data() + nbin, thits.data() + best * nbin, nbin * 8));
  int64_t ta = 0, tb = 0;
  uint64_t ha = 0, hb = 0;
  for (size_t i = 0; i < (size_t)nsub * nbin; ++i) { ta += plane[i]; ha += plane_hits[i]; }
  for (uint32_t b = 0; b < nbin; ++b) { tb += tacc[nominal * nbin + b]; hb += thits[nominal * nbin + b]; }
  CHECK(ta == tb && ha == hb && ha == (uint64_t)nrows * (nchan - 1));
  printf("peak (%u, %u, %u) score %.6g (nominal %.6g)  S/N %.2f -> %.2f  dfreq %.6g (%.6g)  dm %.4f\n", res.kpeak, res.jpeak, res.ipeak, res.score_peak,
         res.score_nominal, res.snr_nominal, res.snr_best, res.dfreq, 2.0 / (nbin * T), res.dm);
  CHECK(res.score_peak >= res.score_nominal && res.score_peak == score[best] && res.snr_best > 10.0);
  CHECK(fabs(res.dfreq - 2.0 / (nbin * T)) <= par.dfreq && fabs(res.dm - 40.0) <= par.ddm);

  // the peaks alone
  CHECK(frbch_foldfit_peaks(&par, score.data(), prof.data(), phits.data(), &res2, err, sizeof err) == FRBCH_OK && !memcmp(&res, &res2, sizeof res));

  // the composite: the same bytes, with and without the cube
  std::vector<double> cube2(cube.size());
  std::vector<uint32_t> chits2(nslot);
  CHECK(frbch_fold_refine_host(&fil, rows.data(), nrows, &model, &par, flag.data(), 0, cube2.data(), chits2.data(), score2.data(), prof2.data(),
                               phits2.data(), &res2, plane2.data(), plane_hits2.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(cube2 == cube && chits2 == chits && score2 == score && prof2 == prof && phits2 == phits && plane2 == plane && plane_hits2 == plane_hits);
  CHECK(!memcmp(&res, &res2, sizeof res) && k[0] == 0 && k[1] == 0 && k[2] == 0);
  std::fill(score2.begin(), score2.end(), 7.0);
  CHECK(frbch_fold_refine_host(&fil, rows.data(), nrows, &model, &par, nullptr, 0, nullptr, nullptr, score2.data(), prof2.data(), phits2.data(), &res2,
                               nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_OK && score2 != score);

  // the refusals
  {
    frbch_foldfit_params bad[12];
    for (frbch_foldfit_params& b : bad) b = par;
    bad[0].size = 8; bad[1].ndm = 4; bad[2].nfreq = 0; bad[3].nbin = 4097; bad[4].nsub = nsub + 1; bad[5].products = 0; bad[6].products = 4;
    bad[7].ddm = NAN; bad[8].dfreq = 0.0; bad[9].dm0 = 1.0e5; bad[10].nwidth = 0; bad[11].widths[2] = 26;
    for (const frbch_foldfit_params& b : bad) {
      err[0] = 0;
      std::fill(score2.begin(), score2.end(), 7.0);
      CHECK(frbch_foldfit_host(&fil, nrows, &b, cube.data(), chits.data(), nullptr, 0, score2.data(), prof2.data(), phits2.data(), &res2, nullptr, nullptr,
                               nullptr, nullptr, k, err, sizeof err) == FRBCH_E_ARG && err[0] && score2[0] == 7.0 && score2.back() == 7.0);
      CHECK(frbch_fold_refine_host(&fil, rows.data(), nrows, &model, &b, nullptr, 0, nullptr, nullptr, score2.data(), prof2.data(), phits2.data(), &res2,
                                   nullptr, nullptr, k, err, sizeof err) == FRBCH_E_ARG && score2[0] == 7.0);
      if (&b != &bad[9]) CHECK(frbch_foldfit_kernel(&fil, nrows, &b, cube.data(), chits.data(), k) == FRBCH_E_ARG);
    }
    frbch_fil_desc flt = fil, manych = fil;
    flt.nbits = 32;
    manych.nchan = 16385;
    CHECK(frbch_foldfit_kernel(&flt, nrows, &par, cube.data(), chits.data(), k) == FRBCH_E_ARG);
    CHECK(frbch_foldfit_kernel(&manych, nrows, &par, cube.data(), chits.data(), k) == FRBCH_E_ARG);
    CHECK(frbch_foldfit_kernel(&fil, nrows, &par, nullptr, chits.data(), k) == FRBCH_E_ARG);
    frbch_fold_model delayed = model;
    delayed.apply_delays = 1;
    CHECK(frbch_fold_refine_host(&fil, rows.data(), nrows, &delayed, &par, nullptr, 0, nullptr, nullptr, score2.data(), prof2.data(), phits2.data(), &res2,
                                 nullptr, nullptr, k, err, sizeof err) == FRBCH_E_ARG && strstr(err, "apply_delays"));
    CHECK(frbch_foldfit_host(&fil, nrows, &par, cube.data(), chits.data(), nullptr, 0, score2.data(), prof2.data(), phits2.data(), &res2, tacc.data(),
                             nullptr, nullptr, nullptr, k, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_foldfit_steps(nullptr, nrows, nbin, f0, nullptr, nullptr, nullptr) == FRBCH_E_ARG);
  }

  // the failure walk: every fallible device-layer call fails once; nothing is left behind and no result is written
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long n = 1; n < 300; ++n, ++steps) {
      std::fill(score2.begin(), score2.end(), 7.0);
      frbch_test_emu_fail_at(n);
      err[0] = 0;
      const int rc = frbch_fold_refine_host(&fil, rows.data(), nrows, &model, &par, flag.data(), 0, cube2.data(), chits2.data(), score2.data(), prof2.data(),
                                            phits2.data(), &res2, plane2.data(), plane_hits2.data(), k, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0] && score2[0] == 7.0 && score2.back() == 7.0);
    }
    CHECK(steps > 25 && steps < 299 && rows == rows0 && score2 == score);
  }
  printf("foldfit_sanitize: ok\n");
  return 0;
}
