// TEST INFRASTRUCTURE ONLY: the structure of a burst under AddressSanitizer and UBSan, as a stand-alone program linked against
// the emulator sources (CPU only; never loaded into python, never run on a GPU): the composite through the generic kernels
// (8-bit rows of 96 channels in subbands of 3, bins partly in front of the data and behind it, a candidate wholly outside, flagged
// and constant channels, a subband with no used channel, both product orders, full lags, 16-bit rows), the ACF stage alone with
// its contract, the fit alone, the refusals, and a failure walk of frbch_burstacf_host.
//   make -C tests/sanitize -f acf.mk run
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
  const uint32_t nchan = 96, nifs = 4, nbin = 40, ffactor = 3, nsub = nchan / ffactor, nlagf = nsub, nlagt = nbin, ndt = 2 * nlagt - 1, ncand = 4;
  const uint64_t nrows = 1500;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1415.0; fil.foff_mhz = -1.0; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  frbch_burst_params bpar = {sizeof(frbch_burst_params), FRBCH_BURST_STOKES};
  frbch_acf_params par = {sizeof(frbch_acf_params), nbin, 3, ffactor, nlagf, nlagt, {0, 0}};
  frbch_acf_fit_params fp = {sizeof(frbch_acf_fit_params), 0, 0.5};

  // rows: a floor with noise, a burst of 9 rows at DM 60 in every product; channel 20 is constant
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(100 + rnd() % 7);
  const double kdm = 1.0 / 2.41e-4;
  for (uint32_t c = 0; c < nchan; ++c) {
    const double f = fil.fch1_mhz + c * fil.foff_mhz;
    const long d = (long)(60.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz)) / fil.tsamp_s + 0.5);
    for (long t = 696; t < 705; ++t)
      for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)(t + d) * nifs + p) * nchan + c] += 60;
  }
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t p = 0; p < nifs; ++p) rows[((size_t)t * nifs + p) * nchan + 20] = 100;
  const std::vector<uint8_t> rows0 = rows;
  // the burst; one whose bins begin in front of the data; one wholly outside; one whose bins run off the end
  frbch_burst_cand cands[ncand] = {{60.0, 700, 9, 70, 100, 0}, {60.0, 40, 6, 8, 100, 0}, {60.0, 5000, 4, 8, 100, 0}, {10.0, 1460, 9, 2, 50, 0}};
  std::vector<uint8_t> flag(nchan, 0);
  flag[3] = flag[95] = flag[30] = flag[31] = flag[32] = 1;                  // subband 10 has no used channel
  const size_t ncell = (size_t)ncand * nsub * nbin, nlag = (size_t)ncand * nlagf * ndt;
  std::vector<int64_t> Y(ncell, 7), A(nlag, 7);
  std::vector<uint32_t> yhits(ncell, 7), P(nlag, 7);
  std::vector<frbch_acf_result> res(ncand);
  std::vector<uint8_t> used((size_t)ncand * nchan, 7);
  uint32_t k[3] = {9, 9, 9};

  CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par, k) == FRBCH_OK && k[0] == 0 && k[1] == 0 && k[2] == 0);
  CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &fp, 0, Y.data(), yhits.data(), A.data(), P.data(),
                            res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(k[0] == 0 && k[1] == 0 && k[2] == 0 && rows == rows0);
  CHECK(res[0].nused == nchan - 6 && used[3] == 0 && used[31] == 0 && used[20] == 0 && used[9] == 1);
  CHECK(res[0].ncomplete == (nsub - 1) * nbin && res[0].r > 0 && res[0].ref > 0.0 && res[0].fitted_t == 1);
  CHECK(res[2].nused == 0 && res[2].k == 0 && res[2].ncomplete == 0 && res[2].ref == 0.0);
  CHECK(res[1].ncomplete > 0 && res[1].ncomplete < res[0].ncomplete && res[3].ncomplete < res[0].ncomplete);
  for (uint32_t j = 0; j < nbin; ++j) {
    CHECK(yhits[(size_t)10 * nbin + j] == 0 && Y[(size_t)10 * nbin + j] == 0);                    // the empty subband
    CHECK(yhits[(size_t)0 * nbin + j] == 3 * 3 && yhits[(size_t)1 * nbin + j] == 3 * 2);          // channel 3 is flagged
    CHECK(yhits[((size_t)2 * nsub + 5) * nbin + j] == 0);
  }
  CHECK(P[(size_t)0 * ndt + nlagt - 1] == res[0].ncomplete && A[(size_t)0 * ndt + nlagt - 1] > 0);
  CHECK(P[(size_t)(nlagf - 1) * ndt + 0] == 1 && P[(size_t)(nlagf - 1) * ndt + ndt - 1] == 1);    // the corner lags: one pair each
  for (uint32_t x = 0; x < ndt; ++x) CHECK(A[x] == A[ndt - 1 - x] && P[x] == P[ndt - 1 - x]);
  const std::vector<int64_t> wantA = A, wantY = Y;
  const std::vector<uint32_t> wantP = P;

  // the fit alone gives the same results, and norm
  {
    int32_t ks[ncand];
    uint32_t rs[ncand], nu[ncand], nc[ncand];
    for (uint32_t i = 0; i < ncand; ++i) { ks[i] = res[i].k; rs[i] = res[i].r; nu[i] = res[i].nused; nc[i] = res[i].ncomplete; }
    std::vector<double> norm(nlag, 7.0);
    std::vector<frbch_acf_result> r2(ncand);
    CHECK(frbch_burstacf_fit(&fil, &par, &fp, ncand, ks, rs, nu, nc, A.data(), P.data(), norm.data(), r2.data(), err, sizeof err) == FRBCH_OK);
    CHECK(memcmp(r2.data(), res.data(), ncand * sizeof(frbch_acf_result)) == 0 && norm[(size_t)2 * nlagf * ndt] == 0.0 && norm[nlagt - 1] > 0.0);
    CHECK(frbch_burstacf_fit(&fil, &par, &fp, ncand, ks, rs, nu, nc, A.data(), P.data(), nullptr, nullptr, nullptr, 0) == FRBCH_OK);
    CHECK(frbch_burstacf_fit(&fil, &par, &fp, ncand, nullptr, rs, nu, nc, A.data(), P.data(), nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    frbch_acf_fit_params bf = fp;
    bf.fit_frac = 0.0;
    CHECK(frbch_burstacf_fit(&fil, &par, &bf, ncand, ks, rs, nu, nc, A.data(), P.data(), nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
  }

  // the ACF stage alone: a plane at the contract's edge, both forms asked for; a plane beyond it
  {
    const uint32_t n = 2, ns = 7, nb = 11, lf = 7, lt = 11;
    std::vector<int32_t> y((size_t)n * ns * nb);
    for (int32_t& v : y) v = (int32_t)(rnd() % ((1u << 22) + 1)) - (1 << 21);
    y[0] = 1 << 21;
    y.back() = -(1 << 21);
    std::vector<int64_t> a1((size_t)n * lf * (2 * lt - 1), 7), a2 = a1;
    uint32_t ku = 9;
    CHECK(frbch_acf2d_kernel(n, ns, nb, lf, lt, FRBCH_ACF_PLAN) == 0 && frbch_acf2d_kernel(n, ns, nb, lf + 1, lt, FRBCH_ACF_PLAN) == FRBCH_E_ARG);
    CHECK(frbch_acf2d_host(y.data(), n, ns, nb, lf, lt, FRBCH_ACF_PLAN, 0, a1.data(), &ku, err, sizeof err) == FRBCH_OK && ku == 0);
    CHECK(frbch_acf2d_host(y.data(), n, ns, nb, lf, lt, FRBCH_ACF_GENERIC, 0, a2.data(), nullptr, nullptr, 0) == FRBCH_OK && a1 == a2);
    int64_t sq = 0;
    for (size_t i = 0; i < (size_t)ns * nb; ++i) sq += (int64_t)y[i] * y[i];
    CHECK(a1[lt - 1] == sq && a1[(size_t)(lf - 1) * (2 * lt - 1)] == (int64_t)y[nb - 1] * y[(size_t)(ns - 1) * nb]);
    y[5] = (1 << 21) + 1;
    std::fill(a1.begin(), a1.end(), 7);
    err[0] = 0;
    CHECK(frbch_acf2d_host(y.data(), n, ns, nb, lf, lt, FRBCH_ACF_PLAN, 0, a1.data(), &ku, err, sizeof err) == FRBCH_E_ARG && err[0] && a1[0] == 7);
    CHECK(frbch_acf2d_host(nullptr, n, ns, nb, lf, lt, FRBCH_ACF_PLAN, 0, a1.data(), &ku, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_acf2d_host(y.data(), n, ns, nb, lf, lt, 2, 0, a1.data(), &ku, err, sizeof err) == FRBCH_E_ARG);
  }

  // every output optional; coherency order; one subband and one bin of 256 rows; 16-bit rows
  CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &fp, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, 0) == FRBCH_OK);
  frbch_burst_params cpar = {sizeof(frbch_burst_params), FRBCH_BURST_COHERENCY};
  CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &cpar, cands, ncand, nullptr, &par, &fp, 0, Y.data(), yhits.data(), A.data(), P.data(), res.data(),
                            used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(res[0].nused == nchan - 1 && res[0].ncomplete == nsub * nbin);
  {
    frbch_acf_params one = {sizeof(frbch_acf_params), 1, 256, nchan, 1, 1, {0, 0}};
    CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, 1, nullptr, &one, &fp, 0, Y.data(), yhits.data(), A.data(), P.data(), res.data(),
                              used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(P[0] == 1 && yhits[0] == 256 * (nchan - 1) && res[0].fitted_d == 0 && res[0].fitted_f == 0 && A[0] > 0);
    std::vector<uint16_t> rows16(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows16[i] = (uint16_t)(rows[i] * 200);
    frbch_fil_desc f16 = fil;
    f16.nbits = 16;
    CHECK(frbch_burstacf_host(&f16, rows16.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &fp, 0, Y.data(), yhits.data(), A.data(), P.data(),
                              res.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(P == wantP && res[0].nused == nchan - 6);
  }

  // the refusals
  {
    const uint32_t S = sizeof(frbch_acf_params);
    const frbch_acf_params bads[] = {{28, nbin, 3, ffactor, nlagf, nlagt, {0, 0}}, {S, 0, 3, ffactor, nlagf, 1, {0, 0}}, {S, 1025, 3, ffactor, nlagf, nlagt, {0, 0}},
                                     {S, nbin, 0, ffactor, nlagf, nlagt, {0, 0}}, {S, nbin, 513, ffactor, nlagf, nlagt, {0, 0}}, {S, nbin, 3, 0, nlagf, nlagt, {0, 0}},
                                     {S, nbin, 3, 5, nlagf, nlagt, {0, 0}}, {S, nbin, 3, 97, nlagf, nlagt, {0, 0}}, {S, nbin, 3, ffactor, 0, nlagt, {0, 0}},
                                     {S, nbin, 3, ffactor, nlagf + 1, nlagt, {0, 0}}, {S, nbin, 3, ffactor, nlagf, 0, {0, 0}},
                                     {S, nbin, 3, ffactor, nlagf, nlagt + 1, {0, 0}}, {S, 1024, 1, 1, 1, 257, {0, 0}}};
    for (const frbch_acf_params& b : bads) {
      err[0] = 0;
      std::fill(A.begin(), A.end(), 7);
      CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &b, &fp, 0, Y.data(), yhits.data(), A.data(), P.data(), res.data(),
                                used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && A[0] == 7);
      CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &b, k) == FRBCH_E_ARG);
    }
    frbch_acf_fit_params bf[3] = {fp, fp, fp};
    bf[0].size = 8; bf[1].fit_frac = 1.0; bf[2].fit_frac = NAN;
    for (const frbch_acf_fit_params& b : bf) {
      err[0] = 0;
      CHECK(frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &b, 0, Y.data(), yhits.data(), A.data(), P.data(), res.data(),
                                used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && A[0] == 7);
    }
    frbch_fil_desc two = fil, flt = fil;
    two.nifs = 2;
    flt.nbits = 32;
    CHECK(frbch_burstacf_kernel(&two, rows.data(), nrows, &cpar, cands, ncand, &par, k) == FRBCH_E_ARG);
    CHECK(frbch_burstacf_kernel(&flt, rows.data(), nrows, &bpar, cands, ncand, &par, k) == FRBCH_E_ARG);
    CHECK(frbch_burstacf_kernel(&fil, nullptr, nrows, &bpar, cands, ncand, &par, k) == FRBCH_E_ARG);
    CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, cands, 0, &par, k) == FRBCH_E_ARG);
    CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, cands, 4097, &par, k) == FRBCH_E_ARG);
    frbch_burst_cand c = cands[0];
    c.width = 0;
    CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, &c, 1, &par, k) == FRBCH_E_ARG);
    CHECK(frbch_burstacf_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par, nullptr) == FRBCH_OK);
  }

  // the failure walk: every fallible device-layer call fails once; nothing is left behind and nothing is written
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long n = 1; n < 200; ++n, ++steps) {
      std::fill(A.begin(), A.end(), 7);
      std::fill(Y.begin(), Y.end(), 7);
      frbch_test_emu_fail_at(n);
      err[0] = 0;
      const int rc = frbch_burstacf_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &fp, 0, Y.data(), yhits.data(), A.data(),
                                         P.data(), res.data(), used.data(), k, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0] && A[0] == 7 && A.back() == 7 && Y[0] == 7);
    }
    CHECK(steps > 25 && steps < 199 && rows == rows0 && A == wantA && Y == wantY && P == wantP);
  }
  printf("acf_sanitize: ok\n");
  return 0;
}
