// TEST INFRASTRUCTURE ONLY: the burst polarisation stage and the polarisation calibration under AddressSanitizer and UBSan,
// as a stand-alone program linked against the emulator sources (CPU only; never loaded into python, never run on a GPU): one
// small call of every entry point through the generic kernels (8-bit and float rows, windows partly and wholly outside the
// data, a masked channel, a dead candidate, the RMSF), the refusals, and a failure walk of the composite.  RM synthesis and
// the delay x RM transform run through one host path (RmFam in frbch_post.cpp), so both members are called here on the same
// data: three trial delays, the one-trial identity with frbch_rmsynth_host byte for byte, the refusals of frbch_rmd_params,
// and the failure walk of frbch_burst_polcal_host.
//   make -C tests/sanitize -f rm.mk run
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
  float dummy_f[2] = {0.f, 0.f};
  const float* dummy = dummy_f;       // frbch_rmsynth_kernel examines the address only
  const uint32_t nchan = 96, nifs = 4, nphi = 129;
  const uint64_t nrows = 1500;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1415.0; fil.foff_mhz = -1.0; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  frbch_burst_params bpar = {sizeof(frbch_burst_params), FRBCH_BURST_STOKES};
  frbch_rm_params rpar = {sizeof(frbch_rm_params), nphi, -6400.0, 100.0};

  // rows: a floor with noise, a burst of 5 rows at DM 60 with a rotating linear polarisation
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
  // the burst; one whose earlier window leaves the data; one wholly outside; one at the very end
  frbch_burst_cand cands[4] = {{60.0, 700, 5, 8, 100, 0}, {60.0, 40, 6, 8, 100, 0}, {60.0, 5000, 4, 8, 100, 0}, {300.0, 1490, 9, 2, 50, 0}};
  const size_t n3 = (size_t)4 * nifs * nchan;
  std::vector<frbch_burst_sums> sums(n3);
  std::vector<float> spec(n3), noise(n3), gain((size_t)nifs * nchan, 1.5f);
  std::vector<uint8_t> used((size_t)4 * nchan);
  uint32_t k1 = 9;

  CHECK(frbch_burstspec_kernel(&fil, rows.data(), nrows, &bpar, cands, 4) == 0);
  CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &bpar, cands, 4, gain.data(), 0, sums.data(), spec.data(), noise.data(), used.data(), &k1,
                             err, sizeof err) == FRBCH_OK);
  CHECK(k1 == 0 && rows == rows0);
  for (uint32_t c = 0; c < nchan; ++c) {
    CHECK(sums[c].on_hits == 5 && sums[c].off_hits == 200 && used[c] == 1 && spec[c] > 60.f && noise[c] > 0.f);
    CHECK(sums[(size_t)1 * nifs * nchan + c].off_hits <= 200 && sums[(size_t)1 * nifs * nchan].off_hits == 129 && used[nchan + c] == 1);
    CHECK(sums[(size_t)2 * nifs * nchan + c].on_hits == 0 && used[2 * nchan + c] == 0 && spec[(size_t)2 * nifs * nchan + c] == 0.f);
  }
  // every output optional; coherency order; float rows
  CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &bpar, cands, 4, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == FRBCH_OK);
  frbch_burst_params cpar = {sizeof(frbch_burst_params), FRBCH_BURST_COHERENCY};
  CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &cpar, cands, 4, nullptr, 0, sums.data(), spec.data(), noise.data(), used.data(), &k1, err,
                             sizeof err) == FRBCH_OK);
  {
    std::vector<float> frows(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) frows[i] = 0.37f * rows[i] - 3.f;
    frows[((size_t)(700) * nifs + 1) * nchan] = NAN;
    frbch_fil_desc ff = fil;
    ff.nbits = 32;
    CHECK(frbch_burstspec_host(&ff, frows.data(), nrows, &bpar, cands, 4, nullptr, 0, sums.data(), spec.data(), noise.data(), used.data(), &k1,
                               err, sizeof err) == FRBCH_OK);
    CHECK(used[0] == 0 && used[1] == 1 && spec[0] == 0.f);
  }

  // the refusals of step 1
  {
    frbch_burst_params bad = bpar;
    bad.size = 4;
    CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &bad, cands, 4, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    bad = bpar;
    bad.products = 2;
    CHECK(frbch_burstspec_kernel(&fil, rows.data(), nrows, &bad, cands, 4) == FRBCH_E_ARG);
    CHECK(frbch_burstspec_kernel(&fil, rows.data(), nrows, &bpar, cands, 0) == FRBCH_E_ARG);
    CHECK(frbch_burstspec_kernel(&fil, rows.data(), nrows, &bpar, cands, 4097) == FRBCH_E_ARG);
    CHECK(frbch_burstspec_kernel(&fil, nullptr, nrows, &bpar, cands, 4) == FRBCH_E_ARG);
    const struct { int field; double v; } cases[] = {{0, 0}, {0, 65537}, {1, 1}, {1, (1 << 20) + 1}, {2, -1.0}, {2, 1.0e5}, {2, NAN}};
    for (const auto& cs : cases) {
      frbch_burst_cand c = cands[0];
      if (cs.field == 0) c.width = (uint32_t)cs.v; else if (cs.field == 1) c.off_len = (uint32_t)cs.v; else c.dm = cs.v;
      CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &bpar, &c, 1, nullptr, 0, sums.data(), nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
      CHECK(err[0]);
    }
    frbch_fil_desc low = fil;
    low.fch1_mhz = 100.0;                                   // 5 .. 100 MHz: the delay passes 2^30 samples
    frbch_burst_cand c = cands[0];
    c.dm = 9.0e4;
    CHECK(frbch_burstspec_host(&low, rows.data(), nrows, &bpar, &c, 1, nullptr, 0, sums.data(), nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    frbch_fil_desc two = fil;
    two.nifs = 2;
    CHECK(frbch_burstspec_kernel(&two, rows.data(), nrows, &cpar, cands, 4) == FRBCH_E_ARG);
  }

  // the table
  {
    std::vector<int32_t> tab(16384);
    CHECK(frbch_rm_table(tab.data()) == FRBCH_OK && frbch_rm_table(nullptr) == FRBCH_E_ARG);
    CHECK(tab[0] == 1 << 22 && tab[4096] == 0 && tab[8192] == -(1 << 22) && tab[12288] == 0 && tab[16383] == tab[1]);
  }

  // step 2 alone: a masked channel holding NaN, a dead candidate, the RMSF
  {
    CHECK(frbch_burstspec_host(&fil, rows.data(), nrows, &bpar, cands, 4, nullptr, 0, sums.data(), spec.data(), noise.data(), used.data(), &k1,
                               err, sizeof err) == FRBCH_OK);
    std::vector<float> q((size_t)4 * nchan), u((size_t)4 * nchan), F((size_t)4 * nphi * 2, 7.f);
    for (uint32_t i = 0; i < 4; ++i)
      for (uint32_t c = 0; c < nchan; ++c) {
        q[(size_t)i * nchan + c] = spec[((size_t)i * nifs + 1) * nchan + c];
        u[(size_t)i * nchan + c] = spec[((size_t)i * nifs + 2) * nchan + c];
      }
    used[17] = 0;
    q[17] = NAN;
    uint32_t k2[2] = {9, 9}, ns = 9;
    CHECK(frbch_rmsynth_kernel(&fil, dummy, 4, &rpar, &ns) == 0 && ns == 1 && frbch_rmsynth_kernel(&fil, nullptr, 4, &rpar, &ns) == FRBCH_E_ARG);
    CHECK(frbch_rmsynth_host(&fil, q.data(), u.data(), used.data(), 4, &rpar, 0, F.data(), k2, err, sizeof err) == FRBCH_OK);
    CHECK(k2[0] == 0 && k2[1] == 1);
    for (uint32_t k = 0; k < nphi; ++k) CHECK(F[((size_t)2 * nphi + k) * 2] == 0.f && F[((size_t)2 * nphi + k) * 2 + 1] == 0.f);
    std::vector<frbch_rm_result> res(4);
    std::vector<float> nq((size_t)4 * nchan, 0.5f);
    CHECK(frbch_rm_peaks(&fil, F.data(), used.data(), nq.data(), nq.data(), 4, &rpar, res.data(), err, sizeof err) == FRBCH_OK);
    CHECK(res[0].fitted == 1 && fabs(res[0].rm - 1500.0) < 100.0 && res[0].nused == nchan - 1 && res[0].snr > 0 && res[0].rm_err > 0);
    CHECK(res[2].nused == 0 && res[2].kpeak == 0 && res[2].fitted == 0 && res[2].peak == 0.0);
    CHECK(frbch_rm_peaks(&fil, F.data(), used.data(), nullptr, nullptr, 4, &rpar, res.data(), err, sizeof err) == FRBCH_OK && res[0].snr == 0.0);
    // the delay x RM transform of the same spectra: three trial delays, of which the second is tau = 0 and so RM synthesis
    {
      const uint32_t ntau = 3;
      const frbch_rmd_params dpar = {sizeof(frbch_rmd_params), nphi, ntau, 0, -6400.0, 100.0, -1.0e-3, 1.0e-3};
      std::vector<float> D((size_t)4 * ntau * nphi * 2, 7.f);
      uint32_t kd[2] = {9, 9};
      ns = 9;
      CHECK(frbch_rmdelay_kernel(&fil, dummy, 4, &dpar, &ns) == 0 && ns == 1 && frbch_rmdelay_kernel(&fil, nullptr, 4, &dpar, &ns) == FRBCH_E_ARG);
      CHECK(frbch_rmdelay_host(&fil, q.data(), u.data(), used.data(), 4, &dpar, 0, D.data(), kd, err, sizeof err) == FRBCH_OK);
      CHECK(kd[0] == 0 && kd[1] == 1);
      for (uint32_t i = 0; i < 4; ++i)
        CHECK(memcmp(&D[((size_t)i * ntau + 1) * nphi * 2], &F[(size_t)i * nphi * 2], (size_t)nphi * 2 * sizeof(float)) == 0);
      std::vector<frbch_rmd_result> dres(5);
      CHECK(frbch_rmdelay_peaks(&fil, D.data(), used.data(), nq.data(), nq.data(), 4, &dpar, dres.data(), err, sizeof err) == FRBCH_OK);
      CHECK(fabs(dres[0].rm - 1500.0) < 100.0 && dres[0].nused == nchan - 1 && dres[0].snr > 0 && dres[0].rm_err > 0 && dres[0].tau_err > 0);
      CHECK(dres[0].sigma_f > 0 && dres[0].fwhm == res[0].fwhm && dres[2].nused == 0 && dres[2].peak == 0.0);
      CHECK(dres[4].nused == 3 && dres[4].sigma_f == 1.0 && dres[4].peak > 0);
      CHECK(frbch_rmdelay_peaks(&fil, D.data(), used.data(), nullptr, nullptr, 4, &dpar, dres.data(), err, sizeof err) == FRBCH_OK);
      CHECK(dres[0].snr == 0.0 && dres[4].nused == 0);
      // ntau = 1, tau_lo = 0: the bytes of frbch_rmsynth_host
      const frbch_rmd_params one_tau = {sizeof(frbch_rmd_params), nphi, 1, 0, -6400.0, 100.0, 0.0, 1.0e-3};
      std::vector<float> E((size_t)4 * nphi * 2, 7.f);
      CHECK(frbch_rmdelay_host(&fil, q.data(), u.data(), used.data(), 4, &one_tau, 0, E.data(), nullptr, err, sizeof err) == FRBCH_OK);
      CHECK(E == F);
    }
    used[17] = 1;
    CHECK(frbch_rmsynth_host(&fil, q.data(), u.data(), used.data(), 4, &rpar, 0, F.data(), k2, err, sizeof err) == FRBCH_E_ARG);
    {
      const frbch_rmd_params dpar = {sizeof(frbch_rmd_params), nphi, 3, 0, -6400.0, 100.0, -1.0e-3, 1.0e-3};
      std::vector<float> D((size_t)4 * 3 * nphi * 2);
      err[0] = 0;
      CHECK(frbch_rmdelay_host(&fil, q.data(), u.data(), used.data(), 4, &dpar, 0, D.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);   // q[17] is NaN
      CHECK(strstr(err, "candidate 0: q or u of a used channel is not finite"));
    }
    // the RMSF: q = used, u = 0 -> exactly 1 at phi = 0 (trial 64)
    std::vector<float> ones((size_t)4 * nchan), zeros((size_t)4 * nchan, 0.f);
    for (size_t i = 0; i < ones.size(); ++i) ones[i] = used[i] ? 1.f : 0.f;
    CHECK(frbch_rmsynth_host(&fil, ones.data(), zeros.data(), used.data(), 4, &rpar, 0, F.data(), nullptr, err, sizeof err) == FRBCH_OK);
    CHECK(F[(size_t)64 * 2] == 1.f && F[(size_t)64 * 2 + 1] == 0.f && F[((size_t)2 * nphi + 64) * 2] == 0.f);
    // one trial; the largest grid is only planned
    frbch_rm_params one = {sizeof(frbch_rm_params), 1, 1500.0, 1.0};
    CHECK(frbch_rmsynth_host(&fil, q.data(), u.data(), used.data(), 1, &one, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);   // q[17] is NaN
    q[17] = 0.f;
    CHECK(frbch_rmsynth_host(&fil, q.data(), u.data(), used.data(), 1, &one, 0, F.data(), nullptr, err, sizeof err) == FRBCH_OK);
    frbch_rm_params big = {sizeof(frbch_rm_params), 1u << 20, -5.0e5, 1.0};
    CHECK(frbch_rmsynth_kernel(&fil, dummy, 64, &big, nullptr) == 0 && frbch_rmsynth_kernel(&fil, dummy, 65, &big, nullptr) == FRBCH_E_ARG);
  }

  // the refusals of step 2
  {
    std::vector<float> q((size_t)nchan, 1.f), F((size_t)nphi * 2);
    std::vector<uint8_t> us(nchan, 1);
    const frbch_rm_params bads[] = {{8, nphi, -6400.0, 100.0}, {sizeof(frbch_rm_params), 0, -6400.0, 100.0}, {sizeof(frbch_rm_params), (1u << 20) + 1, 0.0, 1.0},
                                    {sizeof(frbch_rm_params), nphi, -6400.0, 0.0}, {sizeof(frbch_rm_params), nphi, -6400.0, -1.0},
                                    {sizeof(frbch_rm_params), nphi, -6400.0, INFINITY}, {sizeof(frbch_rm_params), nphi, -6400.0, NAN},
                                    {sizeof(frbch_rm_params), nphi, -1.0001e7, 100.0}, {sizeof(frbch_rm_params), nphi, NAN, 100.0},
                                    {sizeof(frbch_rm_params), nphi, 9.99e6, 100.0}};
    for (const frbch_rm_params& b : bads) {
      err[0] = 0;
      CHECK(frbch_rmsynth_host(&fil, q.data(), q.data(), us.data(), 1, &b, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG && err[0]);
      CHECK(frbch_rmsynth_kernel(&fil, dummy, 1, &b, nullptr) == FRBCH_E_ARG);
    }
    CHECK(frbch_rmsynth_kernel(&fil, dummy, 0, &rpar, nullptr) == FRBCH_E_ARG && frbch_rmsynth_kernel(&fil, dummy, 4097, &rpar, nullptr) == FRBCH_E_ARG);
    frbch_fil_desc wide = fil;
    wide.nchan = 16385;
    wide.foff_mhz = -0.01;
    CHECK(frbch_rmsynth_kernel(&wide, dummy, 1, &rpar, nullptr) == FRBCH_E_ARG);
    frbch_fil_desc neg = fil;
    neg.foff_mhz = -30.0;
    CHECK(frbch_rmsynth_kernel(&neg, dummy, 1, &rpar, nullptr) == FRBCH_E_ARG);
    CHECK(frbch_rmsynth_host(&fil, nullptr, q.data(), us.data(), 1, &rpar, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    // frbch_rmd_params: its size before the file, the phi tests before the tau tests
    const uint32_t sz = sizeof(frbch_rmd_params);
    const struct { frbch_rmd_params p; const char* text; } dbads[] = {
        {{8, nphi, 3, 0, -6400.0, 100.0, 0.0, 1.0e-3}, "frbch_rmd_params: wrong size"},
        {{sz, 0, 3, 0, -6400.0, 100.0, 0.0, 1.0e-3}, "nphi must be 1..2^20"},
        {{sz, nphi, 3, 0, -6400.0, NAN, 0.0, 1.0e-3}, "dphi must be positive and finite"},
        {{sz, nphi, 0, 0, -6400.0, 100.0, 0.0, 1.0e-3}, "ntau must be 1..4096"},
        {{sz, nphi, 4097, 0, -6400.0, 100.0, 0.0, 1.0e-3}, "ntau must be 1..4096"},
        {{sz, 1u << 20, 65, 0, -5.0e5, 1.0, 0.0, 1.0e-3}, "ncand * ntau * nphi exceeds 2^26"},
        {{sz, nphi, 3, 0, -6400.0, 100.0, 0.0, 0.0}, "dtau must be positive and finite"},
        {{sz, nphi, 3, 0, -6400.0, 100.0, 0.0, INFINITY}, "dtau must be positive and finite"},
        {{sz, nphi, 3, 0, -6400.0, 100.0, NAN, 1.0e-3}, "|tau| above 100 microseconds"},
        {{sz, nphi, 3, 0, -6400.0, 100.0, 99.9, 0.1}, "|tau| above 100 microseconds"}};
    for (const auto& b : dbads) {
      err[0] = 0;
      CHECK(frbch_rmdelay_host(&fil, q.data(), q.data(), us.data(), 1, &b.p, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG && strstr(err, b.text));
      CHECK(frbch_rmdelay_kernel(&fil, dummy, 1, &b.p, nullptr) == FRBCH_E_ARG);
    }
    err[0] = 0;
    CHECK(frbch_rmdelay_host(&wide, q.data(), q.data(), us.data(), 1, &dbads[0].p, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(strstr(err, "frbch_rmd_params: wrong size"));                                   // (not "more than 16384 channels")
    CHECK(frbch_rmdelay_host(&fil, q.data(), q.data(), us.data(), 1, nullptr, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    const frbch_rmd_params good = {sz, nphi, 3, 0, -6400.0, 100.0, 0.0, 1.0e-3};
    CHECK(frbch_rmdelay_host(&fil, nullptr, q.data(), us.data(), 1, &good, 0, F.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
  }

  // the composite, a flagged channel, and its failure walk: every fallible device-layer call fails once; nothing is left behind
  {
    std::vector<float> F((size_t)4 * nphi * 2), want;
    std::vector<frbch_rm_result> res(4);
    std::vector<uint8_t> flag(nchan, 0);
    flag[3] = flag[95] = 1;
    uint32_t k3[3] = {9, 9, 9};
    CHECK(frbch_burst_rm_host(&fil, rows.data(), nrows, &bpar, cands, 4, gain.data(), flag.data(), &rpar, 0, spec.data(), noise.data(), used.data(),
                              F.data(), res.data(), k3, err, sizeof err) == FRBCH_OK);
    CHECK(k3[0] == 0 && k3[1] == 0 && k3[2] == 1 && used[3] == 0 && used[95] == 0 && used[4] == 1 && res[0].nused == nchan - 2);
    CHECK(res[0].fitted == 1 && fabs(res[0].rm - 1500.0) < 100.0 && res[2].nused == 0 && rows == rows0);
    want = F;
    frbch_fil_desc two = fil;
    two.nifs = 2;
    CHECK(frbch_burst_rm_host(&two, rows.data(), nrows, &bpar, cands, 4, nullptr, nullptr, &rpar, 0, spec.data(), noise.data(), used.data(), F.data(),
                              res.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_burst_rm_host(&fil, rows.data(), nrows, &bpar, cands, 4, nullptr, nullptr, &rpar, 0, spec.data(), noise.data(), used.data(), nullptr,
                              res.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long k = 1; k < 200; ++k, ++steps) {
      frbch_test_emu_fail_at(k);
      err[0] = 0;
      const int rc = frbch_burst_rm_host(&fil, rows.data(), nrows, &bpar, cands, 4, gain.data(), flag.data(), &rpar, 0, spec.data(), noise.data(),
                                         used.data(), F.data(), res.data(), k3, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0]);
    }
    CHECK(steps > 10 && steps < 199 && rows == rows0 && F == want);
  }

  // the same for the composite of the delay family (one more result record: the combined estimate)
  {
    const uint32_t ntau = 3;
    const frbch_rmd_params dpar = {sizeof(frbch_rmd_params), nphi, ntau, 0, -6400.0, 100.0, -1.0e-3, 1.0e-3};
    std::vector<float> F((size_t)4 * ntau * nphi * 2), want;
    std::vector<frbch_rmd_result> res(5);
    std::vector<uint8_t> flag(nchan, 0);
    flag[3] = flag[95] = 1;
    uint32_t k3[3] = {9, 9, 9};
    CHECK(frbch_burst_polcal_host(&fil, rows.data(), nrows, &bpar, cands, 4, gain.data(), flag.data(), &dpar, 0, spec.data(), noise.data(),
                                  used.data(), F.data(), res.data(), k3, err, sizeof err) == FRBCH_OK);
    CHECK(k3[0] == 0 && k3[1] == 0 && k3[2] == 1 && used[3] == 0 && used[95] == 0 && used[4] == 1 && res[0].nused == nchan - 2);
    CHECK(fabs(res[0].rm - 1500.0) < 100.0 && res[2].nused == 0 && res[4].nused >= 1 && res[4].nused <= 3 && rows == rows0);
    want = F;
    frbch_fil_desc two = fil;
    two.nifs = 2;
    CHECK(frbch_burst_polcal_host(&two, rows.data(), nrows, &bpar, cands, 4, nullptr, nullptr, &dpar, 0, spec.data(), noise.data(), used.data(),
                                  F.data(), res.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_burst_polcal_host(&fil, rows.data(), nrows, &bpar, cands, 4, nullptr, nullptr, &dpar, 0, spec.data(), noise.data(), used.data(),
                                  nullptr, res.data(), nullptr, err, sizeof err) == FRBCH_E_ARG);
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long k = 1; k < 200; ++k, ++steps) {
      frbch_test_emu_fail_at(k);
      err[0] = 0;
      const int rc = frbch_burst_polcal_host(&fil, rows.data(), nrows, &bpar, cands, 4, gain.data(), flag.data(), &dpar, 0, spec.data(), noise.data(),
                                             used.data(), F.data(), res.data(), k3, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0]);
    }
    CHECK(steps > 10 && steps < 199 && rows == rows0 && F == want);
  }
  printf("rm_sanitize: ok\n");
  return 0;
}
