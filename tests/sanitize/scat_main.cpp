// TEST INFRASTRUCTURE ONLY: the scattering of a burst under AddressSanitizer and UBSan, as a stand-alone program linked against
// the emulator sources (CPU only; never loaded into python, never run on a GPU): the bank, the template-bank stage alone with its
// contract and its window off both ends of the row, the composite through the generic kernels (8-bit rows of 96 channels in
// subbands of 3, bins partly in front of the data and behind it, a candidate wholly outside, flagged and constant channels, a
// subband with no used channel, both product orders, 16-bit rows), the fit alone, the refusals, and a failure walk of
// frbch_burstscat_host.
//   make -C tests/sanitize -f scat.mk run
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
  const uint32_t nchan = 96, nifs = 4, nbin = 40, ffactor = 3, nsub = nchan / ffactor, ncand = 4, shift0 = 0, nshift = nbin;
  const uint32_t nsig = 3, ntau = 4, K = nsig * ntau, ntap = 24, lead = 6;
  const uint64_t nrows = 1500;
  frbch_fil_desc fil;
  memset(&fil, 0, sizeof fil);
  fil.size = sizeof fil;
  fil.nchan = nchan; fil.nifs = nifs; fil.nbits = 8;
  fil.fch1_mhz = 1415.0; fil.foff_mhz = -1.0; fil.tsamp_s = 64e-6; fil.tstart_mjd = 59000.0;
  frbch_burst_params bpar = {sizeof(frbch_burst_params), FRBCH_BURST_STOKES};
  frbch_scat_params par = {sizeof(frbch_scat_params), nbin, 3, ffactor, shift0, nshift, {0, 0}};
  frbch_scat_bank_params bp = {sizeof(frbch_scat_bank_params), nsig, ntau, ntap, lead, {0, 0, 0}, 0.75, 1.5, 0.5, 1.5};
  frbch_scat_fit_params fp;
  memset(&fp, 0, sizeof fp);
  fp.size = sizeof fp; fp.nalpha = 3; fp.snr_min = 3.0; fp.alpha[0] = 0.0; fp.alpha[1] = 2.0; fp.alpha[2] = 4.0;

  // the bank: every output, none, and its refusals
  std::vector<int32_t> p((size_t)K * ntap, 7);
  std::vector<int64_t> s1(K, 7), cum((size_t)K * (ntap + 1), 7);
  std::vector<double> tail(K, 7.0), sigma(nsig, 7.0), tau(ntau, 7.0);
  CHECK(frbch_scat_bank(&bp, p.data(), s1.data(), cum.data(), tail.data(), sigma.data(), tau.data(), err, sizeof err) == FRBCH_OK);
  CHECK(frbch_scat_bank(&bp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == FRBCH_OK);
  for (uint32_t k = 0; k < K; ++k) {
    int64_t s = 0, c = 0;
    int32_t top = 0;
    for (uint32_t m = 0; m < ntap; ++m) { s += p[k * ntap + m]; c += (int64_t)p[k * ntap + m] * p[k * ntap + m]; top = p[k * ntap + m] > top ? p[k * ntap + m] : top; }
    CHECK(s == s1[k] && c == cum[(size_t)k * (ntap + 1) + ntap] && cum[(size_t)k * (ntap + 1)] == 0 && top == 32768 && tail[k] >= 0.0 && tail[k] < 1.0);
  }
  CHECK(sigma[0] == 0.75 && sigma[2] == 0.75 * 1.5 * 1.5 && tau[3] == 0.5 * 1.5 * 1.5 * 1.5);
  {
    frbch_scat_bank_params bads[8] = {bp, bp, bp, bp, bp, bp, bp, bp};
    bads[0].size = 60; bads[1].ntap = 1025; bads[2].lead = ntap; bads[3].nsig = 0; bads[4].ntau = 4097; bads[5].sigma0 = 0.2; bads[6].rtau = 1.0; bads[7].tau0 = NAN;
    for (const frbch_scat_bank_params& b : bads) {
      err[0] = 0;
      p[0] = 7;
      CHECK(frbch_scat_bank(&b, p.data(), nullptr, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG && err[0] && p[0] == 7);
    }
    CHECK(frbch_scat_bank(&bp, p.data(), nullptr, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_OK);
  }

  // the stage alone: a plane and a bank at the contract's edge, more taps than bins, the window off both ends; both forms asked for
  {
    const uint32_t n = 2, ns = 3, nb = 11, nt = 5, tp = 17, ld = 9;
    frbch_tbank_shape sh = {sizeof(frbch_tbank_shape), ns, nb, nt, tp, ld, 0, nb};
    std::vector<int32_t> y((size_t)n * ns * nb), P((size_t)nt * tp);
    for (int32_t& v : y) v = (int32_t)(rnd() % ((1u << 22) + 1)) - (1 << 21);
    for (int32_t& v : P) v = (int32_t)(rnd() % (1u << 24)) * 64 - (1 << 29);
    y[0] = 1 << 21; y.back() = -(1 << 21); P[0] = 1 << 30; P.back() = -(1 << 30);
    std::vector<int64_t> c1((size_t)n * ns * nt * nb, 7), c2 = c1;
    uint32_t ku = 9;
    CHECK(frbch_tbank_kernel(n, &sh, FRBCH_TBANK_PLAN) == 0);
    CHECK(frbch_tbank_host(y.data(), P.data(), n, &sh, FRBCH_TBANK_PLAN, 0, c1.data(), &ku, err, sizeof err) == FRBCH_OK && ku == 0);
    CHECK(frbch_tbank_host(y.data(), P.data(), n, &sh, FRBCH_TBANK_GENERIC, 0, c2.data(), nullptr, nullptr, 0) == FRBCH_OK && c1 == c2);
    for (uint32_t u = 0; u < nb; ++u) {                             // plane 1, subband 2, template 4, by hand
      int64_t want = 0;
      for (uint32_t m = 0; m < tp; ++m) {
        const long j = (long)u - (long)ld + (long)m;
        if (j >= 0 && j < (long)nb) want += (int64_t)y[((size_t)1 * ns + 2) * nb + j] * P[(size_t)4 * tp + m];
      }
      CHECK(c1[(((size_t)1 * ns + 2) * nt + 4) * nb + u] == want);
    }
    y[5] = (1 << 21) + 1;
    std::fill(c1.begin(), c1.end(), 7);
    err[0] = 0;
    CHECK(frbch_tbank_host(y.data(), P.data(), n, &sh, FRBCH_TBANK_PLAN, 0, c1.data(), &ku, err, sizeof err) == FRBCH_E_ARG && err[0] && c1[0] == 7);
    y[5] = 0;
    P[3] = -(1 << 30) - 1;
    CHECK(frbch_tbank_host(y.data(), P.data(), n, &sh, FRBCH_TBANK_PLAN, 0, c1.data(), &ku, err, sizeof err) == FRBCH_E_ARG && c1[0] == 7);
    P[3] = 0;
    CHECK(frbch_tbank_host(nullptr, P.data(), n, &sh, FRBCH_TBANK_PLAN, 0, c1.data(), &ku, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_tbank_host(y.data(), P.data(), n, &sh, 2, 0, c1.data(), &ku, err, sizeof err) == FRBCH_E_ARG);
    frbch_tbank_shape bads[7] = {sh, sh, sh, sh, sh, sh, sh};
    bads[0].size = 28; bads[1].nbin = 1025; bads[2].ntap = 0; bads[3].lead = tp; bads[4].ntemp = 4097; bads[5].nshift = nb + 1; bads[6].nsub = 0;
    for (const frbch_tbank_shape& b : bads) {
      CHECK(frbch_tbank_kernel(n, &b, FRBCH_TBANK_PLAN) == FRBCH_E_ARG);
      CHECK(frbch_tbank_host(y.data(), P.data(), n, &b, FRBCH_TBANK_PLAN, 0, c1.data(), &ku, err, sizeof err) == FRBCH_E_ARG && c1[0] == 7);
    }
    CHECK(frbch_tbank_kernel(0, &sh, FRBCH_TBANK_PLAN) == FRBCH_E_ARG && frbch_tbank_kernel(n, nullptr, FRBCH_TBANK_PLAN) == FRBCH_E_ARG);
  }

  // rows: a floor with noise, a burst of 9 rows at DM 60 in every product; channel 20 is constant
  std::vector<uint8_t> rows((size_t)nrows * nifs * nchan);
  for (uint8_t& v : rows) v = (uint8_t)(100 + rnd() % 7);
  const double kdm = 1.0 / 2.41e-4;
  for (uint32_t c = 0; c < nchan; ++c) {
    const double f = fil.fch1_mhz + c * fil.foff_mhz;
    const long d = (long)(60.0 * kdm * (1.0 / (f * f) - 1.0 / (fil.fch1_mhz * fil.fch1_mhz)) / fil.tsamp_s + 0.5);
    for (long t = 696; t < 705; ++t)
      for (uint32_t q = 0; q < nifs; ++q) rows[((size_t)(t + d) * nifs + q) * nchan + c] += 60;
  }
  for (uint64_t t = 0; t < nrows; ++t)
    for (uint32_t q = 0; q < nifs; ++q) rows[((size_t)t * nifs + q) * nchan + 20] = 100;
  const std::vector<uint8_t> rows0 = rows;
  // the burst; one whose bins begin in front of the data; one wholly outside; one whose bins run off the end
  frbch_burst_cand cands[ncand] = {{60.0, 700, 9, 70, 100, 0}, {60.0, 40, 6, 8, 100, 0}, {60.0, 5000, 4, 8, 100, 0}, {10.0, 1460, 9, 2, 50, 0}};
  std::vector<uint8_t> flag(nchan, 0);
  flag[3] = flag[95] = flag[30] = flag[31] = flag[32] = 1;                  // subband 10 has no used channel
  const size_t ncell = (size_t)ncand * nsub * nbin, nout = (size_t)ncand * nsub * K * nshift;
  std::vector<int64_t> Y(ncell, 7), Cc(nout, 7), Nn(nout, 7);
  std::vector<uint32_t> yhits(ncell, 7);
  std::vector<int32_t> y(ncell, 7);
  std::vector<frbch_scat_sub> sub((size_t)ncand * nsub);
  std::vector<frbch_scat_band> band(ncand);
  std::vector<uint8_t> used((size_t)ncand * nchan, 7);
  uint32_t k[3] = {9, 9, 9};

  CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par, &bp, k) == FRBCH_OK && k[0] == 0 && k[1] == 0 && k[2] == 0);
  CHECK(frbch_burstscat_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &bp, &fp, 0, Y.data(), yhits.data(), y.data(), Cc.data(),
                             Nn.data(), sub.data(), band.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(k[0] == 0 && k[1] == 0 && k[2] == 0 && rows == rows0);
  CHECK(band[0].nused == nchan - 6 && used[3] == 0 && used[31] == 0 && used[20] == 0 && used[9] == 1);
  CHECK(band[0].nfit > 20 && band[0].q > 0.0 && band[0].arrival >= 18.0 && band[0].arrival <= 22.0 && band[0].r > 0);
  CHECK(band[2].nused == 0 && band[2].k == 0 && band[2].nfit == 0 && band[2].q == 0.0);
  CHECK(sub[10].nused == 0 && sub[10].q == 0.0 && sub[0].nused == 3 && sub[1].nused == 2 && sub[0].snr > 3.0);
  for (uint32_t u = 0; u < nshift; ++u) {
    CHECK(Nn[((size_t)10 * K + 0) * nshift + u] == 0 && Cc[((size_t)10 * K + 5) * nshift + u] == 0);       // the empty subband
    CHECK(Nn[((size_t)2 * nsub * K) * nshift + u] == 0);                                                   // the dead candidate
  }
  {                                                                 // a complete row: N is the closed form
    const long j0 = 20 - (long)lead;
    CHECK(Nn[((size_t)0 * K + 3) * nshift + 20] == cum[(size_t)3 * (ntap + 1) + (j0 + (long)ntap <= (long)nbin ? ntap : nbin - j0)] - cum[(size_t)3 * (ntap + 1)]);
    CHECK(Nn[((size_t)0 * K + 3) * nshift + 0] == cum[(size_t)3 * (ntap + 1) + ntap] - cum[(size_t)3 * (ntap + 1) + lead]);
  }
  const std::vector<int64_t> wantC = Cc, wantN = Nn, wantY = Y;

  // the fit alone gives the same records, and q
  {
    int32_t ks[ncand];
    uint32_t rs[ncand], nu[ncand];
    std::vector<uint32_t> nus((size_t)ncand * nsub);
    for (uint32_t i = 0; i < ncand; ++i) { ks[i] = band[i].k; rs[i] = band[i].r; nu[i] = band[i].nused; }
    for (size_t i = 0; i < nus.size(); ++i) nus[i] = sub[i].nused;
    std::vector<double> q(nout, 7.0);
    std::vector<frbch_scat_sub> s2(sub.size());
    std::vector<frbch_scat_band> b2(ncand);
    CHECK(frbch_burstscat_fit(&fil, &par, &bp, &fp, ncand, ks, rs, nu, nus.data(), Cc.data(), Nn.data(), q.data(), s2.data(), b2.data(), err, sizeof err) == FRBCH_OK);
    CHECK(memcmp(s2.data(), sub.data(), sub.size() * sizeof(frbch_scat_sub)) == 0 && memcmp(b2.data(), band.data(), ncand * sizeof(frbch_scat_band)) == 0);
    CHECK(q[(size_t)2 * nsub * K * nshift] == 0.0 && q[((size_t)0 * K + sub[0].k) * nshift + sub[0].u] == sub[0].q);
    CHECK(frbch_burstscat_fit(&fil, &par, &bp, &fp, ncand, ks, rs, nu, nus.data(), Cc.data(), Nn.data(), nullptr, nullptr, nullptr, nullptr, 0) == FRBCH_OK);
    CHECK(frbch_burstscat_fit(&fil, &par, &bp, &fp, ncand, nullptr, rs, nu, nus.data(), Cc.data(), Nn.data(), nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    frbch_scat_fit_params bf = fp;
    bf.nalpha = 33;
    CHECK(frbch_burstscat_fit(&fil, &par, &bp, &bf, ncand, ks, rs, nu, nus.data(), Cc.data(), Nn.data(), nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
  }

  // every output optional; coherency order (every cell complete for one candidate alone: N in closed form); 16-bit rows
  CHECK(frbch_burstscat_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &bp, &fp, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, 0) == FRBCH_OK);
  frbch_burst_params cpar = {sizeof(frbch_burst_params), FRBCH_BURST_COHERENCY};
  CHECK(frbch_burstscat_host(&fil, rows.data(), nrows, &cpar, cands, 1, nullptr, &par, &bp, &fp, 0, Y.data(), yhits.data(), y.data(), Cc.data(), Nn.data(),
                             sub.data(), band.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
  CHECK(band[0].nused == nchan - 1 && Nn[((size_t)6 * K + 3) * nshift + 0] == cum[(size_t)3 * (ntap + 1) + ntap] - cum[(size_t)3 * (ntap + 1) + lead]);
  {
    std::vector<uint16_t> rows16(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) rows16[i] = (uint16_t)(rows[i] * 200);
    frbch_fil_desc f16 = fil;
    f16.nbits = 16;
    CHECK(frbch_burstscat_host(&f16, rows16.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &bp, &fp, 0, Y.data(), yhits.data(), y.data(), Cc.data(),
                               Nn.data(), sub.data(), band.data(), used.data(), k, err, sizeof err) == FRBCH_OK);
    CHECK(Nn == wantN && band[0].nused == nchan - 6);
  }

  // the refusals
  {
    const uint32_t S = sizeof(frbch_scat_params);
    const frbch_scat_params bads[] = {{28, nbin, 3, ffactor, shift0, nshift, {0, 0}}, {S, 0, 3, ffactor, 0, 1, {0, 0}}, {S, 1025, 3, ffactor, shift0, nshift, {0, 0}},
                                      {S, nbin, 0, ffactor, shift0, nshift, {0, 0}}, {S, nbin, 513, ffactor, shift0, nshift, {0, 0}}, {S, nbin, 3, 0, shift0, nshift, {0, 0}},
                                      {S, nbin, 3, 5, shift0, nshift, {0, 0}}, {S, nbin, 3, 97, shift0, nshift, {0, 0}}, {S, nbin, 3, ffactor, shift0, 0, {0, 0}},
                                      {S, nbin, 3, ffactor, 1, nshift, {0, 0}}, {S, nbin, 3, ffactor, nbin + 1, 1, {0, 0}}};
    for (const frbch_scat_params& b : bads) {
      err[0] = 0;
      std::fill(Cc.begin(), Cc.end(), 7);
      CHECK(frbch_burstscat_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &b, &bp, &fp, 0, Y.data(), yhits.data(), y.data(), Cc.data(), Nn.data(),
                                 sub.data(), band.data(), used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && Cc[0] == 7);
      CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &b, &bp, k) == FRBCH_E_ARG);
    }
    frbch_scat_fit_params bf[4] = {fp, fp, fp, fp};
    bf[0].size = 8; bf[1].nalpha = 0; bf[2].alpha[1] = NAN; bf[3].snr_min = INFINITY;
    for (const frbch_scat_fit_params& b : bf) {
      err[0] = 0;
      CHECK(frbch_burstscat_host(&fil, rows.data(), nrows, &bpar, cands, ncand, nullptr, &par, &bp, &b, 0, Y.data(), yhits.data(), y.data(), Cc.data(), Nn.data(),
                                 sub.data(), band.data(), used.data(), k, err, sizeof err) == FRBCH_E_ARG && err[0] && Cc[0] == 7);
    }
    frbch_scat_bank_params bb = bp;
    bb.lead = ntap;
    CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par, &bb, k) == FRBCH_E_ARG);
    frbch_fil_desc two = fil, flt = fil;
    two.nifs = 2;
    flt.nbits = 32;
    CHECK(frbch_burstscat_kernel(&two, rows.data(), nrows, &cpar, cands, ncand, &par, &bp, k) == FRBCH_E_ARG);
    CHECK(frbch_burstscat_kernel(&flt, rows.data(), nrows, &bpar, cands, ncand, &par, &bp, k) == FRBCH_E_ARG);
    CHECK(frbch_burstscat_kernel(&fil, nullptr, nrows, &bpar, cands, ncand, &par, &bp, k) == FRBCH_E_ARG);
    CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, cands, 0, &par, &bp, k) == FRBCH_E_ARG);
    frbch_burst_cand c = cands[0];
    c.width = 0;
    CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, &c, 1, &par, &bp, k) == FRBCH_E_ARG);
    CHECK(frbch_burstscat_kernel(&fil, rows.data(), nrows, &bpar, cands, ncand, &par, &bp, nullptr) == FRBCH_OK);
  }

  // the failure walk: every fallible device-layer call fails once; nothing is left behind and nothing is written
  {
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long n = 1; n < 200; ++n, ++steps) {
      std::fill(Cc.begin(), Cc.end(), 7);
      std::fill(Y.begin(), Y.end(), 7);
      frbch_test_emu_fail_at(n);
      err[0] = 0;
      const int rc = frbch_burstscat_host(&fil, rows.data(), nrows, &bpar, cands, ncand, flag.data(), &par, &bp, &fp, 0, Y.data(), yhits.data(), y.data(),
                                          Cc.data(), Nn.data(), sub.data(), band.data(), used.data(), k, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0] && Cc[0] == 7 && Cc.back() == 7 && Y[0] == 7);
    }
    CHECK(steps > 25 && steps < 199 && rows == rows0 && Cc == wantC && Y == wantY && Nn == wantN);
  }
  printf("scat_sanitize: ok\n");
  return 0;
}
