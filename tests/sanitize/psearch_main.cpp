// TEST INFRASTRUCTURE ONLY: the host side of the periodicity search under AddressSanitizer and UBSan, as a stand-alone program
// linked against the emulator sources (CPU only; never loaded into python, never run on a GPU): frbch_psearch_thresholds,
// the step-8 reduction (frbch_psearch_sift) and frbch_ps_group_cands on edge inputs -- no record, one record, all ties, 10^5
// records, capacity errors, refused arguments -- and one small frbch_psearch_host call through the generic kernels.
//   make -C tests/sanitize -f psearch.mk run
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "frbch.h"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static frbch_ps_cand rec(uint32_t dm, uint32_t h, uint32_t k, float H) {
  frbch_ps_cand c;
  memset(&c, 0, sizeof c);
  c.dm_index = dm; c.h = h; c.k = k; c.power = H;
  return c;
}

int main() {
  char err[256];
  const uint32_t n = 1u << 16;
  const double tsamp = 64e-6;
  // thresholds: the whole range of sigma, and what is refused
  float thr[5];
  const double sigmas[] = {1e-6, 0.5, 6.0, 29.999, 30.0};
  for (double sg : sigmas) {
    CHECK(frbch_psearch_thresholds(sg, thr) == FRBCH_OK);
    for (int f = 1; f < 5; ++f) CHECK(thr[f] > thr[f - 1] && thr[f] < 1000.f);
  }
  CHECK(frbch_psearch_thresholds(0.0, thr) == FRBCH_E_ARG && frbch_psearch_thresholds(30.5, thr) == FRBCH_E_ARG);
  CHECK(frbch_psearch_thresholds(NAN, thr) == FRBCH_E_ARG && frbch_psearch_thresholds(6.0, nullptr) == FRBCH_E_ARG);

  uint64_t ncand = 99, ngroup = 99;
  // no record
  CHECK(frbch_psearch_sift(nullptr, 0, n, tsamp, nullptr, 0, &ncand, err, sizeof err) == FRBCH_OK && ncand == 0);
  CHECK(frbch_ps_group_cands(nullptr, 0, 2, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 0);
  // one record; a huge and an infinite power
  {
    std::vector<frbch_ps_cand> raw = {rec(0, 16, 1000, 80.f)}, out(1);
    CHECK(frbch_psearch_sift(raw.data(), 1, n, tsamp, out.data(), 1, &ncand, err, sizeof err) == FRBCH_OK && ncand == 1);
    CHECK(out[0].sigma > 5.0 && out[0].sigma < 20.0 && out[0].freq_hz > 0.0);
    std::vector<frbch_ps_group> g(1);
    CHECK(frbch_ps_group_cands(out.data(), 1, 1, g.data(), 1, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1 && g[0].nmember == 1);
    raw = {rec(0, 1, 5, 3.0e38f), rec(1, 16, 7, INFINITY), rec(2, 8, 9, 0.f), rec(3, 2, 11, 1e-30f)};
    out.resize(4);
    CHECK(frbch_psearch_sift(raw.data(), 4, n, tsamp, out.data(), 4, &ncand, err, sizeof err) == FRBCH_OK && ncand == 4);
    for (const frbch_ps_cand& c : out) CHECK(isfinite(c.sigma) && c.sigma >= 0.0);
  }
  // all ties: 2000 copies of one record in one series (every one survives: none is larger, none comes first), and the same
  // record in 2000 series; capacity errors report the count
  {
    std::vector<frbch_ps_cand> raw(2000, rec(3, 4, 400, 50.f)), out(2000);
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, out.data(), out.size(), &ncand, err, sizeof err) == FRBCH_OK && ncand == 2000);
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, out.data(), 10, &ncand, err, sizeof err) == FRBCH_E_CAPACITY && ncand == 2000);
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, nullptr, 0, &ncand, err, sizeof err) == FRBCH_E_CAPACITY && ncand == 2000);
    std::vector<frbch_ps_group> g(2000);
    CHECK(frbch_ps_group_cands(out.data(), 2000, 2, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1 && g[0].nmember == 2000);
    for (uint32_t i = 0; i < 2000; ++i) raw[i].dm_index = i;
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, out.data(), out.size(), &ncand, err, sizeof err) == FRBCH_OK && ncand == 2000);
    CHECK(frbch_ps_group_cands(out.data(), 2000, 1, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1);
    CHECK(frbch_ps_group_cands(out.data(), 2000, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_CAPACITY && ngroup == 1);
    for (uint32_t i = 0; i < 2000; ++i) raw[i].dm_index = 3 * i;                       // three trials apart: never joined at gap 2
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, out.data(), out.size(), &ncand, err, sizeof err) == FRBCH_OK);
    CHECK(frbch_ps_group_cands(out.data(), 2000, 2, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 2000);
  }
  // 10^5 records over 64 series, every fold, bins all over the spectrum
  {
    const uint32_t folds[5] = {1, 2, 4, 8, 16};
    std::vector<frbch_ps_cand> raw, out(100000);
    for (int i = 0; i < 100000; ++i) raw.push_back(rec(rnd() % 64, folds[rnd() % 5], 1 + rnd() % (n / 2 - 1), 20.f + (float)(rnd() % 1000) * 0.1f));
    CHECK(frbch_psearch_sift(raw.data(), raw.size(), n, tsamp, out.data(), out.size(), &ncand, err, sizeof err) == FRBCH_OK);
    CHECK(ncand > 1000 && ncand <= 100000);
    for (uint64_t i = 1; i < ncand; ++i) CHECK(out[i - 1].dm_index <= out[i].dm_index);
    std::vector<frbch_ps_group> g(ncand);
    CHECK(frbch_ps_group_cands(out.data(), ncand, 2, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup >= 1 && ngroup <= ncand);
    uint64_t members = 0;
    for (uint64_t i = 0; i < ngroup; ++i) { members += g[i].nmember; CHECK(i == 0 || g[i - 1].best.sigma >= g[i].best.sigma); }
    CHECK(members == ncand);
    printf("10^5 raw records: %llu survive, %llu groups\n", (unsigned long long)ncand, (unsigned long long)ngroup);
  }
  // refused arguments
  {
    frbch_ps_cand bad = rec(0, 3, 10, 30.f), out;
    CHECK(frbch_psearch_sift(&bad, 1, n, tsamp, &out, 1, &ncand, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_ps_group_cands(&bad, 1, 2, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
    bad = rec(0, 1, n / 2, 30.f);
    CHECK(frbch_psearch_sift(&bad, 1, n, tsamp, &out, 1, &ncand, err, sizeof err) == FRBCH_E_ARG);
    bad = rec(0, 1, 10, 30.f);
    CHECK(frbch_psearch_sift(&bad, 1, 3000, tsamp, &out, 1, &ncand, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_psearch_sift(&bad, 1, n, 0.0, &out, 1, &ncand, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_ps_group_cands(&bad, 1, 0, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_ps_group_cands(&bad, 1, 17, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
  }
  // one whole call through the generic kernels: three series of 5000 samples, a pulse train in the middle one
  {
    std::vector<float> y(3 * 5000);
    for (float& v : y) v = 100.f + (float)(rnd() % 64);
    for (int t = 7; t < 5000; t += 50) y[5000 + t] += 300.f;
    frbch_ps_params par;
    memset(&par, 0, sizeof par);
    par.size = sizeof par;
    par.sigma = 5.0;
    par.tsamp_s = 1e-3;
    std::vector<frbch_ps_cand> out(4096);
    uint32_t used[2] = {9, 9};
    CHECK(frbch_psearch_host(y.data(), 3, 5000, &par, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_OK);
    CHECK(ncand > 0 && used[0] == 0 && used[1] == 0 && frbch_psearch_nfft(5000, &par) == 4096);
    par.nharm = 3;
    CHECK(frbch_psearch_host(y.data(), 3, 5000, &par, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
  }
  printf("psearch_sanitize: ok\n");
  return 0;
}
