// TEST INFRASTRUCTURE ONLY: the acceleration search under AddressSanitizer and UBSan, as a stand-alone program linked against
// the emulator sources (CPU only; never loaded into python, never run on a GPU): frbch_pasearch_plan, the refusals, the
// resampler at the edge of its range and with a tail beyond n, a small frbch_pasearch_host call through the generic kernels with
// an odd number of series and every batch size, a failure walk, and frbch_pa_group_cands on edge inputs.
//   make -C tests/sanitize -f accel.mk run
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

static frbch_pa_cand rec(uint32_t dm, uint32_t acc, uint32_t h, uint32_t k, double sigma) {
  frbch_pa_cand c;
  memset(&c, 0, sizeof c);
  c.dm_index = dm; c.acc_index = acc; c.h = h; c.k = k; c.power = 30.f; c.sigma = sigma;
  return c;
}

int main() {
  char err[512];
  const uint32_t n = 4096;
  const double tsamp = 1e-3, c_light = 299792458.0;
  frbch_ps_params par;
  memset(&par, 0, sizeof par);
  par.size = sizeof par;
  par.sigma = 4.0;
  par.tsamp_s = tsamp;

  // the plan
  {
    uint32_t pn = 0, rows = 0, nb = 0;
    uint64_t bytes = 0;
    CHECK(frbch_pasearch_plan(3, 5000, &par, 5, 0, &pn, &rows, &nb, &bytes, err, sizeof err) == FRBCH_OK);
    CHECK(pn == n && rows == 20 && nb == 1 && bytes > (uint64_t)rows * 10 * n);
    CHECK(frbch_pasearch_plan(3, 5000, &par, 5, 1, &pn, &rows, &nb, nullptr, err, sizeof err) == FRBCH_OK && rows == 4 && nb == 5);
    CHECK(frbch_pasearch_plan(3, 5000, &par, 5, 9, nullptr, &rows, &nb, nullptr, nullptr, 0) == FRBCH_OK && rows == 8 && nb == 3);
    CHECK(frbch_pasearch_plan(65534, 1u << 22, &par, 1024, 0, &pn, &rows, &nb, &bytes, err, sizeof err) == FRBCH_OK);
    CHECK(pn == (1u << 22) && rows == 65534 && nb == 1024);
    CHECK(frbch_pasearch_plan(65535, 5000, &par, 5, 0, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_plan(0, 5000, &par, 5, 0, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_plan(3, 5000, &par, 0, 0, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_plan(3, 5000, &par, 1025, 0, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_plan(3, 4000, &par, 5, 0, nullptr, nullptr, nullptr, nullptr, err, sizeof err) == FRBCH_E_ARG);
  }

  std::vector<float> y(3 * 5000);
  for (float& v : y) v = 100.f + (float)(rnd() % 64);
  for (int t = 7; t < 4096; t += 50) y[5000 + t] += 300.f;
  for (int d = 0; d < 3; ++d)
    for (int t = 4096; t < 5000; ++t) y[(size_t)d * 5000 + t] = 1.0e6f;
  const std::vector<float> y0 = y;
  // the largest accepted trial (q n <= 0.5 in the library's arithmetic) and the first double beyond it
  double edge = c_light / ((double)n * tsamp);
  while (fabs((edge * tsamp) / (2.0 * 299792458.0)) * (double)n > 0.5) edge = nextafter(edge, 0.0);
  const double beyond = nextafter(edge, INFINITY);

  // the resampler: both edges, zero, a tail of 1e6 beyond n that no output may hold
  {
    const double accs[5] = {-edge, -1.0e7, 0.0, 1.0e7, edge};
    std::vector<float> out((size_t)5 * 3 * n, -1.f);
    uint32_t used = 9;
    CHECK(frbch_resample_host(y.data(), 3, 5000, n, tsamp, accs, 5, 0, out.data(), &used, err, sizeof err) == FRBCH_OK && used == 0);
    for (float v : out) CHECK(v >= 100.f && v < 1000.f);
    for (int d = 0; d < 3; ++d) {
      CHECK(memcmp(&out[((size_t)2 * 3 + d) * n], &y[(size_t)d * 5000], n * sizeof(float)) == 0);        // a = 0: the series itself
      for (int i = 0; i < 5; ++i) {
        CHECK(out[((size_t)i * 3 + d) * n] == y[(size_t)d * 5000]);                                         // u(0) = 0
        CHECK(out[((size_t)i * 3 + d) * n + n - 1] == y[(size_t)d * 5000 + n - 1]);                         // u(n - 1) = n - 1
      }
    }
    CHECK(frbch_resample_host(y.data(), 3, 5000, 8192, tsamp, accs, 5, 0, out.data(), &used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_resample_host(y.data(), 3, 5000, n, 0.0, accs, 5, 0, out.data(), &used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_resample_host(y.data(), 3, 5000, n, tsamp, accs, 0, 0, out.data(), &used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_resample_host(nullptr, 3, 5000, n, tsamp, accs, 5, 0, out.data(), &used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_resample_kernel(y.data(), 5000, out.data()) == 0 && frbch_resample_kernel(nullptr, 5000, out.data()) == FRBCH_E_ARG);
  }

  // the refusals of the search
  std::vector<frbch_pa_cand> out(8192);
  uint64_t ncand = 99;
  uint32_t used[3] = {9, 9, 9};
  {
    const double unsorted[2] = {1.0, 0.0}, twice[2] = {1.0, 1.0}, nan_[2] = {0.0, NAN}, inf_[2] = {0.0, INFINITY}, far[2] = {0.0, beyond},
                 nfar[2] = {-beyond, 0.0}, ok[2] = {-edge, edge};
    for (const double* a : {unsorted, twice, nan_, inf_, far, nfar}) {
      err[0] = 0;
      CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, a, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG && err[0]);
    }
    CHECK(strstr(err, "the largest is") != nullptr);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, ok, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_OK);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, ok, 0, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, ok, 1025, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, nullptr, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
    CHECK(frbch_pasearch_host(y.data(), 65535, 5000, &par, ok, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
    frbch_ps_params bad = par;
    bad.size -= 8;
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &bad, ok, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
    bad = par;
    bad.nharm = 3;
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &bad, ok, 2, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_E_ARG);
  }

  // a small search: three series (an odd count: a pad row per trial), five trials, every batch size gives the same bytes; trial
  // a = 0 gives the records of frbch_psearch_host
  {
    const double accs[5] = {-2.0e5, -1.0e5, 0.0, 1.0e5, 2.0e5};
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, 0, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_OK);
    CHECK(ncand > 0 && ncand <= out.size() && used[0] == 0 && used[1] == 0 && used[2] == 0);
    const uint64_t want_n = ncand;
    const std::vector<frbch_pa_cand> want(out.begin(), out.begin() + (long)want_n);
    for (uint64_t i = 1; i < want_n; ++i) CHECK(want[i - 1].acc_index <= want[i].acc_index);
    for (uint32_t rows = 1; rows <= 21; ++rows) {
      CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, rows, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_OK);
      CHECK(ncand == want_n && memcmp(out.data(), want.data(), want_n * sizeof(frbch_pa_cand)) == 0);
    }
    std::vector<frbch_ps_cand> plain(4096);
    uint64_t nplain = 0;
    uint32_t u2[2];
    CHECK(frbch_psearch_host(y.data(), 3, 5000, &par, 0, plain.data(), plain.size(), &nplain, u2, err, sizeof err) == FRBCH_OK && nplain > 0);
    uint64_t j = 0;
    for (const frbch_pa_cand& c : want) {
      if (c.acc_index != 2) continue;
      CHECK(j < nplain && c.dm_index == plain[j].dm_index && c.h == plain[j].h && c.k == plain[j].k && c.power == plain[j].power &&
            c.sigma == plain[j].sigma && c.freq_hz == plain[j].freq_hz && c.acc_ms2 == 0.0);
      ++j;
    }
    CHECK(j == nplain);
    // capacity
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, 0, 0, out.data(), 1, &ncand, used, err, sizeof err) == FRBCH_E_CAPACITY && ncand == want_n);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, 0, 0, nullptr, 0, &ncand, used, err, sizeof err) == FRBCH_E_CAPACITY && ncand == want_n);
    // the failure walk: every fallible device-layer call fails once; nothing is left behind, the input stays, a plain call follows
    const uint64_t live = frbch_test_emu_live();
    int steps = 0;
    for (long k = 1; k < 400; ++k, ++steps) {
      frbch_test_emu_fail_at(k);
      err[0] = 0;
      const int rc = frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, 8, 0, out.data(), out.size(), &ncand, used, err, sizeof err);
      frbch_test_emu_fail_at(0);
      CHECK(frbch_test_emu_live() == live);
      if (rc == FRBCH_OK) break;
      CHECK(rc < 0 && err[0]);
    }
    CHECK(steps > 30 && steps < 399 && y == y0);
    CHECK(frbch_pasearch_host(y.data(), 3, 5000, &par, accs, 5, 8, 0, out.data(), out.size(), &ncand, used, err, sizeof err) == FRBCH_OK);
    CHECK(ncand == want_n && memcmp(out.data(), want.data(), want_n * sizeof(frbch_pa_cand)) == 0);
    printf("small search: %llu records, failure walk of %d steps\n", (unsigned long long)want_n, steps);
  }

  // grouping: no record, one record, a chain through a middle trial, all ties, 10^5 records, refused arguments
  {
    uint64_t ngroup = 99;
    CHECK(frbch_pa_group_cands(nullptr, 0, 2, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 0);
    std::vector<frbch_pa_cand> c = {rec(0, 0, 1, 100, 7.0), rec(0, 1, 1, 101, 8.0), rec(0, 2, 1, 102, 9.0)};
    std::vector<frbch_pa_group> g(3);
    CHECK(frbch_pa_group_cands(c.data(), 1, 2, 1, g.data(), 1, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1 && g[0].nmember == 1);
    CHECK(frbch_pa_group_cands(c.data(), 3, 2, 1, g.data(), 3, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1);
    CHECK(g[0].nmember == 3 && g[0].best.k == 102 && g[0].acc_index_lo == 0 && g[0].acc_index_hi == 2);
    c.erase(c.begin() + 1);                                                        // without the middle trial: two groups
    CHECK(frbch_pa_group_cands(c.data(), 2, 2, 1, g.data(), 3, &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 2);
    CHECK(frbch_pa_group_cands(c.data(), 2, 2, 1, g.data(), 1, &ngroup, err, sizeof err) == FRBCH_E_CAPACITY && ngroup == 2);
    CHECK(frbch_pa_group_cands(c.data(), 2, 2, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_CAPACITY && ngroup == 2);
    std::vector<frbch_pa_cand> ties(2000, rec(3, 4, 4, 400, 7.0));
    g.resize(2000);
    CHECK(frbch_pa_group_cands(ties.data(), 2000, 1, 1, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1 && g[0].nmember == 2000);
    for (uint32_t i = 0; i < 2000; ++i) ties[i].acc_index = 2 * i;                  // two trials apart: never joined at gap 1
    CHECK(frbch_pa_group_cands(ties.data(), 2000, 1, 1, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 2000);
    CHECK(frbch_pa_group_cands(ties.data(), 2000, 1, 2, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup == 1);
    const uint32_t folds[5] = {1, 2, 4, 8, 16};
    std::vector<frbch_pa_cand> many;
    for (int i = 0; i < 100000; ++i) many.push_back(rec(rnd() % 64, rnd() % 33, folds[rnd() % 5], 1 + rnd() % 32767, 5.0 + (double)(rnd() % 1000) * 0.01));
    g.resize(many.size());
    CHECK(frbch_pa_group_cands(many.data(), many.size(), 2, 1, g.data(), g.size(), &ngroup, err, sizeof err) == FRBCH_OK && ngroup >= 1);
    uint64_t members = 0;
    for (uint64_t i = 0; i < ngroup; ++i) {
      members += g[i].nmember;
      CHECK(i == 0 || g[i - 1].best.sigma >= g[i].best.sigma);
      CHECK(g[i].acc_index_lo <= g[i].best.acc_index && g[i].best.acc_index <= g[i].acc_index_hi);
    }
    CHECK(members == many.size());
    printf("10^5 records: %llu groups\n", (unsigned long long)ngroup);
    frbch_pa_cand bad = rec(0, 0, 3, 10, 6.0);
    CHECK(frbch_pa_group_cands(&bad, 1, 2, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
    bad = rec(0, 0, 1, 0, 6.0);
    CHECK(frbch_pa_group_cands(&bad, 1, 2, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
    bad = rec(0, 0, 1, 10, 6.0);
    for (uint32_t gap : {0u, 17u}) {
      CHECK(frbch_pa_group_cands(&bad, 1, gap, 1, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
      CHECK(frbch_pa_group_cands(&bad, 1, 2, gap, nullptr, 0, &ngroup, err, sizeof err) == FRBCH_E_ARG);
    }
    CHECK(frbch_pa_group_cands(&bad, 1, 2, 1, nullptr, 0, nullptr, err, sizeof err) == FRBCH_E_ARG);
  }
  printf("accel_sanitize: ok\n");
  return 0;
}
