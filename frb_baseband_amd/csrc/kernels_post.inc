// Kernels behind the filterbank (SURVEY 8f rows 3 and 4): incoherent dedispersion of the [t][chan] rows (what the
// reference delegates to PRESTO's prepdata / prepsubband, process_vdif.py:202-229) and the phase fold of the rows (what
// base2fil.sh:474 delegates to `dspsr -E <par> -L 10 -A -d1 <fil>`).  Same macro layer as kernels_generic.inc, so the
// CPU unit tests run them through the host emulator too.  All sums over integer samples are exact (int64 / uint64
// accumulation, order-independent); float32 rows are summed in double in a fixed order.

struct PostParams {
  const uint8_t* rows;       // [nrows][nifs][nchan] samples of `nbits` (8, 16: unsigned; 32: float); product `prod` is used
  uint64_t nrows;
  int nchan, nifs, nbits, prod;
  // ---- clip + zero-DM + dedispersion ----
  const uint8_t* flagged;    // [nrows] 1 = time sample clipped: every channel reads as repl[c]; null = none
  const double* repl;        // [nchan] replacement values (integers for integer rows)
  const int32_t* tile_range; // tiled dedispersion: [DM group][channel tile] (smallest delay, rows spanned beyond the time tile)
  int nd, ct;                // ... DMs per workgroup, channels per tile
  double* rowsum;            // [nrows] S[t] = sum over channels of the (clipped) row
  double* colsum;            // [nchunks][nchan] per-chunk sums over unflagged rows (reduced in chunk order by the host)
  const int32_t* delays;     // [ndm][nchan] delay in samples, >= 0
  float* out;                // [ndm][nout]
  uint64_t nout;
  int ndm, zerodm;
  uint64_t rows_per_chunk;   // colsum: rows per workgroup row
  // ---- fold ----
  unsigned long long* prof_i;  // [nsub][nbin][nchan] sums (integer rows)
  double* prof_f;              // same for float rows
  uint32_t* hits;              // [nsub][nbin][nchan]
  const double* chan_delay_s;  // [nchan] dispersion delay relative to the reference frequency (null = fold as dspsr does: no delays)
  double t0_s;                 // (tstart - PEPOCH) in seconds
  double tsamp_s, f0, half_f1;
  int nbin;
  uint64_t rows_per_sub;
  uint32_t nsub;
  // ---- band-limited dedispersion (frbch_dedisperse_bands_*): out is [ndm * nband][nout] ----
  const uint16_t* band_ab;     // [nband][2] (a, b) of band j (the range kernel of the tiled form reads it)
  int nband, bsub, cps;        // bands, sub-bands, channels per sub-band
  int bw_min, bw_max;          // widths b - a that are listed
  uint32_t* pre;               // tiled form: [ndm][bsub][nout] sum over the channels below sub-band edge k + 1
  double* prez;                // ... the same sum of the zero-DM row sums S (zerodm only)
};

DEVFN inline double post_sample(const PostParams& p, uint64_t t, int c) {
  const uint64_t i = (t * (uint64_t)p.nifs + (uint64_t)p.prod) * (uint64_t)p.nchan + (uint64_t)c;
  if (p.nbits == 8) return (double)p.rows[i];
  if (p.nbits == 16) return (double)((const uint16_t*)p.rows)[i];
  return (double)((const float*)p.rows)[i];
}
DEVFN inline double post_value(const PostParams& p, uint64_t t, int c) {
  if (p.flagged && p.flagged[t]) return p.repl[c];
  return post_sample(p, t, c);
}

// S[t] = sum_c value(t, c), channels in ascending index order (fixed order: bit-reproducible for float rows as well).
// grid (ceil(nrows / 256), 1), one thread per row.
KERNEL(frbch_post_rowsum, PostParams) {
  K_PROLOGUE;
  (void)smem;
  (void)by;
  PHASE {
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t < p.nrows) {
      double s = 0.0;
      for (int c = 0; c < p.nchan; ++c) s += post_value(p, t, c);
      p.rowsum[t] = s;
    }
  }
}

// colsum[chunk][c] = sum over the unflagged rows of this workgroup's chunk, rows in ascending order.
// grid (ceil(nchan / 256), nchunks).
KERNEL(frbch_post_colsum, PostParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int c = bx * nthr + tid;
    if (c < p.nchan) {
      const uint64_t r0 = (uint64_t)by * p.rows_per_chunk;
      const uint64_t r1 = r0 + p.rows_per_chunk < p.nrows ? r0 + p.rows_per_chunk : p.nrows;
      double s = 0.0;
      for (uint64_t t = r0; t < r1; ++t)
        if (!(p.flagged && p.flagged[t])) s += post_sample(p, t, c);
      p.colsum[(size_t)by * p.nchan + c] = s;
    }
  }
}

// y[dm][t] = sum_c value(t + delay[dm][c], c)  -  (zerodm ? sum_c S[t + delay[dm][c]] / nchan : 0), as float32.
// grid (ceil(nout / 256), ndm), one thread per output sample, channels in ascending order.
KERNEL(frbch_post_dedisp, PostParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t < p.nout) {
      const int32_t* dly = p.delays + (size_t)by * p.nchan;
      double a = 0.0, b = 0.0;
      for (int c = 0; c < p.nchan; ++c) {
        const uint64_t ti = t + (uint64_t)dly[c];
        a += post_value(p, ti, c);
        if (p.zerodm) b += p.rowsum[ti];
      }
      const double y = p.zerodm ? a - b / (double)p.nchan : a;
      p.out[(size_t)by * p.nout + t] = (float)y;
    }
  }
}

// Band-limited dedispersion (include/frbch.h, "band-limited single-pulse search"): for band j = [a, b) of sub-bands
// y[dm][j][t] = sum_{c in [a cps, b cps)} value(t + delay[dm][c], c)  -  (zerodm ? the same sum of S / nchan : 0), as float32.
// grid (ceil(nout / 256), ndm), one thread per (dm, t).  For every first sub-band a the thread walks the channels upwards
// once and stores the running sums at the sub-band edges b whose width is listed: every band is summed from its own first
// channel in ascending order (float rows come out to the bit; band [0, bsub) is frbch_post_dedisp's series), and the rows
// are read once per first sub-band, not once per band.  Bands are numbered by ascending a, then b: the order of the walk.
KERNEL(frbch_post_dedisp_bands, PostParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t < p.nout) {
      const int32_t* dly = p.delays + (size_t)by * p.nchan;
      int j = 0;
      for (int a = 0; a < p.bsub; ++a) {
        double s = 0.0, z = 0.0;
        for (int b = a + 1; b <= p.bsub && b - a <= p.bw_max; ++b) {
          for (int c = (b - 1) * p.cps; c < b * p.cps; ++c) {
            const uint64_t ti = t + (uint64_t)dly[c];
            s += post_value(p, ti, c);
            if (p.zerodm) z += p.rowsum[ti];
          }
          if (b - a < p.bw_min) continue;
          const double y = p.zerodm ? s - z / (double)p.nchan : s;
          p.out[((size_t)by * p.nband + j) * p.nout + t] = (float)y;
          ++j;
        }
      }
    }
  }
}

// Phase of row t (channel c): tau = t0 + t * tsamp [- delay_c];  turns = f0 tau + (f1/2) tau^2;  bin = floor(frac(turns) * nbin).
// Every operation is a separately rounded double operation (no contraction), so the bin is the oracle's bit for bit.
DEVFN inline int post_bin(const PostParams& p, uint64_t t, int c) {
  POST_NO_CONTRACT
  const double tt = (double)t * p.tsamp_s;
  double tau = p.t0_s + tt;
  if (p.chan_delay_s) tau = tau - p.chan_delay_s[c];
  const double a = p.f0 * tau;
  const double b = (p.half_f1 * tau) * tau;
  const double turns = a + b;
  const double fr = turns - floor(turns);
  int bin = (int)(fr * (double)p.nbin);
  if (bin >= p.nbin) bin = p.nbin - 1;
  return bin;
}

// Fold: profile[sub][bin][chan] += value, hits += 1.  grid (ceil(nchan / 256), ceil(nrows / rows_per_chunk)); a thread owns
// one channel and walks the rows of its chunk, keeping a running sum while (sub, bin) stays the same (a bin lasts several
// rows) and flushing it with one atomic.  Integer rows: uint64 sums, exact in any order.
KERNEL(frbch_post_fold, PostParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int c = bx * nthr + tid;
    if (c < p.nchan) {
      const uint64_t r0 = (uint64_t)by * p.rows_per_chunk;
      const uint64_t r1 = r0 + p.rows_per_chunk < p.nrows ? r0 + p.rows_per_chunk : p.nrows;
      long long cur = -1;
      double acc = 0.0;
      uint32_t n = 0;
      for (uint64_t t = r0; t < r1; ++t) {
        const uint64_t sub = t / p.rows_per_sub;
        if (sub >= p.nsub) break;
        const long long slot = ((long long)sub * p.nbin + post_bin(p, t, c)) * (long long)p.nchan + c;
        if (slot != cur) {
          if (n) {
            if (p.prof_i) ATOMIC_ADD_U64(p.prof_i + cur, (unsigned long long)acc);
            else ATOMIC_ADD_F64(p.prof_f + cur, acc);
            ATOMIC_ADD_U32(p.hits + cur, n);
          }
          cur = slot;
          acc = 0.0;
          n = 0;
        }
        acc += post_sample(p, t, c);      // (integer rows: < 2^53, exact)
        ++n;
      }
      if (n) {
        if (p.prof_i) ATOMIC_ADD_U64(p.prof_i + cur, (unsigned long long)acc);
        else ATOMIC_ADD_F64(p.prof_f + cur, acc);
        ATOMIC_ADD_U32(p.hits + cur, n);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fold of EVERY product of the rows in one pass, with a phase model (frbch_foldp_*): either the F0 / F1 / PEPOCH polynomial
// of post_bin (optionally with a constant Doppler factor) or the blocks of a TEMPO polyco -- the predictor dspsr itself
// folds with (base2fil.sh:474), which carries the barycentric, binary and position terms.
// ---------------------------------------------------------------------------------------------------------------------
struct FoldSeg {               // one polyco block, times relative to the start of the file
  double dt0_min;              // (tstart - TMID) * 1440
  double rphase, f0;           // RPHASE reduced to [0, 1), reference rotation frequency
  double coeff[15];
  int ncoeff, pad;
};

struct FoldpParams {
  const uint8_t* rows;         // [nrows][nifs][nchan] samples of `nbits`
  uint64_t nrows;
  int nchan, nifs, nbits, nbin;
  unsigned long long* prof_i;  // [nsub][nifs][nbin][nchan] sums (integer rows)
  double* prof_f;              // same for float rows; for frbch_post_u64_to_f64: where the integer sums go as doubles
  uint64_t nconv;              // frbch_post_u64_to_f64: entries
  uint32_t* hits;              // [nsub][nbin][nchan], shared by the products
  const double* chan_delay_s;  // [nchan] or null, as PostParams
  double t0_s, tsamp_s, f0, half_f1, doppler;   // nseg = 0: the polynomial of post_bin, tau stretched by (1 + doppler)
  const FoldSeg* seg;          // [nseg] ascending TMID
  const uint64_t* seg_row;     // [nseg] first row of every block (seg_row[0] = 0); the kernels only compare row numbers
  int nseg;
  uint32_t nsub;
  uint64_t rows_per_sub, rows_per_chunk;
  // ---- LDS kernel (kernels_post_fast.inc) ----
  uint32_t* slot;              // [nrows] sub * nbin + bin of every row (no per-channel delays: the bin depends on the row only)
  uint32_t* slot_hits;         // [nsub * nbin] rows per slot
  int ct, ct_log2, ntile;      // channels per tile (a power of two), tiles per row
  uint32_t chunks_per_sub;
};

DEVFN inline double foldp_sample(const FoldpParams& p, uint64_t t, int q, int c) {
  const uint64_t i = (t * (uint64_t)p.nifs + (uint64_t)q) * (uint64_t)p.nchan + (uint64_t)c;
  if (p.nbits == 8) return (double)p.rows[i];
  if (p.nbits == 16) return (double)((const uint16_t*)p.rows)[i];
  return (double)((const float*)p.rows)[i];
}

// Phase of row t (channel c) in polyco block s -- TEMPO's PHASE = RPHASE + DT 60 F0 + C1 + DT C2 + DT^2 C3 + ..., DT in minutes:
//   sec = t tsamp [- delay_c];  dt = (tstart - TMID_s) 1440 + sec / 60;  turns = (rphase + (dt 60) f0) + horner(coeff, dt),
// Horner from the highest coefficient down.  nseg = 0: post_bin's tau, then tau + tau doppler when doppler != 0.  Every
// operation is rounded on its own (no contraction), so a numpy restatement gives the same bin bit for bit.
DEVFN inline int foldp_bin(const FoldpParams& p, uint64_t t, int c, int s) {
  POST_NO_CONTRACT
  const double tt = (double)t * p.tsamp_s;
  double turns;
  if (p.nseg) {
    double sec = tt;
    if (p.chan_delay_s) sec = sec - p.chan_delay_s[c];
    const FoldSeg& g = p.seg[s];
    const double dt = g.dt0_min + sec / 60.0;
    double h = g.coeff[g.ncoeff - 1];
    for (int i = g.ncoeff - 2; i >= 0; --i) {
      const double hd = h * dt;
      h = hd + g.coeff[i];
    }
    const double lin = (dt * 60.0) * g.f0;
    const double lead = g.rphase + lin;
    turns = lead + h;
  } else {
    double tau = p.t0_s + tt;
    if (p.chan_delay_s) tau = tau - p.chan_delay_s[c];
    if (p.doppler != 0.0) {
      const double stretch = tau * p.doppler;
      tau = tau + stretch;
    }
    const double a = p.f0 * tau;
    const double b = (p.half_f1 * tau) * tau;
    turns = a + b;
  }
  const double fr = turns - floor(turns);
  int bin = (int)(fr * (double)p.nbin);
  if (bin >= p.nbin) bin = p.nbin - 1;
  return bin;
}

DEVFN inline void foldp_flush(const FoldpParams& p, long long slot, int c, const double* acc, uint32_t n) {
  const long long sub = slot / p.nbin, bin = slot - sub * p.nbin;
  for (int q = 0; q < p.nifs; ++q) {
    const size_t i = (((size_t)sub * p.nifs + q) * p.nbin + (size_t)bin) * p.nchan + c;
    if (p.prof_i) ATOMIC_ADD_U64(p.prof_i + i, (unsigned long long)acc[q]);
    else ATOMIC_ADD_F64(p.prof_f + i, acc[q]);
  }
  ATOMIC_ADD_U32(p.hits + (size_t)slot * p.nchan + c, n);
}

// profile[sub][product][bin][chan] += value, hits[sub][bin][chan] += 1: the grid and the run-length accumulation of
// frbch_post_fold; a thread loads the nifs (<= 4) products of its channel per row and computes the phase once for them all.
KERNEL(frbch_post_foldp, FoldpParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int c = bx * nthr + tid;
    if (c < p.nchan) {
      const uint64_t r0 = (uint64_t)by * p.rows_per_chunk;
      const uint64_t r1 = r0 + p.rows_per_chunk < p.nrows ? r0 + p.rows_per_chunk : p.nrows;
      long long cur = -1;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      uint32_t n = 0;
      int s = 0;
      for (uint64_t t = r0; t < r1; ++t) {
        const uint64_t sub = t / p.rows_per_sub;
        if (sub >= p.nsub) break;
        while (s + 1 < p.nseg && p.seg_row[s + 1] <= t) ++s;
        const long long slot = (long long)sub * p.nbin + foldp_bin(p, t, c, s);
        if (slot != cur) {
          if (n) foldp_flush(p, cur, c, acc, n);
          cur = slot;
          acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
          n = 0;
        }
        for (int q = 0; q < p.nifs; ++q) acc[q] += foldp_sample(p, t, q, c);      // (integer rows: < 2^53, exact)
        ++n;
      }
      if (n) foldp_flush(p, cur, c, acc, n);
    }
  }
}

// the exact integer sums as doubles (every value < 2^53).  grid (ceil(nconv / 256), 1)
KERNEL(frbch_post_u64_to_f64, FoldpParams) {
  K_PROLOGUE;
  (void)smem;
  (void)by;
  PHASE {
    const uint64_t i = (uint64_t)bx * nthr + tid;
    if (i < p.nconv) p.prof_f[i] = (double)p.prof_i[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Single-pulse search of the dedispersed series (frbch_spsearch_*; include/frbch.h states the arithmetic): per-block
// statistics in double in a FIXED order, samples normalised and quantised to integers q = floor(z 1024 + 0.5), and from
// there on integers only -- boxcar sums, threshold and local-maximum tests are exact in any order, so the generic kernel
// below, the LDS kernel of kernels_post_fast.inc and tests/spsearch_oracle.py agree to the bit.
// ---------------------------------------------------------------------------------------------------------------------
#ifndef ATOMIC_FETCH_ADD_U32   // (a device layer without it: workgroups are host threads there)
#define ATOMIC_FETCH_ADD_U32(ptr, v) __atomic_fetch_add((unsigned int*)(ptr), (unsigned int)(v), __ATOMIC_RELAXED)
#endif

struct SpPeak {                // a raw peak: local maximum of one width's boxcar series above the threshold
  uint32_t dm, width;
  uint64_t t;                  // first sample of the boxcar
  long long sum;               // S_w[t]
};

struct SpParams {
  const float* series;         // [ndm][nout]
  uint64_t nout;
  int ndm;
  uint64_t blk_len;            // L: samples per statistics block (the last block runs to nout)
  uint32_t nblk;               // max(1, nout / L)
  double* stats;               // [ndm][nblk][2]: mean, 1 / sigma of the second round; a dead block holds (0, 0)
  int32_t* q;                  // [ndm][nout] quantised samples (generic kernels only)
  int nwidth;
  int width[16];               // ascending
  long long thr[16];           // T_w = ceil(threshold 1024 sqrt(w))
  SpPeak* peaks;               // [peak_cap], appended in any order
  uint32_t* npeak;             // every raw peak counts, stored or not
  uint32_t peak_cap;
};

constexpr int kSpPartials = 64;            // partial sums per block = threads of frbch_post_sp_stats
constexpr double kSpClip = 65536.0;        // |z| is clipped here: |q| <= 2^26, a sum of 1024 of them < 2^37

// q of sample x with its block's (mean, 1 / sigma); every operation rounded on its own
DEVFN inline int32_t sp_quantise(float x, double mean, double inv) {
  POST_NO_CONTRACT
  if (inv == 0.0) return 0;                                      // dead block (x may be anything, NaN included)
  const double d = (double)x - mean;
  double z = d * inv;
  if (z > kSpClip) z = kSpClip;
  if (z < -kSpClip) z = -kSpClip;
  const double zs = z * 1024.0;
  return (int32_t)floor(zs + 0.5);
}

DEVFN inline void sp_append(const SpParams& p, int dm, int w, uint64_t t, long long s) {
  const uint32_t i = ATOMIC_FETCH_ADD_U32(p.npeak, 1u);
  if (i < p.peak_cap) {
    SpPeak k;
    k.dm = (uint32_t)dm; k.width = (uint32_t)w; k.t = t; k.sum = s;
    p.peaks[i] = k;
  }
}

// Block statistics: grid (nblk, ndm), 64 threads, smem 64 x 3 doubles + 2.  Thread j sums the samples at block positions
// j, j + 64, ... in ascending order; thread 0 adds the 64 partials in ascending j.  Round 2 keeps |x - mean1| <= 3 sigma1,
// every sample in its own partial.
KERNEL(frbch_post_sp_stats, SpParams) {
  K_PROLOGUE;
  (void)nthr;
  double* part = (double*)smem;                                  // [3][64]: s1, s2, n
  double* first = part + 3 * kSpPartials;                        // mean1, 3 sigma1 (sigma1 = 0: dead)
  const uint64_t b0 = (uint64_t)bx * p.blk_len;
  const uint64_t b1 = (uint32_t)bx + 1 == p.nblk ? p.nout : b0 + p.blk_len;
  const float* x = p.series + (size_t)by * p.nout;
  double* out = p.stats + ((size_t)by * p.nblk + bx) * 2;
  for (int round = 0; round < 2; ++round) {
    PHASE {
      POST_NO_CONTRACT
      double s1 = 0.0, s2 = 0.0, n = 0.0;
      if (tid < kSpPartials && (round == 0 || first[1] > 0.0)) {
        for (uint64_t t = b0 + tid; t < b1; t += kSpPartials) {
          const double v = (double)x[t];
          if (round == 1 && !(fabs(v - first[0]) <= first[1])) continue;
          const double vv = v * v;
          s1 = s1 + v;
          s2 = s2 + vv;
          n = n + 1.0;
        }
      }
      if (tid < kSpPartials) { part[tid] = s1; part[kSpPartials + tid] = s2; part[2 * kSpPartials + tid] = n; }
    }
    SYNC;
    PHASE {
      POST_NO_CONTRACT
      if (tid == 0) {
        double s1 = 0.0, s2 = 0.0, n = 0.0;
        for (int j = 0; j < kSpPartials; ++j) { s1 = s1 + part[j]; s2 = s2 + part[kSpPartials + j]; n = n + part[2 * kSpPartials + j]; }
        double mean = 0.0, sig = 0.0;
        if (n > 0.0) {
          mean = s1 / n;
          const double m2 = s2 / n;
          const double mm = mean * mean;
          const double var = m2 - mm;
          sig = var > 0.0 ? sqrt(var) : 0.0;
        }
        if (round == 0) {
          first[0] = mean;
          first[1] = 3.0 * sig;
        } else {
          const bool live = first[1] > 0.0 && sig > 0.0;
          out[0] = live ? mean : 0.0;
          out[1] = live ? 1.0 / sig : 0.0;
        }
      }
    }
    SYNC;
  }
}

DEVFN inline const double* sp_block(const SpParams& p, int dm, uint64_t t) {
  uint64_t b = t / p.blk_len;
  if (b >= p.nblk) b = p.nblk - 1;
  return p.stats + ((size_t)dm * p.nblk + b) * 2;
}

// q[dm][t] for the generic search.  grid (ceil(nout / 256), ndm)
KERNEL(frbch_post_sp_quant, SpParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t < p.nout) {
      const double* st = sp_block(p, by, t);
      p.q[(size_t)by * p.nout + t] = sp_quantise(p.series[(size_t)by * p.nout + t], st[0], st[1]);
    }
  }
}

// S_w[t] of the quantised series, summed directly
DEVFN inline long long sp_boxcar(const int32_t* q, uint64_t t, int w) {
  long long s = 0;
  for (int i = 0; i < w; ++i) s += q[t + i];
  return s;
}

// The generic search: grid (ceil(nout / 256), ndm), one thread per (dm, t).  The widths ascend, so S_w[t] grows from the
// previous width's sum; a sum that passes the threshold is compared with its neighbours t - h .. t + h (h = w / 2, cut to
// the valid range), strictly greater than the earlier ones, not less than the later ones.
KERNEL(frbch_post_sp_search, SpParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t < p.nout) {
      const int32_t* q = p.q + (size_t)by * p.nout;
      long long s = 0;
      int have = 0;
      for (int k = 0; k < p.nwidth; ++k) {
        const int w = p.width[k];
        if ((uint64_t)w > p.nout || t > p.nout - (uint64_t)w) break;
        for (; have < w; ++have) s += q[t + have];
        if (s < p.thr[k]) continue;
        const uint64_t h = (uint64_t)(w / 2), last = p.nout - (uint64_t)w;
        const uint64_t lo = t > h ? t - h : 0, hi = t + h < last ? t + h : last;
        bool peak = true;
        long long v = sp_boxcar(q, lo, w);
        for (uint64_t u = lo; u <= hi && peak; ++u) {
          if (u < t) peak = s > v;
          else if (u > t) peak = s >= v;
          if (u < hi) v += (long long)q[u + w] - (long long)q[u];
        }
        if (peak) sp_append(p, by, w, t, s);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Corner turn (SURVEY 8f row 2): what jive5ab's spif2file does with the recipe strings of spif2file.sh:31-113 -- one
// recorder stream in which every W-bit word holds one time sample of ALL channels is split into one 2-channel stream
// per IF ("tag"): output group g takes bits src[g][0..glen) of every word, in that order, LSB first.
// ---------------------------------------------------------------------------------------------------------------------
struct CornerParams {
  const uint8_t* frames;     // recorder frames (header + payload), words never straddle a frame
  uint32_t frame_bytes, header_bytes, payload_bytes;
  uint64_t nwords;           // words in the launch; nwords * glen is a whole number of bytes
  int word_bits;             // W: 4, 8, 16, 32 or 64
  int ngroup, glen;          // output streams, bits each takes per word (1, 2, 4 or 8)
  int swap_sign_mag;         // Mark5B: exchange the two bits of every 2-bit sample first (spif2file.sh:79-94)
  uint8_t src[16][8];        // source bit of output bit k of group g
  uint8_t* out[16];          // [nwords * glen / 8] bytes each
};

DEVFN inline uint64_t corner_word(const CornerParams& p, uint64_t k) {
  const uint64_t bit = k * (uint64_t)p.word_bits;
  const uint64_t byte = bit >> 3;
  const uint64_t fr = byte / p.payload_bytes;
  const uint8_t* src = p.frames + fr * p.frame_bytes + p.header_bytes + (byte - fr * p.payload_bytes);
  const int nbytes = (p.word_bits + 7) >> 3;
  uint64_t w = 0;
  for (int i = 0; i < nbytes; ++i) w |= (uint64_t)src[i] << (8 * i);
  if (p.word_bits < 8) w = (w >> (bit & 7)) & ((1ull << p.word_bits) - 1);
  if (p.swap_sign_mag) w = ((w & 0x5555555555555555ull) << 1) | ((w >> 1) & 0x5555555555555555ull);
  return w;
}

// one thread = 64 / glen consecutive words = eight output bytes of every group.  grid (ceil(nwords * glen / 64 / 256), 1)
KERNEL(frbch_post_cornerturn, CornerParams) {
  K_PROLOGUE;
  (void)smem;
  (void)by;
  PHASE {
    const int wpt = 64 / p.glen;
    const uint64_t t = (uint64_t)bx * nthr + tid;
    if (t * wpt < p.nwords) {
      uint64_t acc[16];
      for (int g = 0; g < p.ngroup; ++g) acc[g] = 0;
      const uint64_t left = p.nwords - t * wpt;
      const int nw = left < (uint64_t)wpt ? (int)left : wpt;       // (the last thread may hold fewer words)
      for (int j = 0; j < nw; ++j) {
        const uint64_t w = corner_word(p, t * wpt + j);
        for (int g = 0; g < p.ngroup; ++g) {
          uint64_t v = 0;
          for (int k = 0; k < p.glen; ++k) v |= ((w >> p.src[g][k]) & 1ull) << k;
          acc[g] |= v << (j * p.glen);
        }
      }
      for (int g = 0; g < p.ngroup; ++g) {
        uint8_t* dst = p.out[g] + t * 8;
        for (int i = 0; i < nw * p.glen / 8; ++i) dst[i] = (uint8_t)(acc[g] >> (8 * i));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Candidate cut-outs (frbch_cutout_*; include/frbch.h states the arithmetic): per candidate the dedispersed
// frequency-time plane FT[nf][nt] and the DM-time plane DT[ndm][nt], time bins of `tfactor` rows, with the number of
// present samples of every pixel.  No clip, no zero-DM filter.  A "plane row" is a frequency bin (FT: the channels
// [b cpb, (b + 1) cpb) at the delays of the candidate's DM) or a trial DM (DT: all channels at the delays of dm_k).
// ---------------------------------------------------------------------------------------------------------------------
struct CutCand {
  long long t0;                // first row of time bin 0 at the top of the band: sample - (nt / 2) * tfactor (may be negative)
  int tfactor, pad;
};

struct CutParams {
  const uint8_t* rows;         // [nrows][nifs][nchan] samples of `nbits`; product `prod` is used
  uint64_t nrows;
  int nchan, nifs, nbits, prod;
  int nt, nf, ndm, cpb;        // cpb = nchan / nf
  int kind;                    // 0: the frequency-time plane, 1: the DM-time plane
  int ncand;                   // candidates of this launch
  const CutCand* cand;         // [ncand]
  const int32_t* ft_delays;    // [ncand][nchan]
  const int32_t* dt_delays;    // [ncand][ndm][nchan]
  float* out;                  // [ncand][plane rows][nt]
  uint32_t* hits;              // same shape
  // ---- LDS kernel (kernels_post_fast.inc) ----
  const int32_t* tile_range;   // [ncand][row group][channel tile] (smallest delay, rows spanned beyond the time tile; span < 0: no channel of the tile belongs to the group)
  int ngrp, nct;
};

DEVFN inline double cut_sample(const CutParams& p, long long s, int c) {
  const uint64_t i = ((uint64_t)s * (uint64_t)p.nifs + (uint64_t)p.prod) * (uint64_t)p.nchan + (uint64_t)c;
  if (p.nbits == 8) return (double)p.rows[i];
  if (p.nbits == 16) return (double)((const uint16_t*)p.rows)[i];
  return (double)((const float*)p.rows)[i];
}

// The generic form, the correctness anchor and the fallback: grid (ceil(plane rows * nt / 256), ncand), one thread per
// pixel, channels ascending, the rows of the bin ascending inside, sums in double.
KERNEL(frbch_post_cutout, CutParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int nrow = p.kind ? p.ndm : p.nf;
    const long long pix = (long long)bx * nthr + tid;
    if (pix < (long long)nrow * p.nt) {
      const int r = (int)(pix / p.nt), j = (int)(pix - (long long)r * p.nt);
      const CutCand cd = p.cand[by];
      const int32_t* dly = p.kind ? p.dt_delays + ((size_t)by * p.ndm + r) * p.nchan : p.ft_delays + (size_t)by * p.nchan;
      const int c0 = p.kind ? 0 : r * p.cpb, c1 = p.kind ? p.nchan : (r + 1) * p.cpb;
      const long long tb = cd.t0 + (long long)j * cd.tfactor;
      double a = 0.0;
      uint32_t n = 0;
      for (int c = c0; c < c1; ++c) {
        const long long s0 = tb + (long long)dly[c];
        for (int u = 0; u < cd.tfactor; ++u) {
          const long long s = s0 + u;
          if (s >= 0 && s < (long long)p.nrows) {
            a += cut_sample(p, s, c);
            ++n;
          }
        }
      }
      const size_t o = ((size_t)by * nrow + r) * p.nt + j;
      p.out[o] = (float)a;
      p.hits[o] = n;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Interference (frbch_rfi_*; include/frbch.h states the arithmetic): per (block of rows, channel) the sums S = sum x and
// Q = sum x x of one product, and the in-place replacement of the masked cells.
// ---------------------------------------------------------------------------------------------------------------------
struct RfiPeak { float num; uint32_t k; };   // frbch_rfi_peak
struct RfiParams {
  uint8_t* rows;               // [nrows][nifs][nchan] samples of `nbits`; product `prod` is used (apply writes it)
  uint64_t nrows;
  int nchan, nifs, nbits, prod;
  uint32_t block_rows, nblk;
  uint32_t blk0, pad;          // block of workgroup row 0 (a launch holds at most 65535 blocks)
  unsigned long long* stats_i; // [nblk][nchan][2] (S, Q), integer rows
  double* stats_f;             // the same for float rows
  const uint8_t* mask;         // [nblk][nchan], apply
  const double* repl;          // [nchan], apply
  // ---- fast kernel (kernels_post_fast.inc) ----
  int tile_bytes, ntile;       // bytes of a row a workgroup owns (a power of two, 64 .. 1024); tiles per row
  // ---- periodicity (frbch_rfi_peaks_*): n = block_rows = 2^log2n ----
  const float* tw;             // [n / 2][2] the host's table W[k] = (cos, -sin)(2 pi k / n)
  RfiPeak* peaks;              // [nblk][nchan]
  int log2n, pad2;
};

// The generic form, the correctness anchor and the fallback (and the only kernel for float rows): grid (ceil(nchan / 256),
// nblk), one thread per channel, rows ascending.
KERNEL(frbch_post_rfi_stats, RfiParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    POST_NO_CONTRACT
    const int c = bx * nthr + tid;
    const uint64_t b = (uint64_t)p.blk0 + (uint64_t)by;
    if (c < p.nchan) {
      const uint64_t r0 = b * p.block_rows;
      const uint64_t r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const uint64_t first = (uint64_t)p.prod * (uint64_t)p.nchan + (uint64_t)c;
      const size_t o = ((size_t)b * p.nchan + c) * 2;
      if (p.nbits == 32) {
        const float* x = (const float*)p.rows;
        double s = 0.0, q = 0.0;
        for (uint64_t t = r0; t < r1; ++t) {
          const double v = (double)x[t * pitch + first];
          const double vv = v * v;
          s = s + v;
          q = q + vv;
        }
        p.stats_f[o] = s;
        p.stats_f[o + 1] = q;
      } else {
        unsigned long long s = 0, q = 0;
        for (uint64_t t = r0; t < r1; ++t) {
          const unsigned long long v = p.nbits == 8 ? (unsigned long long)p.rows[t * pitch + first]
                                                    : (unsigned long long)((const uint16_t*)p.rows)[t * pitch + first];
          s += v;
          q += v * v;
        }
        p.stats_i[o] = s;
        p.stats_i[o + 1] = q;
      }
    }
  }
}

// Every sample of a masked cell becomes repl[c]; nothing else is written.  grid (ceil(nchan / 256), nblk), one thread per
// cell: a thread whose cell is unmasked returns after reading the mask, so a workgroup without a masked cell costs one read.
KERNEL(frbch_post_rfi_apply, RfiParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int c = bx * nthr + tid;
    const uint64_t b = (uint64_t)p.blk0 + (uint64_t)by;
    if (c < p.nchan && p.mask[(size_t)b * p.nchan + c]) {
      const uint64_t r0 = b * p.block_rows;
      const uint64_t r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const uint64_t first = (uint64_t)p.prod * (uint64_t)p.nchan + (uint64_t)c;
      double r = p.repl[c];
      if (p.nbits != 32) {                        // a caller's value outside the code range (or a NaN) is clamped, not converted
        const double top = p.nbits == 8 ? 255.0 : 65535.0;
        if (!(r >= 0.0)) r = 0.0;
        if (r > top) r = top;
      }
      if (p.nbits == 8) {
        const uint8_t v = (uint8_t)r;
        for (uint64_t t = r0; t < r1; ++t) p.rows[t * pitch + first] = v;
      } else if (p.nbits == 16) {
        const uint16_t v = (uint16_t)r;
        for (uint64_t t = r0; t < r1; ++t) ((uint16_t*)p.rows)[t * pitch + first] = v;
      } else {
        const float v = (float)r;
        for (uint64_t t = r0; t < r1; ++t) ((float*)p.rows)[t * pitch + first] = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Periodicity (frbch_rfi_peaks_*; include/frbch.h states the arithmetic): the largest bin of the power spectrum of every
// (block, channel) cell, two real channels per complex transform.  The helpers below ARE the arithmetic: the generic kernel
// and the fast one (kernels_post_fast.inc) call the same butterfly and the same bin formula, so that they differ in schedule only.
// ---------------------------------------------------------------------------------------------------------------------
DEVFN inline bool rfi_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// the mean of a cell and whether the cell is tested: S, Q, mean and var of step 1 of frbch_rfi_mask
DEVFN inline bool rfi_cell_mean(const RfiParams& p, uint64_t b, int c, double nb, double* mean) {
  POST_NO_CONTRACT
  const size_t i = ((size_t)b * p.nchan + c) * 2;
  const double S = p.nbits == 32 ? p.stats_f[i] : (double)p.stats_i[i];
  const double Q = p.nbits == 32 ? p.stats_f[i + 1] : (double)p.stats_i[i + 1];
  const double m = S / nb;
  const double mm = m * m;
  const double qn = Q / nb;
  double var = qn - mm;
  if (var < 0.0) var = 0.0;                                                        // (a NaN stays a NaN)
  *mean = m;
  return rfi_finite(m) && rfi_finite(var) && var != 0.0;
}

// u' = u + w v, v' = u - w v: the two products of each component first, every operation rounded on its own
DEVFN inline void rfi_bfly(float& ur, float& ui, float& vr, float& vi, float wr, float wi) {
  POST_NO_CONTRACT
  const float a = wr * vr;
  const float b = wi * vi;
  const float c = wr * vi;
  const float d = wi * vr;
  const float tr = a - b;
  const float ti = c + d;
  const float xr = ur + tr;
  const float xi = ui + ti;
  const float yr = ur - tr;
  const float yi = ui - ti;
  ur = xr; ui = xi; vr = yr; vi = yi;
}

// bin k of the two channels of a pair from A = Z[k], B = Z[n - k]
DEVFN inline void rfi_bins(float ar, float ai, float br, float bi, float* n0, float* n1) {
  POST_NO_CONTRACT
  const float s0 = ar + br;
  const float d0 = ai - bi;
  const float s1 = ai + bi;
  const float d1 = br - ar;
  const float s0s = s0 * s0;
  const float d0d = d0 * d0;
  const float s1s = s1 * s1;
  const float d1d = d1 * d1;
  *n0 = s0s + d0d;
  *n1 = s1s + d1d;
}

DEVFN inline int rfi_bitrev(int j, int bits) {
  int r = 0;
  for (int q = 0; q < bits; ++q) { r = (r << 1) | (j & 1); j >>= 1; }
  return r;
}

// The generic form, the correctness anchor and the fallback (and the only kernel for float rows): grid (ceil(nchan / 2), nblk),
// a workgroup per (block, channel pair); smem = n complex values and 2 x nthr partial peaks.  One stage of n / 2 butterflies
// between two barriers; then every thread walks the bins k = 1 + tid, 1 + tid + nthr, ... and one thread per channel takes the
// largest of the partials, the lowest k among equals -- what the walk over ascending k keeps.
KERNEL(frbch_post_rfi_peaks, RfiParams) {
  K_PROLOGUE;
  const int n = (int)p.block_rows, L = p.log2n;
  float* z = (float*)smem;                                                         // [n][2]
  RfiPeak* part = (RfiPeak*)(smem + (size_t)n * 8);                                // [2][nthr]
  const uint64_t b = (uint64_t)p.blk0 + (uint64_t)by;
  const int c0 = 2 * bx, c1 = c0 + 1;
  const uint64_t r0 = b * p.block_rows;
  const uint64_t r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;
  const int nbr = (int)(r1 - r0);
  double mean0 = 0.0, mean1 = 0.0;
  bool t0 = false, t1 = false;
  if (2 * nbr >= n) {
    t0 = rfi_cell_mean(p, b, c0, (double)nbr, &mean0);
    if (c1 < p.nchan) t1 = rfi_cell_mean(p, b, c1, (double)nbr, &mean1);
  }
  const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
  const uint64_t first = (uint64_t)p.prod * (uint64_t)p.nchan;
  PHASE {
    POST_NO_CONTRACT
    for (int j = tid; j < n; j += nthr) {
      float x0 = 0.f, x1 = 0.f;
      if (j < nbr) {
        const uint64_t i = (r0 + (uint64_t)j) * pitch + first;
        if (t0) {
          const double v = p.nbits == 8 ? (double)p.rows[i + c0] : p.nbits == 16 ? (double)((const uint16_t*)p.rows)[i + c0]
                                                                                  : (double)((const float*)p.rows)[i + c0];
          const double d = v - mean0;
          x0 = (float)d;
        }
        if (t1) {
          const double v = p.nbits == 8 ? (double)p.rows[i + c1] : p.nbits == 16 ? (double)((const uint16_t*)p.rows)[i + c1]
                                                                                  : (double)((const float*)p.rows)[i + c1];
          const double d = v - mean1;
          x1 = (float)d;
        }
      }
      const int i = rfi_bitrev(j, L);
      z[2 * i] = x0;
      z[2 * i + 1] = x1;
    }
  }
  SYNC;
  for (int s = 1; s <= L; ++s) {
    PHASE {
      const int half = 1 << (s - 1);
      for (int i = tid; i < n / 2; i += nthr) {
        const int j = i & (half - 1);
        const int u = ((i >> (s - 1)) << s) + j, v = u + half;
        const int k = j << (L - s);
        rfi_bfly(z[2 * u], z[2 * u + 1], z[2 * v], z[2 * v + 1], p.tw[2 * k], p.tw[2 * k + 1]);
      }
    }
    SYNC;
  }
  PHASE {
    RfiPeak q0, q1;
    q0.num = 0.f; q0.k = 0u; q1.num = 0.f; q1.k = 0u;
    for (int k = 1 + tid; k < n / 2; k += nthr) {
      float n0, n1;
      rfi_bins(z[2 * k], z[2 * k + 1], z[2 * (n - k)], z[2 * (n - k) + 1], &n0, &n1);
      if (n0 > q0.num) { q0.num = n0; q0.k = (uint32_t)k; }
      if (n1 > q1.num) { q1.num = n1; q1.k = (uint32_t)k; }
    }
    part[tid] = q0;
    part[nthr + tid] = q1;
  }
  SYNC;
  PHASE {
    if (tid < 2 && c0 + tid < p.nchan) {
      RfiPeak best;
      best.num = 0.f; best.k = 0u;
      for (int t = 0; t < nthr; ++t) {
        const RfiPeak q = part[tid * nthr + t];
        if (q.num > best.num || (q.num == best.num && q.k < best.k)) best = q;
      }
      p.peaks[(size_t)b * p.nchan + c0 + tid] = best;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Periodicity search of the dedispersed series (frbch_psearch_*; include/frbch.h states the arithmetic): the mean of every
// series in a FIXED order, two series per complex transform of n = 2^L points with the butterfly and the bin formula of the
// periodicity test above (rfi_bfly, rfi_bins), block levels in double in ascending k, harmonic sums in float in ascending j.
// The kernels below are the generic form: the transform goes stage by stage through the work array in global memory.  The
// fast form (kernels_post_fast.inc) replaces the load and the stages by LDS-resident passes and shares everything else.
// ---------------------------------------------------------------------------------------------------------------------
struct PsPeak { uint32_t dm, h, k; float H; };   // a raw peak of the fold h
struct PsParams {
  const float* series;         // [ndm][nout]; only t < n is read
  uint64_t nout;
  int ndm, npair, log2n, logb;  // logb: log2 of wblock
  uint32_t n;                  // 2^log2n
  const float* tw;             // [n / 2][2] the host's table W[k]
  double* mean;                // [ndm]
  uint32_t* live;              // [ndm] 1: the mean is finite
  float* work;                 // [npair][n][2]
  float* pw;                   // [ndm][n / 2]: N[k], then p[k] in place
  uint32_t wblock, nblk;       // B; blocks of the bins 1 .. n/2 - 1 (the last one may be short or long)
  uint32_t kmin, nfold;        // folds 1, 2, 4, ... 2^(nfold - 1)
  float thr[5];
  PsPeak* peaks;
  uint32_t* npeak;
  uint32_t peak_cap;
  int stage;                   // generic: the stage of this launch
  int s0, rcur, logc;          // fast: stages done before this pass, stages of it, log2 of the columns of a tile
};

constexpr int kPsPartials = 64;
constexpr int kPsBatch = 32;                // samples of a partial sum loaded ahead of their additions (the chain of additions is what the rule fixes)

// grid (ndm), 64 threads, smem 64 doubles: partial j adds positions j, j + 64, ... ascending, thread 0 the partials in ascending j
KERNEL(frbch_post_ps_mean, PsParams) {
  K_PROLOGUE;
  (void)by; (void)nthr;
  double* part = (double*)smem;
  const float* x = p.series + (size_t)bx * p.nout;
  PHASE {
    POST_NO_CONTRACT
    if (tid < kPsPartials) {
      double s = 0.0;
      uint32_t t = (uint32_t)tid;
      for (; t < p.n; t += (uint32_t)(kPsBatch * kPsPartials)) {   // kPsBatch loads in flight, added in order (n is a multiple of 4096)
        float v[kPsBatch];
        for (int u = 0; u < kPsBatch; ++u) v[u] = x[t + (uint32_t)(u * kPsPartials)];
        for (int u = 0; u < kPsBatch; ++u) s = s + (double)v[u];
      }
      part[tid] = s;
    }
  }
  SYNC;
  PHASE {
    POST_NO_CONTRACT
    if (tid == 0) {
      double s = 0.0;
      for (int j = 0; j < kPsPartials; ++j) s = s + part[j];
      const double m = s / (double)p.n;
      p.mean[bx] = m;
      p.live[bx] = rfi_finite(m) ? 1u : 0u;
    }
  }
}

// z of sample t of the pair: (series 2 pair, series 2 pair + 1), 0 for a dead or missing one
DEVFN inline void ps_sample(const PsParams& p, int pair, uint32_t t, float* a, float* b) {
  POST_NO_CONTRACT
  const int d0 = 2 * pair, d1 = d0 + 1;
  *a = 0.f; *b = 0.f;
  if (p.live[d0]) { const double d = (double)p.series[(size_t)d0 * p.nout + t] - p.mean[d0]; *a = (float)d; }
  if (d1 < p.ndm && p.live[d1]) { const double d = (double)p.series[(size_t)d1 * p.nout + t] - p.mean[d1]; *b = (float)d; }
}

// grid (n / 256, npair): work[pair][bitrev(t)] = z[t]
KERNEL(frbch_post_ps_load, PsParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint32_t t = (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid;
    if (t < p.n) {
      float a, b;
      ps_sample(p, by, t, &a, &b);
      float* z = p.work + ((size_t)by * p.n + (size_t)rfi_bitrev((int)t, p.log2n)) * 2;
      z[0] = a; z[1] = b;
    }
  }
}

// grid (n / 512, npair): stage p.stage, one butterfly a thread
KERNEL(frbch_post_ps_stage, PsParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint32_t i = (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid;
    if (i < p.n / 2) {
      const int s = p.stage;
      const uint32_t half = 1u << (s - 1);
      const uint32_t j = i & (half - 1);
      const uint32_t u = ((i >> (s - 1)) << s) + j, v = u + half;
      const uint32_t k = j << (p.log2n - s);
      float* z = p.work + (size_t)by * p.n * 2;
      rfi_bfly(z[2 * (size_t)u], z[2 * (size_t)u + 1], z[2 * (size_t)v], z[2 * (size_t)v + 1], p.tw[2 * (size_t)k], p.tw[2 * (size_t)k + 1]);
    }
  }
}

// grid (n / 512, npair): N[k] of both series of the pair; bin 0 holds 0
KERNEL(frbch_post_ps_power, PsParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint32_t k = (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid;
    const uint32_t nh = p.n / 2;
    if (k < nh) {
      float n0 = 0.f, n1 = 0.f;
      if (k) {
        const float* z = p.work + (size_t)by * p.n * 2;
        rfi_bins(z[2 * (size_t)k], z[2 * (size_t)k + 1], z[2 * (size_t)(p.n - k)], z[2 * (size_t)(p.n - k) + 1], &n0, &n1);
      }
      const int d0 = 2 * by, d1 = d0 + 1;
      p.pw[(size_t)d0 * nh + k] = p.live[d0] ? n0 : 0.f;
      if (d1 < p.ndm) p.pw[(size_t)d1 * nh + k] = p.live[d1] ? n1 : 0.f;
    }
  }
}

// grid (ceil(nblk / 64), ndm), a thread per block of bins: the level m = (S - max) / (cnt - 1), then p[k] = N[k] / m in place
KERNEL(frbch_post_ps_norm, PsParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    POST_NO_CONTRACT
    const uint32_t b = (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid;
    if (b < p.nblk) {
      const uint32_t nh = p.n / 2;
      const uint32_t k0 = 1u + b * p.wblock, k1 = b + 1 == p.nblk ? nh : k0 + p.wblock;
      float* x = p.pw + (size_t)by * nh;
      double S = 0.0;
      float mx = 0.f;
      for (uint32_t k = k0; k < k1; ++k) {
        const float v = x[k];
        S = S + (double)v;
        if (v > mx) mx = v;
      }
      const double num = S - (double)mx;
      const double m = num / (double)(k1 - k0 - 1u);
      const bool ok = rfi_finite(m) && m > 0.0;
      for (uint32_t k = k0; k < k1; ++k) {
        float q = 0.f;
        if (ok && k >= p.kmin) { const double r = (double)x[k] / m; q = (float)r; }
        x[k] = q;
      }
    }
  }
}

// H_h[k]: j ascending, every addition rounded
DEVFN inline float ps_hsum(const float* x, uint32_t k, uint32_t h) {
  POST_NO_CONTRACT
  float acc = 0.f;
  for (uint32_t j = 1; j <= h; ++j) {
    const uint32_t i = (uint32_t)(((uint64_t)j * k + h / 2) / h);
    acc = acc + x[i];
  }
  return acc;
}

DEVFN inline void ps_append(const PsParams& p, int dm, uint32_t h, uint32_t k, float H) {
  const uint32_t i = ATOMIC_FETCH_ADD_U32(p.npeak, 1u);
  if (i < p.peak_cap) {
    PsPeak q;
    q.dm = (uint32_t)dm; q.h = h; q.k = k; q.H = H;
    p.peaks[i] = q;
  }
}

// The terms of all folds at bin k are p at the sixteen fractions m / 16 of k: term j of fold h is p[(j k + h / 2) / h] =
// p[(m k + 8) / 16] with m = 16 j / h (the same integer; m k < 2^25).  H_h[k] from the terms q[m - 1]: j ascending, every addition
// rounded.  (Constant trip counts and indices: the terms stay in registers.)
template <int H> DEVFN inline float ps_hsum_terms(const float (&q)[16]) {
  POST_NO_CONTRACT
  float acc = 0.f;
  for (int j = 1; j <= H; ++j) acc = acc + q[j * (16 / H) - 1];
  return acc;
}

// bin k of series dm: every fold's sum (sixteen loads serve all five), threshold and local-maximum test
DEVFN inline void ps_harm_bin(const PsParams& p, int dm, uint32_t k) {
  const uint32_t nh = p.n / 2;
  if (k < p.kmin || k < 1 || k >= nh) return;
  const float* x = p.pw + (size_t)dm * nh;
  uint32_t nf = 0;                                                   // folds whose range holds k
  while (nf < p.nfold && ((uint64_t)p.kmin << nf) <= k) ++nf;
  const uint32_t skip = (16u >> (nf - 1)) - 1u;                      // fold 2^(nf-1) needs the fractions m with m & skip == 0
  float q[16];
  for (int m = 1; m <= 16; ++m) q[m - 1] = ((uint32_t)m & skip) == 0u ? x[((uint32_t)m * k + 8u) >> 4] : 0.f;
  const float H[5] = {ps_hsum_terms<1>(q), ps_hsum_terms<2>(q), ps_hsum_terms<4>(q), ps_hsum_terms<8>(q), ps_hsum_terms<16>(q)};
  for (int f = 0; f < 5; ++f) {
    if ((uint32_t)f >= nf || !(H[f] >= p.thr[f])) continue;
    const uint32_t h = 1u << f;
    const uint64_t first = (uint64_t)h * p.kmin;
    if (k > first && !(H[f] > ps_hsum(x, k - 1, h))) continue;
    if (k + 1 < nh && !(H[f] >= ps_hsum(x, k + 1, h))) continue;
    ps_append(p, dm, h, k, H[f]);
  }
}

// grid (n / 512, ndm), a thread per bin
KERNEL(frbch_post_ps_harm, PsParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE { ps_harm_bin(p, by, (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid); }
}

// ---------------------------------------------------------------------------------------------------------------------
// Time-domain resampling for the acceleration search (frbch_resample_*, frbch_pasearch_*; include/frbch.h states the rule):
// out[trial][row][t] = x[row][u(t)], u(t) = t + (int64)rint(q (double)(t (t - n))), one double product per output and nothing
// that could contract.  A pure gather: the bytes of the output are those of the input.  Rows dm >= ndm of a trial (the zero
// partner of an odd last series) are written as 0.  The kernel below is the generic form; the fast form
// (kernels_post_fast.inc) stages the window of a tile of outputs through the LDS.
// ---------------------------------------------------------------------------------------------------------------------
struct ResParams {
  const float* series;         // [ndm][nout]; only positions < n are read
  uint64_t nout;
  uint32_t n;                  // outputs per row
  int ndm, rows_per_trial;     // rows_per_trial >= ndm: rows of a trial in `out`
  const double* q;             // [trials of this launch]
  float* out;                  // [trials of this launch][rows_per_trial][n]
};

// u(t) of the rule.  For an accepted q (|q| n <= 0.5) it lies in 0 .. n - 1; the clamp never moves it and is there so that no
// q whatever could take an address out of the row.
DEVFN inline uint32_t res_index(double q, uint32_t t, uint32_t n) {
  POST_NO_CONTRACT
  const int64_t prod = (int64_t)t * ((int64_t)t - (int64_t)n);
  const double g = rint(q * (double)prod);
  int64_t u = (int64_t)t + (int64_t)g;
  if (u < 0) u = 0;
  if (u > (int64_t)n - 1) u = (int64_t)n - 1;
  return (uint32_t)u;
}

// grid (n / 256, trials * rows_per_trial), one output per thread
KERNEL(frbch_post_resample, ResParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const uint32_t t = (uint32_t)bx * (uint32_t)nthr + (uint32_t)tid;
    if (t < p.n) {
      const int trial = by / p.rows_per_trial, dm = by - trial * p.rows_per_trial;
      float v = 0.f;
      if (dm < p.ndm) v = p.series[(size_t)dm * p.nout + res_index(p.q[trial], t, p.n)];
      p.out[(size_t)by * p.n + t] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Burst polarisation (frbch_burstspec_*, frbch_rmsynth_*; include/frbch.h states the arithmetic).  The sums of a burst's
// three windows for every (candidate, product, channel), and the integer transform of Q and U over the Faraday depths.
// The kernels below are the generic forms; the fast forms (kernels_post_fast.inc) give the same bits.
// ---------------------------------------------------------------------------------------------------------------------
struct BurstCand {
  long long on_lo;             // first on-pulse row at the top of the band: sample - width / 2 (may be negative)
  uint32_t width, off_gap, off_len, pad;
};
struct BurstSums { double on_sum, off_sum, off_sumsq; uint32_t on_hits, off_hits; };   // frbch_burst_sums
struct BurstParams {
  const uint8_t* rows;         // [nrows][nifs][nchan] samples of `nbits`; every product is read
  uint64_t nrows;
  int nchan, nifs, nbits, ncand;
  const BurstCand* cand;       // [ncand]
  const int32_t* delays;       // [ncand][nchan]
  BurstSums* sums;             // [ncand][nifs][nchan]
};

// window w of a candidate in ascending row order: 0 = the earlier off-pulse window, 1 = on-pulse, 2 = the later off-pulse window
DEVFN inline void burst_window(const BurstCand& cd, int w, long long* w0, uint32_t* len) {
  if (w == 0) { *w0 = cd.on_lo - (long long)cd.off_gap - (long long)cd.off_len; *len = cd.off_len; }
  else if (w == 1) { *w0 = cd.on_lo; *len = cd.width; }
  else { *w0 = cd.on_lo + (long long)cd.width + (long long)cd.off_gap; *len = cd.off_len; }
}
// present rows of window [w0, w0 + len) read at delay n: [lo, hi) of the file
DEVFN inline void burst_clip(long long w0, uint32_t len, long long n, long long nrows, long long* lo, long long* hi) {
  long long a = w0 + n, b = w0 + n + (long long)len;
  if (a < 0) a = 0;
  if (b > nrows) b = nrows;
  if (b < a) b = a;
  *lo = a;
  *hi = b;
}

// grid (ceil(nchan / 256), ncand * nifs), one thread per (candidate, product, channel), rows ascending
KERNEL(frbch_post_burst_sums, BurstParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    POST_NO_CONTRACT
    const int c = bx * nthr + tid;
    const int cand = by / p.nifs, pr = by - cand * p.nifs;
    if (c < p.nchan) {
      const BurstCand cd = p.cand[cand];
      const long long n = (long long)p.delays[(size_t)cand * p.nchan + c];
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const uint64_t first = (uint64_t)pr * (uint64_t)p.nchan + (uint64_t)c;
      unsigned long long si[2] = {0, 0}, qi = 0;       // [0] on, [1] off
      double sf[2] = {0.0, 0.0}, qf = 0.0;
      uint32_t hits[2] = {0, 0};
      for (int w = 0; w < 3; ++w) {
        long long w0, lo, hi;
        uint32_t len;
        burst_window(cd, w, &w0, &len);
        burst_clip(w0, len, n, (long long)p.nrows, &lo, &hi);
        const int a = w == 1 ? 0 : 1;
        hits[a] += (uint32_t)(hi - lo);
        if (p.nbits == 32) {
          const float* x = (const float*)p.rows;
          for (long long t = lo; t < hi; ++t) {
            const double v = (double)x[(uint64_t)t * pitch + first];
            const double vv = v * v;
            sf[a] = sf[a] + v;
            if (a) qf = qf + vv;
          }
        } else {
          for (long long t = lo; t < hi; ++t) {
            const unsigned long long v = p.nbits == 8 ? (unsigned long long)p.rows[(uint64_t)t * pitch + first]
                                                      : (unsigned long long)((const uint16_t*)p.rows)[(uint64_t)t * pitch + first];
            si[a] += v;
            if (a) qi += v * v;
          }
        }
      }
      BurstSums o;
      o.on_sum = p.nbits == 32 ? sf[0] : (double)si[0];
      o.off_sum = p.nbits == 32 ? sf[1] : (double)si[1];
      o.off_sumsq = p.nbits == 32 ? qf : (double)qi;
      o.on_hits = hits[0];
      o.off_hits = hits[1];
      p.sums[((size_t)cand * p.nifs + pr) * p.nchan + c] = o;
    }
  }
}

struct RmRec { int32_t qi, ui; unsigned long long p0, d; };    // one used channel of a candidate: 24 bytes
struct RmCand { uint32_t nrec, pad; double inv; };             // used channels (the records are packed); inv_i of the rule
struct RmParams {
  const RmRec* rec;            // [ncand][nchan], the first nrec of a candidate are its used channels in ascending c
  const RmCand* cand;          // [ncand]
  const int32_t* table;        // C[16384]
  float* out;                  // [ncand][nphi][2]
  long long* part;             // fast kernel with nsplit > 1: [nsplit][ncand][nphi][2]
  int nchan, nphi, ncand, nsplit, chunk, pad;
};

// one term of the transform: the table index of phase ph, and the four products
DEVFN inline void rm_term(const int32_t* tab, unsigned long long ph, int32_t qi, int32_t ui, long long* re, long long* im) {
  const int j = (int)(((ph + (1ull << 49)) >> 50) & 16383ull);
  const long long cj = tab[j], sj = tab[(j - 4096) & 16383];
  *re += (long long)qi * cj + (long long)ui * sj;
  *im += (long long)ui * cj - (long long)qi * sj;
}
DEVFN inline void rm_store(float* out, long long re, long long im, double inv) {
  POST_NO_CONTRACT
  out[0] = (float)((double)re * inv);
  out[1] = (float)((double)im * inv);
}

// grid (ceil(nphi / 256), ncand), one thread per (candidate, trial), channels ascending, the table in global memory
KERNEL(frbch_post_rm, RmParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int k = bx * nthr + tid;
    if (k < p.nphi) {
      const RmCand cd = p.cand[by];
      const RmRec* rec = p.rec + (size_t)by * p.nchan;
      long long re = 0, im = 0;
      for (uint32_t r = 0; r < cd.nrec; ++r) {
        const RmRec rc = rec[r];
        rm_term(p.table, rc.p0 + rc.d * (unsigned long long)k, rc.qi, rc.ui, &re, &im);
      }
      rm_store(p.out + ((size_t)by * p.nphi + k) * 2, re, im, cd.inv);
    }
  }
}

// The delay x RM transform (frbch_rmdelay_*): a second axis on the transform above, ph = p0 + k d + m e with the first tau
// trial's phase folded into p0.  Every term goes through rm_term, so this kernel and the fast one differ in schedule only.
struct RmdRec { int32_t qi, ui; unsigned long long p0, d, e; };   // one used channel of a candidate: 32 bytes
struct RmdParams {
  const RmdRec* rec;           // [ncand][nchan], packed as RmParams::rec
  const RmCand* cand;          // [ncand]
  const int32_t* table;        // C[16384]
  float* out;                  // [ncand][ntau][nphi][2]
  long long* part;             // fast kernel with nsplit > 1: [nsplit][ncand][ntau][nphi][2]
  int nchan, nphi, ntau, ncand, nsplit, chunk;
};

// grid (ceil(ntau nphi / 256), ncand), one thread per (candidate, tau trial, phi trial), channels ascending
KERNEL(frbch_post_rmd, RmdParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ntau * p.nphi) {
      const unsigned long long m = (unsigned long long)(idx / p.nphi), k = (unsigned long long)(idx % p.nphi);
      const RmCand cd = p.cand[by];
      const RmdRec* rec = p.rec + (size_t)by * p.nchan;
      long long re = 0, im = 0;
      for (uint32_t r = 0; r < cd.nrec; ++r) {
        const RmdRec rc = rec[r];
        rm_term(p.table, rc.p0 + rc.d * k + rc.e * m, rc.qi, rc.ui, &re, &im);
      }
      rm_store(p.out + ((size_t)by * p.ntau * p.nphi + (size_t)idx) * 2, re, im, cd.inv);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Polarisation profile of a burst (frbch_polprof_*; include/frbch.h states the arithmetic): per (candidate, time bin) the
// band sum of I, V and of (Q, U) rotated back by the RM, in int64.  Every channel's part of a bin goes through pp_term in
// both forms, so the generic kernel below and the fast one (kernels_post_fast.inc) differ in schedule only; the sums are
// exact, so they give the same bits.
// ---------------------------------------------------------------------------------------------------------------------
struct PolRec {                // one channel of a candidate: 80 bytes
  double mean[4], g[4];        // the off-pulse mean and the gain of every product
  int32_t cc, sc;              // C[j], S[j] of the channel's rotation
  int32_t delay;               // n_c(dm)
  uint32_t used;
};
struct PolCand { long long t0; double scale; };   // first row of bin 0 at the top of the band; 2^k
struct PolParams {
  const uint8_t* rows;         // [nrows][4][nchan] samples of `nbits` (8 or 16)
  uint64_t nrows;
  int nchan, nifs, nbits, ncand;
  const PolCand* cand;         // [ncand]
  const PolRec* rec;           // [ncand][nchan]
  long long* acc;              // [ncand][nbin][4]: I, Re, Im, V
  uint32_t* hits;              // [ncand][nbin]
  long long* part;             // fast kernel: [ncand][ntile][nbin][4]
  uint32_t* hpart;             // fast kernel: [ncand][ntile][nbin]
  int nbin, tfactor, coh, ntile, brun, pad;
};

// the part of one channel in one bin: S[p] the sums of its h present rows
DEVFN inline void pp_term(const PolRec& r, int coh, double scale, const uint32_t* S, uint32_t h, long long* a) {
  POST_NO_CONTRACT
  double x[4];
  for (int pr = 0; pr < 4; ++pr) {
    const double m = (double)h * r.mean[pr];
    const double d = (double)S[pr] - m;
    x[pr] = d * r.g[pr];
  }
  double xi = x[0], xq = x[1], xu = x[2], xv = x[3];
  if (coh) { xi = x[0] + x[1]; xq = 2.0 * x[2]; xu = 2.0 * x[3]; xv = x[0] - x[1]; }
  const long long Xi = (long long)rint(xi * scale), Xq = (long long)rint(xq * scale);
  const long long Xu = (long long)rint(xu * scale), Xv = (long long)rint(xv * scale);
  const long long cj = r.cc, sj = r.sc;
  a[0] += Xi;
  a[1] += Xq * cj + Xu * sj;
  a[2] += Xu * cj - Xq * sj;
  a[3] += Xv;
}

// grid (ceil(nbin / 256), ncand), one thread per (candidate, bin), channels ascending, rows ascending
KERNEL(frbch_post_polprof, PolParams) {
  K_PROLOGUE;
  (void)smem;
  PHASE {
    const int j = bx * nthr + tid;
    if (j < p.nbin) {
      const PolCand cd = p.cand[by];
      const PolRec* rec = p.rec + (size_t)by * p.nchan;
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const long long b0 = cd.t0 + (long long)j * (long long)p.tfactor;
      long long a[4] = {0, 0, 0, 0};
      uint32_t hits = 0;
      for (int c = 0; c < p.nchan; ++c) {
        if (!rec[c].used) continue;
        long long lo, hi;
        burst_clip(b0, (uint32_t)p.tfactor, (long long)rec[c].delay, (long long)p.nrows, &lo, &hi);
        if (hi <= lo) continue;
        uint32_t S[4] = {0, 0, 0, 0};
        for (long long t = lo; t < hi; ++t)
          for (int pr = 0; pr < 4; ++pr) {
            const uint64_t o = (uint64_t)t * pitch + (uint64_t)pr * (uint64_t)p.nchan + (uint64_t)c;
            S[pr] += p.nbits == 8 ? (uint32_t)p.rows[o] : (uint32_t)((const uint16_t*)p.rows)[o];
          }
        pp_term(rec[c], p.coh, cd.scale, S, (uint32_t)(hi - lo), a);
        hits += (uint32_t)(hi - lo);
      }
      long long* o = p.acc + ((size_t)by * p.nbin + j) * 4;
      o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
      p.hits[(size_t)by * p.nbin + j] = hits;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// DM of a burst (frbch_dmscan_*; include/frbch.h states the arithmetic): per (candidate, trial DM, time bin) the band sum of
// the baseline-free, noise-weighted samples read at the trial's delays, in int64.  Every channel's part of a bin goes through
// dm_term in both forms, so the generic kernel below and the fast one (kernels_post_fast.inc) differ in schedule only; the
// sums are exact, so they give the same bits.
// ---------------------------------------------------------------------------------------------------------------------
struct DmRec {                 // one channel of a candidate: 24 bytes
  double mean, w;              // the off-pulse mean (over the products read) and 1 / sqrt(var_c)
  uint32_t used, pad;
};
struct DmCand { long long t0; double scale; };    // first row of bin 0 at the top of the band; 2^k
struct DmParams {
  const uint8_t* rows;         // [nrows][nifs][nchan] samples of `nbits` (8 or 16)
  uint64_t nrows;
  int nchan, nifs, nbits, ncand;
  const DmCand* cand;          // [ncand]
  const DmRec* rec;            // [ncand][nchan]
  const int32_t* delays;       // [ncand][ntrial][nchan]: n_c(dm_k)
  long long* acc;              // [ncand][ntrial][nbin]
  uint32_t* hits;              // [ncand][ntrial][nbin]
  long long* part;             // fast kernel: [ncand][ntile][ntrial][nbin]
  uint32_t* hpart;             // fast kernel: the same shape
  int ntrial, nbin, tfactor, p0, np, ntile, trun, brun;      // p0, np: the first product read and their number (1 or 2)
};

// the part of one channel in one bin of one trial: S the sum of its h present rows over the products read
DEVFN inline long long dm_term(double mean, double w, double scale, uint32_t S, uint32_t h) {
  POST_NO_CONTRACT
  const double m = (double)h * mean;
  const double d = (double)S - m;
  const double x = d * w;
  return (long long)rint(x * scale);
}

// grid (ceil(ncand ntrial nbin / 256)), one thread per (candidate, trial, bin), channels ascending, rows ascending
KERNEL(frbch_post_dmscan, DmParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ncand * p.ntrial * p.nbin) {
      const int j = (int)(idx % p.nbin);
      const long long ik = idx / p.nbin;                       // candidate * ntrial + trial
      const int cand = (int)(ik / p.ntrial);
      const DmCand cd = p.cand[cand];
      const DmRec* rec = p.rec + (size_t)cand * p.nchan;
      const int32_t* dl = p.delays + (size_t)ik * p.nchan;
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const long long b0 = cd.t0 + (long long)j * (long long)p.tfactor;
      long long a = 0;
      uint32_t hits = 0;
      for (int c = 0; c < p.nchan; ++c) {
        if (!rec[c].used) continue;
        long long lo, hi;
        burst_clip(b0, (uint32_t)p.tfactor, (long long)dl[c], (long long)p.nrows, &lo, &hi);
        if (hi <= lo) continue;
        uint32_t S = 0;
        for (long long t = lo; t < hi; ++t)
          for (int pr = p.p0; pr < p.p0 + p.np; ++pr) {
            const uint64_t o = (uint64_t)t * pitch + (uint64_t)pr * (uint64_t)p.nchan + (uint64_t)c;
            S += p.nbits == 8 ? (uint32_t)p.rows[o] : (uint32_t)((const uint16_t*)p.rows)[o];
          }
        a += dm_term(rec[c].mean, rec[c].w, cd.scale, S, (uint32_t)(hi - lo));
        hits += (uint32_t)(hi - lo);
      }
      p.acc[idx] = a;
      p.hits[idx] = hits;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Structure of a burst (frbch_burstacf_*, frbch_acf2d_*; include/frbch.h states the arithmetic): the dedispersed dynamic
// spectrum per (candidate, subband, bin) from the same dm_term as the DM scan, its largest complete cell, the quantised
// int32 plane, and the two-dimensional autocorrelation of such a plane in int64.  Every sum is an exact integer sum, so the
// generic kernels below and the fast ones (kernels_post_fast.inc) differ in schedule only.
// ---------------------------------------------------------------------------------------------------------------------
struct DynParams {
  const uint8_t* rows;         // [nrows][nifs][nchan] samples of `nbits` (8 or 16)
  uint64_t nrows;
  int nchan, nifs, nbits, ncand;
  const DmCand* cand;          // [ncand]
  const DmRec* rec;            // [ncand][nchan]
  const int32_t* delays;       // [ncand][nchan]: n_c(cand.dm)
  const uint32_t* nused_s;     // [ncand][nsub]: the used channels of a subband
  long long* Y;                // [ncand][nsub][nbin]
  uint32_t* yhits;             // [ncand][nsub][nbin]
  long long* part;             // fast kernel, join form: [ncand][ntile][nbin]
  uint32_t* hpart;             // the same shape
  long long* rowmax;           // [ncand][nsub]: the largest |Y| over the complete cells of a subband
  int32_t* shift;              // [ncand]: r_i
  int32_t* y;                  // [ncand][nsub][nbin]
  int32_t* mask;               // [ncand][nsub][nbin]: 1 = complete
  int nsub, nbin, tfactor, ffactor, p0, np, ntile, brun, gl;      // gl: the lanes a shuffle reduction spans (fast kernel)
};

// grid (ceil(ncand nsub nbin / 256)), one thread per (candidate, subband, bin), channels ascending, rows ascending
KERNEL(frbch_post_dynspec, DynParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ncand * p.nsub * p.nbin) {
      const int j = (int)(idx % p.nbin);
      const long long is = idx / p.nbin;                       // candidate * nsub + subband
      const int cand = (int)(is / p.nsub), s = (int)(is % p.nsub);
      const DmCand cd = p.cand[cand];
      const DmRec* rec = p.rec + (size_t)cand * p.nchan;
      const int32_t* dl = p.delays + (size_t)cand * p.nchan;
      const uint64_t pitch = (uint64_t)p.nifs * (uint64_t)p.nchan;
      const long long b0 = cd.t0 + (long long)j * (long long)p.tfactor;
      long long a = 0;
      uint32_t hits = 0;
      for (int c = s * p.ffactor; c < (s + 1) * p.ffactor; ++c) {
        if (!rec[c].used) continue;
        long long lo, hi;
        burst_clip(b0, (uint32_t)p.tfactor, (long long)dl[c], (long long)p.nrows, &lo, &hi);
        if (hi <= lo) continue;
        uint32_t S = 0;
        for (long long t = lo; t < hi; ++t)
          for (int pr = p.p0; pr < p.p0 + p.np; ++pr) {
            const uint64_t o = (uint64_t)t * pitch + (uint64_t)pr * (uint64_t)p.nchan + (uint64_t)c;
            S += p.nbits == 8 ? (uint32_t)p.rows[o] : (uint32_t)((const uint16_t*)p.rows)[o];
          }
        a += dm_term(rec[c].mean, rec[c].w, cd.scale, S, (uint32_t)(hi - lo));
        hits += (uint32_t)(hi - lo);
      }
      p.Y[idx] = a;
      p.yhits[idx] = hits;
    }
  }
}

DEVFN inline bool acf_complete(uint32_t nused_s, uint32_t yhits, int tfactor) { return nused_s > 0 && yhits == (uint32_t)tfactor * nused_s; }

// grid (ceil(ncand nsub / 256)), one thread per (candidate, subband): the largest |Y| over its complete cells
KERNEL(frbch_post_acf_rowmax, DynParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long is = (long long)bx * nthr + tid;
    if (is < (long long)p.ncand * p.nsub) {
      const uint32_t nu = p.nused_s[is];
      long long m = 0;
      for (int j = 0; j < p.nbin; ++j) {
        const long long v = p.Y[(size_t)is * p.nbin + j];
        if (acf_complete(nu, p.yhits[(size_t)is * p.nbin + j], p.tfactor)) m = m > (v < 0 ? -v : v) ? m : (v < 0 ? -v : v);
      }
      p.rowmax[is] = m;
    }
  }
}

// grid (ceil(ncand / 256)), one thread per candidate: m_i, and from its bit length the shift r_i
KERNEL(frbch_post_acf_shift, DynParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const int cand = bx * nthr + tid;
    if (cand < p.ncand) {
      long long m = 0;
      for (int s = 0; s < p.nsub; ++s) m = m > p.rowmax[(size_t)cand * p.nsub + s] ? m : p.rowmax[(size_t)cand * p.nsub + s];
      int b = 0;
      while (m) { ++b; m >>= 1; }
      p.shift[cand] = b > 21 ? b - 21 : 0;
    }
  }
}

// grid (ceil(ncand nsub nbin / 256)), one thread per cell: y and the 0 / 1 plane of the complete cells
KERNEL(frbch_post_acf_quant, DynParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ncand * p.nsub * p.nbin) {
      const long long is = idx / p.nbin;
      const int r = p.shift[is / p.nsub];
      const bool ok = acf_complete(p.nused_s[is], p.yhits[idx], p.tfactor);
      const long long v = p.Y[idx];
      p.y[idx] = !ok ? 0 : (int32_t)(r > 0 ? (v + (1ll << (r - 1))) >> r : v);
      p.mask[idx] = ok ? 1 : 0;
    }
  }
}

struct Acf2Params {
  const int32_t* y;            // [n][nsub][nbin], |y| <= 2^21
  long long* A;                // [n][nlagf][2 nlagt - 1]
  long long* part;             // fast kernel: [n][nslab][nlagf][2 nlagt - 1]
  int n, nsub, nbin, nlagf, nlagt;
  int sb, dfr, nrun, nrunp, bw, nslab;       // fast kernel: the plan (acf2_plan_rule)
};

// grid (ceil(n nlagf (2 nlagt - 1) / 256)), one thread per (plane, df, dt), s then j ascending
KERNEL(frbch_post_acf2d, Acf2Params) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const int ndt = 2 * p.nlagt - 1;
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.n * p.nlagf * ndt) {
      const int dt = (int)(idx % ndt) - (p.nlagt - 1);
      const int df = (int)((idx / ndt) % p.nlagf);
      const int32_t* y = p.y + (size_t)(idx / ((long long)ndt * p.nlagf)) * p.nsub * p.nbin;
      const int jlo = dt < 0 ? -dt : 0, jhi = dt > 0 ? p.nbin - dt : p.nbin;
      long long a = 0;
      for (int s = 0; s + df < p.nsub; ++s) {
        const int32_t* u = y + (size_t)s * p.nbin;
        const int32_t* v = y + (size_t)(s + df) * p.nbin + dt;
        for (int j = jlo; j < jhi; ++j) a += (long long)u[j] * (long long)v[j];
      }
      p.A[idx] = a;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Scattering of a burst, the template-bank stage (frbch_tbank_*, frbch_burstscat_*; include/frbch.h states the arithmetic):
// C[plane][s][k][u] = the sum over the taps m of y[plane][s][shift0 + u - lead + m] P[k][m], int64, terms whose bin lies
// outside the row absent.  |y| <= 2^21, |P| <= 2^30, ntap <= 1024: every sum is below 2^61 and exact in any order, so the
// generic kernel below and the fast one (kernels_post_fast.inc) differ in schedule only.
// ---------------------------------------------------------------------------------------------------------------------
struct TbankParams {
  const int32_t* y;            // [n][nsub][nbin], |y| <= 2^21
  const int32_t* P;            // [ntemp][ntap], |P| <= 2^30
  long long* C;                // [n][nsub][ntemp][nshift]
  int n, nsub, nbin, ntemp, ntap, lead, shift0, nshift;
  int sw, kr, nrun, nrunp, lw, ntap8;        // fast kernel: the plan (tbank_plan_rule)
};

// grid (ceil(n nsub ntemp nshift / 256)), one thread per (plane, subband, template, shift), taps ascending
KERNEL(frbch_post_tbank, TbankParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.n * p.nsub * p.ntemp * p.nshift) {
      const int u = (int)(idx % p.nshift);
      const int k = (int)((idx / p.nshift) % p.ntemp);
      const int32_t* y = p.y + (size_t)(idx / ((long long)p.nshift * p.ntemp)) * p.nbin;      // row (plane, s)
      const int32_t* t = p.P + (size_t)k * p.ntap;
      const int j0 = p.shift0 + u - p.lead;                                                  // the bin of tap 0
      const int mlo = j0 < 0 ? -j0 : 0, mhi = p.nbin - j0 < p.ntap ? p.nbin - j0 : p.ntap;
      long long a = 0;
      for (int m = mlo; m < mhi; ++m) a += (long long)y[j0 + m] * (long long)t[m];
      p.C[idx] = a;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Refinement of a fold (frbch_foldfit_*; include/frbch.h states the arithmetic): the folded cube of frbch_foldp_* is shifted
// per channel over a run of DMs (stage 1) and per sub-integration over a grid of spin offsets (stage 2), in exact integers,
// and every trial profile is scored in double with a fixed summation order.  The integer sums are exact in any order, the
// score goes through ff_term and the 64 partial sums of the header, so the generic kernels below and the fast ones
// (kernels_post_fast.inc) differ in schedule only.
// ---------------------------------------------------------------------------------------------------------------------
struct FfParams {
  const double* cube;          // [nsub][nifs][nbin][nchan], exact integers (frbch_foldp_*)
  const uint32_t* chits;       // [nsub][nbin][nchan]
  const uint8_t* use;          // [nchan]: 1 = the channel is added
  const int32_t* shd;          // [ndm][nchan], 0 .. nbin - 1
  const int32_t* shp;          // [nspin][nsub]: (-shP) mod nbin, 0 .. nbin - 1 (frbch_post_ff_prof: [ntrial][nsub], the listed trials')
  const uint32_t* trial;       // frbch_post_ff_prof: [ntrial], a listed trial as dm * nspin + spin
  long long* A;                // [ndm][nsub][nbin]
  unsigned long long* HA;      // [ndm][nsub][nbin]
  long long* totA;             // [ndm][nsub]: the sum of A over the bins
  unsigned long long* totH;    // [ndm][nsub]
  double* score;               // [ntrial] or NULL
  long long* pacc;             // [ntrial][nbin] or NULL: the trial profiles
  unsigned long long* phits;   // [ntrial][nbin] or NULL
  long long* part;             // fast stage 1 with ngrp > 1: [ngrp][ndm][nsub][nbin]
  uint32_t* hpart;             // the same shape
  int nchan, nifs, nbin, nsub, ndm, nspin, ntrial, products;   // nspin = nfdot * nfreq
  int ngrp, sc, lstride, nrun;                                  // fast kernels: the plan (ff_plan_rule)
};

// the masked products of one (sub-integration, bin, channel)
DEVFN inline long long ff_sample(const FfParams& p, int s, int b, int c) {
  long long v = 0;
  for (int q = 0; q < p.nifs; ++q)
    if ((p.products >> q) & 1) v += (long long)p.cube[(((size_t)s * p.nifs + q) * p.nbin + b) * p.nchan + c];
  return v;
}

// stage 1: grid (ceil(ndm nsub nbin / 256)), one thread per (DM, sub-integration, bin), channels ascending
KERNEL(frbch_post_ff_dm, FfParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ndm * p.nsub * p.nbin) {
      const int b = (int)(idx % p.nbin);
      const int s = (int)((idx / p.nbin) % p.nsub);
      const int32_t* sh = p.shd + (size_t)(idx / ((long long)p.nbin * p.nsub)) * p.nchan;
      long long a = 0;
      unsigned long long h = 0;
      for (int c = 0; c < p.nchan; ++c) {
        if (!p.use[c]) continue;
        int j = b + sh[c];
        if (j >= p.nbin) j -= p.nbin;
        a += ff_sample(p, s, j, c);
        h += p.chits[((size_t)s * p.nbin + j) * p.nchan + c];
      }
      p.A[idx] = a;
      p.HA[idx] = h;
    }
  }
}

// the totals of a (DM, sub-integration): grid (ceil(ndm nsub / 256)), one thread each; both forms run it
KERNEL(frbch_post_ff_tot, FfParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ndm * p.nsub) {
      const long long* a = p.A + (size_t)idx * p.nbin;
      const unsigned long long* h = p.HA + (size_t)idx * p.nbin;
      long long ta = 0;
      unsigned long long th = 0;
      for (int b = 0; b < p.nbin; ++b) { ta += a[b]; th += h[b]; }
      p.totA[idx] = ta;
      p.totH[idx] = th;
    }
  }
}

// the part of one bin in the score of a trial (0 for a bin without hits, which leaves every partial sum as it is)
DEVFN inline double ff_term(long long B, unsigned long long H, double M) {
  POST_NO_CONTRACT
  if (!H) return 0.0;
  const double x = (double)B / (double)H;
  const double d = x - M;
  const double dd = d * d;
  return (double)H * dd;
}

// M of a DM from the totals of its sub-integrations; *any = 0: no hit at all
DEVFN inline double ff_mean(const FfParams& p, int k, int* any) {
  POST_NO_CONTRACT
  long long ta = 0;
  unsigned long long th = 0;
  for (int s = 0; s < p.nsub; ++s) { ta += p.totA[(size_t)k * p.nsub + s]; th += p.totH[(size_t)k * p.nsub + s]; }
  *any = th != 0;
  return th ? (double)ta / (double)th : 0.0;
}

// B and H of one bin of a trial
DEVFN inline void ff_bin(const FfParams& p, int k, const int32_t* sh, int b, long long* B, unsigned long long* H) {
  long long a = 0;
  unsigned long long h = 0;
  for (int s = 0; s < p.nsub; ++s) {
    int j = b + sh[s];
    if (j >= p.nbin) j -= p.nbin;
    const size_t at = ((size_t)k * p.nsub + s) * p.nbin + j;
    a += p.A[at];
    h += p.HA[at];
  }
  *B = a;
  *H = h;
}

// stage 2: grid (ceil(ntrial / 256)), one thread per trial; the 64 partial sums one after the other, each over its bins
// ascending, added as they are finished (ascending q)
KERNEL(frbch_post_ff_spin, FfParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    POST_NO_CONTRACT
    const long long t = (long long)bx * nthr + tid;
    if (t < (long long)p.ntrial) {
      const int k = (int)(t / p.nspin);
      const int32_t* sh = p.shp + (size_t)(t % p.nspin) * p.nsub;
      int any = 0;
      const double M = ff_mean(p, k, &any);
      double sum = 0.0;
      int nhit = 0;
      for (int q = 0; q < 64; ++q) {
        double part = 0.0;
        for (int b = q; b < p.nbin; b += 64) {
          long long B;
          unsigned long long H;
          ff_bin(p, k, sh, b, &B, &H);
          if (p.pacc) { p.pacc[(size_t)t * p.nbin + b] = B; p.phits[(size_t)t * p.nbin + b] = H; }
          if (H) ++nhit;
          part = part + ff_term(B, H, M);
        }
        sum = sum + part;
      }
      if (p.score) p.score[t] = any && nhit >= 2 ? sum : 0.0;
    }
  }
}

// the profiles of a short list of trials (the nominal and the best one): grid (ceil(ntrial nbin / 256)), one thread per (trial, bin)
KERNEL(frbch_post_ff_prof, FfParams) {
  K_PROLOGUE;
  (void)smem; (void)by;
  PHASE {
    const long long idx = (long long)bx * nthr + tid;
    if (idx < (long long)p.ntrial * p.nbin) {
      const long long t = idx / p.nbin;
      long long B;
      unsigned long long H;
      ff_bin(p, (int)(p.trial[t] / (uint32_t)p.nspin), p.shp + (size_t)t * p.nsub, (int)(idx % p.nbin), &B, &H);
      p.pacc[idx] = B;
      p.phits[idx] = H;
    }
  }
}
