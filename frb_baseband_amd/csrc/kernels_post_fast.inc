// Tiled incoherent dedispersion (HIP only; the generic frbch_post_dedisp of kernels_post.inc stays the emulable form and the
// fallback).  prepsubband's DM ranges (process_vdif.py:202-229: -lodm / -numdms / -dmstep) mean MANY series from the same rows:
// the per-sample kernel re-reads every row byte once per DM with lanes a whole row apart.  Here a workgroup owns 256
// consecutive output samples x ND consecutive DMs and walks the channels tile by tile (64 bytes of every row: 64 / 32 / 16
// channels of 8- / 16-bit / float samples), in ASCENDING channel order: the rows a tile needs -- [t0 + dmin, t0 + dmin +
// 256 + span), dmin / span over the tile's channels and the group's DMs, precomputed by the host -- are copied to the LDS
// once (coalesced 16-byte pieces, rows 68 bytes apart: lanes of one column read distinct banks), together with their clip
// flags and zero-DM row sums, and every thread adds its ND series from there.  Sums in double, channels ascending, exactly
// the order of frbch_post_dedisp and of oracle/post_oracle.py: float rows come out bit-identical, integer rows are exact.
namespace fast {
constexpr int kDedTT = 256, kDedRowB = 68, kDedND = 8;
constexpr int kDedRowsCap = 900;   // rows of a tile the LDS holds (61 KB of samples + 7 KB of row sums + flags)

template <int BPV, bool FLAGS, bool ZERODM>
__global__ void __launch_bounds__(256) frbch_post_dedisp_tiled(PostParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* tile = smem;                                              // [rows][68]
  double* rs = reinterpret_cast<double*>(smem + (size_t)kDedRowsCap * kDedRowB + 16);   // [rows] zero-DM row sums
  unsigned char* fl = reinterpret_cast<unsigned char*>(rs + kDedRowsCap);  // [rows] clip flags
  constexpr int CT = 64 / BPV;
  const int tid = threadIdx.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * kDedTT;
  const uint64_t t = t0 + tid;
  const int dm0 = blockIdx.y * kDedND;
  const int nd = min(kDedND, p.ndm - dm0);
  const int nct = p.nchan / CT;
  const size_t row_stride = (size_t)p.nifs * p.nchan * BPV;               // bytes between rows of the file
  const unsigned char* src0 = p.rows + (size_t)p.prod * p.nchan * BPV;
  double a[kDedND], b[kDedND];
#pragma unroll
  for (int d = 0; d < kDedND; ++d) a[d] = b[d] = 0.0;
  for (int ctile = 0; ctile < nct; ++ctile) {
    const int32_t dmin = p.tile_range[((size_t)blockIdx.y * nct + ctile) * 2];
    const int32_t span = p.tile_range[((size_t)blockIdx.y * nct + ctile) * 2 + 1];
    const int rows = kDedTT + span;                                        // <= kDedRowsCap (the host checked)
    const uint64_t r0 = t0 + (uint64_t)dmin;
    __syncthreads();                                                       // the previous tile is consumed
    for (int i = tid; i < rows * 4; i += 256) {                            // 16-byte pieces: 4 per row
      const int r = i >> 2, part = i & 3;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r0 + r < p.nrows) v = *reinterpret_cast<const uint4*>(src0 + (r0 + r) * row_stride + (size_t)ctile * 64 + part * 16);
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16) = v.x;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 4) = v.y;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 8) = v.z;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 12) = v.w;
    }
    if (ZERODM || FLAGS)
      for (int r = tid; r < rows; r += 256) {
        const bool in = r0 + r < p.nrows;
        if (ZERODM) rs[r] = in ? p.rowsum[r0 + r] : 0.0;
        if (FLAGS) fl[r] = in ? p.flagged[r0 + r] : 0;
      }
    __syncthreads();
    if (t < p.nout) {
      for (int cl = 0; cl < CT; ++cl) {
        const int c = ctile * CT + cl;
        const double rep = FLAGS ? p.repl[c] : 0.0;
#pragma unroll
        for (int d = 0; d < kDedND; ++d) {
          if (d < nd) {
            const int r = tid + p.delays[(size_t)(dm0 + d) * p.nchan + c] - dmin;
            double v;
            if (BPV == 1) v = (double)tile[r * kDedRowB + cl];
            else if (BPV == 2) v = (double)*reinterpret_cast<const uint16_t*>(tile + r * kDedRowB + cl * 2);
            else v = (double)*reinterpret_cast<const float*>(tile + r * kDedRowB + cl * 4);
            if (FLAGS && fl[r]) v = rep;
            a[d] += v;
            if (ZERODM) b[d] += rs[r];
          }
        }
      }
    }
  }
  if (t < p.nout) {
#pragma unroll
    for (int d = 0; d < kDedND; ++d)
      if (d < nd) {
        const double y = ZERODM ? a[d] - b[d] / (double)p.nchan : a[d];
        p.out[(size_t)(dm0 + d) * p.nout + t] = (float)y;
      }
  }
}

// Band-limited dedispersion, tiled form (frbch_dedisperse_bands_*; the generic frbch_post_dedisp_bands stays the emulable
// form and the fallback).  The schedule is frbch_post_dedisp_tiled's -- 256 output samples x kDedND DMs per workgroup, the
// rows of a channel tile staged through the LDS with their clip flags and row sums, channels ascending -- so the rows are
// read once per DM group whatever the number of bands.  8- / 16-bit rows only: the running sum over the channels is an
// exact integer (nchan <= 65536 samples of 16 bit fit uint32), and so is the running sum of the zero-DM row sums (below 2^48:
// exact in a double, its 64 bits).  A sub-band is a whole number of tiles (the host checked): behind the last tile of sub-band
// k the running sums are stored as the prefix at edge k + 1, pre[dm][k][t] (the prefix at edge 0 is 0 and is not stored).
// frbch_post_bands_ranges then forms band [a, b) as the difference of two prefixes: exact, whatever cancels.
template <int BPV, bool FLAGS, bool ZERODM>
__global__ void __launch_bounds__(256) frbch_post_dedisp_bands_tiled(PostParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* tile = smem;                                              // [rows][68]
  double* rs = reinterpret_cast<double*>(smem + (size_t)kDedRowsCap * kDedRowB + 16);   // [rows] zero-DM row sums
  unsigned char* fl = reinterpret_cast<unsigned char*>(rs + kDedRowsCap);  // [rows] clip flags
  constexpr int CT = 64 / BPV;
  const int tid = threadIdx.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * kDedTT;
  const uint64_t t = t0 + tid;
  const int dm0 = blockIdx.y * kDedND;
  const int nd = min(kDedND, p.ndm - dm0);
  const int nct = p.nchan / CT, tps = p.cps / CT;                          // channel tiles, tiles per sub-band
  const size_t row_stride = (size_t)p.nifs * p.nchan * BPV;
  const unsigned char* src0 = p.rows + (size_t)p.prod * p.nchan * BPV;
  uint32_t a[kDedND];
  double b[kDedND];
#pragma unroll
  for (int d = 0; d < kDedND; ++d) { a[d] = 0u; b[d] = 0.0; }
  for (int ctile = 0, left = tps, k = 0; ctile < nct; ++ctile) {
    const int32_t dmin = p.tile_range[((size_t)blockIdx.y * nct + ctile) * 2];
    const int32_t span = p.tile_range[((size_t)blockIdx.y * nct + ctile) * 2 + 1];
    const int rows = kDedTT + span;                                        // <= kDedRowsCap (the host checked)
    const uint64_t r0 = t0 + (uint64_t)dmin;
    __syncthreads();                                                       // the previous tile is consumed
    for (int i = tid; i < rows * 4; i += 256) {                            // 16-byte pieces: 4 per row
      const int r = i >> 2, part = i & 3;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (r0 + r < p.nrows) v = *reinterpret_cast<const uint4*>(src0 + (r0 + r) * row_stride + (size_t)ctile * 64 + part * 16);
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16) = v.x;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 4) = v.y;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 8) = v.z;
      *reinterpret_cast<uint32_t*>(tile + r * kDedRowB + part * 16 + 12) = v.w;
    }
    if (ZERODM || FLAGS)
      for (int r = tid; r < rows; r += 256) {
        const bool in = r0 + r < p.nrows;
        if (ZERODM) rs[r] = in ? p.rowsum[r0 + r] : 0.0;
        if (FLAGS) fl[r] = in ? p.flagged[r0 + r] : 0;
      }
    __syncthreads();
    if (t < p.nout) {
      for (int cl = 0; cl < CT; ++cl) {
        const int c = ctile * CT + cl;
        const uint32_t rep = FLAGS ? (uint32_t)p.repl[c] : 0u;             // (an integer on integer rows)
#pragma unroll
        for (int d = 0; d < kDedND; ++d) {
          if (d < nd) {
            const int r = tid + p.delays[(size_t)(dm0 + d) * p.nchan + c] - dmin;
            uint32_t v;
            if (BPV == 1) v = tile[r * kDedRowB + cl];
            else v = *reinterpret_cast<const uint16_t*>(tile + r * kDedRowB + cl * 2);
            if (FLAGS && fl[r]) v = rep;
            a[d] += v;
            if (ZERODM) b[d] += rs[r];
          }
        }
      }
      if (--left == 0) {                                                   // sub-band k ends with this tile
#pragma unroll
        for (int d = 0; d < kDedND; ++d)
          if (d < nd) {
            const size_t at = ((size_t)(dm0 + d) * p.bsub + k) * p.nout + t;
            p.pre[at] = a[d];
            if (ZERODM) p.prez[at] = b[d];
          }
        left = tps;
        ++k;
      }
    }
  }
}

// out[dm * nband + j][t] = (float)( (double)(pre_b - pre_a) - (zerodm ? (prez_b - prez_a) / nchan : 0) ) for band j = [a, b).
// grid (ceil(nout / 256), nband, ndm), one thread per output sample: two (four) coalesced loads, one coalesced store.
template <bool ZERODM>
__global__ void __launch_bounds__(256) frbch_post_bands_ranges(PostParams p) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.nout) return;
  const int j = blockIdx.y, dm = blockIdx.z;
  const int a = p.band_ab[2 * j], b = p.band_ab[2 * j + 1];
  const size_t base = (size_t)dm * p.bsub * p.nout + t;
  const uint32_t hi = p.pre[base + (size_t)(b - 1) * p.nout];
  const uint32_t lo = a ? p.pre[base + (size_t)(a - 1) * p.nout] : 0u;
  double y = (double)(hi - lo);
  if (ZERODM) {
    const double zh = p.prez[base + (size_t)(b - 1) * p.nout];
    const double zl = a ? p.prez[base + (size_t)(a - 1) * p.nout] : 0.0;
    y = y - (zh - zl) / (double)p.nchan;
  }
  p.out[((size_t)dm * p.nband + j) * p.nout + t] = (float)y;
}

// ---------------------------------------------------------------------------------------------------------------------
// All-product fold in the LDS (HIP only; frbch_post_foldp of kernels_post.inc stays the emulable form and the fallback).
// The production form: integer rows, no per-channel delays (what dspsr does with a filterbank), so the bin depends on the
// row only.  frbch_post_foldp_slots computes slot[t] = sub * nbin + bin ONCE per row (nchan times fewer fp64 phases) and
// counts the rows of every slot -- the hits are the same for every channel, frbch_post_foldp_hits copies them out.
// frbch_post_foldp_lds: a workgroup of 1024 threads owns (one product, a tile of CT channels, a run of rows inside one
// sub-integration) and keeps uint32 acc[nbin][CT] in the LDS.  A lane owns one dword of the row piece (4 / 2 channels of
// 8- / 16-bit samples); the CT * BPV / 4 lanes of a row piece sit side by side, and the 1024 / that many lane groups each
// walk a contiguous share of the run, 8 rows in flight per lane (non-temporal dword loads), summing in registers while
// the slot stays the same (a bin lasts several rows) and adding to the LDS when it changes.  Lane l's value k of bin b
// lives at column (k LPR + l + b LPR) mod CT: lanes of one row piece hit consecutive banks, and lane groups of one wave
// that are in different bins are rotated apart.  At the end every non-zero (bin, channel) goes to the 64-bit global sums
// with one atomic.  Integer sums are exact in any order: the result equals the generic kernel's to the bit.
constexpr int kFoldThreads = 1024, kFoldUnroll = 8;
constexpr size_t kFoldLdsBudget = 128 * 1024;      // acc[nbin][CT] (of 160 KiB per CU)
constexpr int kFoldWgPerCu = 2;                    // row runs are sized for about this many workgroups per CU
constexpr uint32_t kFoldNoSlot = 0xFFFFFFFFu;

__global__ void __launch_bounds__(256) frbch_post_foldp_slots(FoldpParams p) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= p.nrows) return;
  const uint64_t sub = t / p.rows_per_sub;               // < nsub = ceil(nrows / rows_per_sub)
  int s = 0;
  while (s + 1 < p.nseg && p.seg_row[s + 1] <= t) ++s;
  const uint32_t slot = (uint32_t)sub * (uint32_t)p.nbin + (uint32_t)foldp_bin(p, t, 0, s);
  p.slot[t] = slot;
  atomicAdd(p.slot_hits + slot, 1u);
}

__global__ void __launch_bounds__(256) frbch_post_foldp_hits(FoldpParams p) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;      // over [nsub * nbin][nchan]
  if (i < p.nconv) p.hits[i] = p.slot_hits[i / (uint64_t)p.nchan];
}

// grid (nsub * chunks_per_sub, ntile * nifs)
template <int BPV>
__global__ void __launch_bounds__(kFoldThreads) frbch_post_foldp_lds(FoldpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* acc = reinterpret_cast<uint32_t*>(smem);                    // [nbin][CT], columns rotated by bin * LPR
  constexpr int VPL = 4 / BPV;                                          // values per lane (one dword)
  const int tid = threadIdx.x;
  const int ct = p.ct, cmask = ct - 1, lpr = ct / VPL, nrg = kFoldThreads / lpr;
  const int tile = blockIdx.y % p.ntile, prod = blockIdx.y / p.ntile;
  const uint32_t sub = blockIdx.x / p.chunks_per_sub, chunk = blockIdx.x % p.chunks_per_sub;
  const uint64_t s0 = (uint64_t)sub * p.rows_per_sub;
  const uint64_t s1 = s0 + p.rows_per_sub < p.nrows ? s0 + p.rows_per_sub : p.nrows;
  const uint64_t r0 = s0 + (uint64_t)chunk * p.rows_per_chunk;
  if (r0 >= s1) return;                                                 // (the last sub-integration may be short; whole workgroup)
  const uint64_t r1 = r0 + p.rows_per_chunk < s1 ? r0 + p.rows_per_chunk : s1;
  const int nacc = p.nbin * ct;
  for (int i = tid; i < nacc; i += kFoldThreads) acc[i] = 0u;
  __syncthreads();
  const int g = tid / lpr, l = tid % lpr;
  const uint64_t rpg = (r1 - r0 + (uint64_t)nrg - 1) / (uint64_t)nrg;   // rows per lane group
  const uint64_t tb = r0 + (uint64_t)g * rpg;
  const uint64_t te = tb + rpg < r1 ? tb + rpg : r1;
  const size_t stride = (size_t)p.nifs * p.nchan * BPV;                 // bytes between rows of the file
  const unsigned char* src = p.rows + ((size_t)prod * p.nchan + (size_t)tile * ct) * BPV + (size_t)l * 4;
  const uint32_t base = sub * (uint32_t)p.nbin;
  uint32_t cur = kFoldNoSlot;
  uint32_t a[VPL];
#pragma unroll
  for (int k = 0; k < VPL; ++k) a[k] = 0u;
  auto to_lds = [&]() {
    if (cur == kFoldNoSlot) return;
    const int b = (int)(cur - base);
#pragma unroll
    for (int k = 0; k < VPL; ++k)
      if (a[k]) atomicAdd(acc + b * ct + ((k * lpr + l + b * lpr) & cmask), a[k]);
  };
  for (uint64_t t = tb; t < te; t += kFoldUnroll) {
    uint32_t v[kFoldUnroll], sl[kFoldUnroll];
#pragma unroll
    for (int u = 0; u < kFoldUnroll; ++u) {
      const bool in = t + u < te;
      v[u] = in ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(src + (t + u) * stride)) : 0u;
      sl[u] = in ? p.slot[t + u] : kFoldNoSlot;
    }
#pragma unroll
    for (int u = 0; u < kFoldUnroll; ++u) {
      if (sl[u] == kFoldNoSlot) continue;                               // past the end of this lane group's rows
      if (sl[u] != cur) {
        to_lds();
        cur = sl[u];
#pragma unroll
        for (int k = 0; k < VPL; ++k) a[k] = 0u;
      }
      if constexpr (BPV == 1) {
        a[0] += v[u] & 0xFFu;
        a[1] += (v[u] >> 8) & 0xFFu;
        a[2] += (v[u] >> 16) & 0xFFu;
        a[3] += v[u] >> 24;
      } else {
        a[0] += v[u] & 0xFFFFu;
        a[1] += v[u] >> 16;
      }
    }
  }
  to_lds();
  __syncthreads();
  unsigned long long* dst = p.prof_i + (((size_t)sub * p.nifs + prod) * p.nbin) * p.nchan + (size_t)tile * ct;
  for (int i = tid; i < nacc; i += kFoldThreads) {
    const int b = i >> p.ct_log2, ch = i & cmask;
    const int pos = (ch % VPL) * lpr + ch / VPL;                        // channel ch = value ch % VPL of lane ch / VPL
    const uint32_t v = acc[b * ct + ((pos + b * lpr) & cmask)];
    if (v) atomicAdd(dst + (size_t)b * p.nchan + ch, (unsigned long long)v);
  }
}
// ---------------------------------------------------------------------------------------------------------------------
// Single-pulse search in the LDS (HIP only; frbch_post_sp_quant + frbch_post_sp_search of kernels_post.inc stay the emulable
// form and the fallback).  A workgroup of 256 threads owns one DM and kSpTile consecutive start samples t.  It needs the
// quantised samples q[t0 - hmax .. t0 + kSpTile - 1 + hmax + wmax - 1], hmax = wmax / 2: wmax behind the last boxcar and
// the local-maximum window of the widest boxcar on both sides.  They are loaded ONCE, coalesced (lane i takes sample
// a + i, a + 256 + i, ...), normalised and quantised on the way in from the per-block (mean, 1 / sigma) table, and turned
// into one exclusive prefix sum P[0 .. n] of 64-bit integers (|q| <= 2^26 and n < 2^12: no overflow): every thread sums a
// run of kSpRun consecutive samples in registers, the run totals are scanned with wave shuffles and four wave totals,
// and the runs are written back.  From there S_w[t] = P[t - a + w] - P[t - a] is two LDS reads at stride 1 across the
// lanes (64-bit words, consecutive lanes on consecutive bank pairs: conflict-free).  Every (width, t) is first held
// against the threshold; only the rare survivors walk their local-maximum window.  Peaks go to the global list through
// an ordinary vector atomic counter (the host sorts).  LDS: 24 KiB of P + 32 bytes: six workgroups per CU.
// The host takes this kernel when kSpTile + 2 wmax <= kSpLdsN (wmax <= 512) and nout < 2^31 (32-bit sample indices).
constexpr int kSpTile = 2048, kSpLdsN = 3072, kSpThreads = 256, kSpRun = kSpLdsN / kSpThreads;
constexpr int kSpMaxWidth = (kSpLdsN - kSpTile) / 2;

__global__ void __launch_bounds__(kSpThreads) frbch_post_sp_search_lds(SpParams p) {
  __shared__ long long pre[kSpLdsN + 1];
  __shared__ long long wave_tot[kSpThreads / 64];
  const int tid = threadIdx.x, dm = blockIdx.y;
  const int nout = (int)p.nout;
  const int wmax = p.width[p.nwidth - 1], hmax = wmax / 2;
  const int t0 = (int)blockIdx.x * kSpTile;
  const int a = t0 - hmax;                                        // sample of P's first difference (may be negative)
  const int n = kSpTile + 2 * hmax + wmax - 1;                    // <= kSpLdsN - 1
  const float* x = p.series + (size_t)dm * p.nout;
  const double* st = p.stats + (size_t)dm * p.nblk * 2;
  const uint32_t blk_len = (uint32_t)p.blk_len;
  for (int i = tid; i < kSpLdsN; i += kSpThreads) {               // raw q first: pre[i + 1] = q[a + i], 0 outside the series
    const int g = a + i;
    long long v = 0;
    if (i < n && g >= 0 && g < nout) {
      uint32_t b = (uint32_t)g / blk_len;
      if (b >= p.nblk) b = p.nblk - 1;
      v = sp_quantise(x[g], st[2 * b], st[2 * b + 1]);
    }
    pre[i + 1] = v;
  }
  if (tid == 0) pre[0] = 0;
  __syncthreads();
  long long run[kSpRun], tot = 0;
#pragma unroll
  for (int k = 0; k < kSpRun; ++k) {
    tot += pre[tid * kSpRun + k + 1];
    run[k] = tot;
  }
  long long incl = tot;                                           // inclusive scan of the run totals over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long up = __shfl_up(incl, d, 64);
    if ((tid & 63) >= d) incl += up;
  }
  if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
  __syncthreads();                                                // (also: every run has been read)
  long long base = incl - tot;
  for (int wv = 0; wv < (tid >> 6); ++wv) base += wave_tot[wv];
#pragma unroll
  for (int k = 0; k < kSpRun; ++k) pre[tid * kSpRun + k + 1] = base + run[k];
  __syncthreads();
  for (int k = 0; k < p.nwidth; ++k) {
    const int w = p.width[k];
    if (w > nout) break;                                          // the widths ascend
    const long long thr = p.thr[k];
    const int h = w / 2, last = nout - w;
    for (int j = tid; j < kSpTile; j += kSpThreads) {
      const int t = t0 + j;
      if (t > last) break;
      const int li = t - a;
      const long long s = pre[li + w] - pre[li];
      if (s < thr) continue;
      const int lo = t - h > 0 ? t - h : 0, hi = t + h < last ? t + h : last;
      bool peak = true;
      for (int u = lo; u < t && peak; ++u) peak = s > pre[u - a + w] - pre[u - a];
      for (int u = t + 1; u <= hi && peak; ++u) peak = s >= pre[u - a + w] - pre[u - a];
      if (peak) sp_append(p, dm, w, (uint64_t)t, s);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Candidate cut-outs in the LDS (HIP only; frbch_post_cutout of kernels_post.inc stays the emulable form and the fallback).
// One launch per plane kind for ALL candidates: grid (time tile, group of kCutNR plane rows, candidate).  A plane row is a
// trial DM (KIND 1, the DM-time plane) or a frequency bin (KIND 0, the frequency-time plane).  The shape is that of
// frbch_post_dedisp_tiled: a workgroup of 256 threads owns kCutNR plane rows and a run of whole time bins of one
// candidate -- bpt = 256 / tfactor bins, bpt * tfactor <= 256 consecutive ROWS, one row per thread -- and walks the 64-byte
// channel tiles in ascending order.  The rows a tile needs, [first row + dmin, ... + 256 + span) with dmin / span over the
// tile's channels and the group's plane rows precomputed by the host, are copied to the LDS once (coalesced 16-byte
// pieces, rows 68 bytes = 17 banks apart: the lanes of a wave read consecutive rows of one column, 64 distinct banks);
// rows outside [0, nrows) are zero-filled.  Every thread adds its row's samples into kCutNR uint32 accumulators (at most
// 2 rows x 16384 channels x 65535 < 2^32: exact), and keeps them across ALL channel tiles, so the DM-time plane needs no
// global atomics.  A bin longer than 256 rows (tfactor up to 512) is one workgroup's: it walks the bin in chunks of 256
// rows with the same accumulators.  At the end the accumulators go to the LDS once and one thread per pixel adds the
// tfactor entries of its bin (uint64), converts and stores.  Hits need no data: interior pixels (every row of every
// channel of the group present, decided from the same dmin / span table) hold channels x tfactor, the others add a
// clamp per channel.  Integer sums are exact in any order: the result equals the generic kernel's to the bit.
constexpr int kCutTT = 256, kCutRowB = 68, kCutNR = 8;
constexpr int kCutRowsCap = 900;           // rows of a tile the LDS holds (61 KB); the launch asks only for the largest tile it has
constexpr int kCutMaxChan = 16384;         // uint32 accumulators
constexpr size_t kCutRedBytes = (size_t)kCutNR * kCutTT * sizeof(uint32_t);

template <int BPV, int KIND>
__global__ void __launch_bounds__(kCutTT) frbch_post_cutout_lds(CutParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CT = 64 / BPV;
  const int tid = threadIdx.x;
  const int cand = blockIdx.z, g = blockIdx.y;
  const CutCand cd = p.cand[cand];
  const int f = cd.tfactor;
  const int bpt = f >= kCutTT ? 1 : kCutTT / f;                            // time bins of a workgroup
  const int j0 = (int)blockIdx.x * bpt;
  if (j0 >= p.nt) return;                                                  // (the grid is sized for the smallest bpt; whole workgroup)
  const int nbin = min(bpt, p.nt - j0);
  const int rows_wg = nbin * f;                                            // <= 256 unless bpt = 1
  const int nrow = KIND ? p.ndm : p.nf;
  const int r0 = g * kCutNR;
  const int nd = min(kCutNR, nrow - r0);
  const int c_lo = KIND ? 0 : r0 * p.cpb, c_hi = KIND ? p.nchan : (r0 + nd) * p.cpb;
  const size_t row_stride = (size_t)p.nifs * p.nchan * BPV;                // bytes between rows of the file
  const unsigned char* src0 = p.rows + (size_t)p.prod * p.nchan * BPV;
  const int32_t* rng = p.tile_range + ((size_t)cand * p.ngrp + g) * p.nct * 2;
  const int32_t* dly = KIND ? p.dt_delays + ((size_t)cand * p.ndm + r0) * p.nchan : p.ft_delays + (size_t)cand * p.nchan;
  const long long tb = cd.t0 + (long long)j0 * f;                          // first row of the workgroup at the top of the band
  const long long nrows = (long long)p.nrows;
  uint32_t a[kCutNR];
#pragma unroll
  for (int d = 0; d < kCutNR; ++d) a[d] = 0u;
  int glo = INT32_MAX, ghi = INT32_MIN;                                    // delays of the whole group: for the hits
  const int ct0 = c_lo / CT, ct1 = (c_hi - 1) / CT;
  for (int chunk = 0; chunk * kCutTT < rows_wg; ++chunk) {
    const int nr = min(kCutTT, rows_wg - chunk * kCutTT);                  // rows of this chunk, one per thread
    for (int ctile = ct0; ctile <= ct1; ++ctile) {
      const int32_t dmin = rng[ctile * 2], span = rng[ctile * 2 + 1];
      if (span < 0) continue;
      glo = min(glo, dmin);
      ghi = max(ghi, dmin + span);
      const int rows = nr + span;                                          // <= kCutRowsCap (the host checked)
      const long long first = tb + (long long)chunk * kCutTT + dmin;
      __syncthreads();                                                     // the previous tile is consumed
      for (int i = tid; i < rows * 4; i += kCutTT) {                       // 16-byte pieces: 4 per row
        const int r = i >> 2, part = i & 3;
        const long long s = first + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (s >= 0 && s < nrows) v = *reinterpret_cast<const uint4*>(src0 + (size_t)s * row_stride + (size_t)ctile * 64 + part * 16);
        *reinterpret_cast<uint32_t*>(smem + r * kCutRowB + part * 16) = v.x;
        *reinterpret_cast<uint32_t*>(smem + r * kCutRowB + part * 16 + 4) = v.y;
        *reinterpret_cast<uint32_t*>(smem + r * kCutRowB + part * 16 + 8) = v.z;
        *reinterpret_cast<uint32_t*>(smem + r * kCutRowB + part * 16 + 12) = v.w;
      }
      __syncthreads();
      if (tid < nr) {
        const int cb = max(c_lo, ctile * CT), ce = min(c_hi, (ctile + 1) * CT);
        if (KIND) {
          for (int c = cb; c < ce; ++c) {
#pragma unroll
            for (int d = 0; d < kCutNR; ++d)
              if (d < nd) {
                const unsigned char* q = smem + ((tid + (dly[(size_t)d * p.nchan + c] - dmin)) * kCutRowB + (c * BPV - ctile * 64));
                a[d] += BPV == 1 ? (uint32_t)*q : (uint32_t)*reinterpret_cast<const uint16_t*>(q);
              }
          }
        } else {
          int dd = cb / p.cpb - r0, rem = cb % p.cpb;                      // plane row of channel c, and c's place in its bin
          for (int c = cb; c < ce; ++c) {
            const unsigned char* q = smem + ((tid + (dly[c] - dmin)) * kCutRowB + (c * BPV - ctile * 64));
            const uint32_t v = BPV == 1 ? (uint32_t)*q : (uint32_t)*reinterpret_cast<const uint16_t*>(q);
#pragma unroll
            for (int d = 0; d < kCutNR; ++d) a[d] += d == dd ? v : 0u;
            if (++rem == p.cpb) { rem = 0; ++dd; }
          }
        }
      }
    }
  }
  __syncthreads();                                                         // the last tile is consumed
  uint32_t* red = reinterpret_cast<uint32_t*>(smem);                       // [kCutNR][256]
#pragma unroll
  for (int d = 0; d < kCutNR; ++d) red[d * kCutTT + tid] = a[d];
  __syncthreads();
  const int per = min(f, kCutTT);                                          // entries of a bin (a bin of more rows folded them)
  const int nch = KIND ? p.nchan : p.cpb;
  for (int i = tid; i < nd * nbin; i += kCutTT) {
    const int d = i / nbin, jb = i - d * nbin;
    unsigned long long s = 0;
    for (int k = 0; k < per; ++k) s += red[d * kCutTT + jb * per + k];
    const long long t = tb + (long long)jb * f;
    uint32_t n;
    if (t + glo >= 0 && t + (f - 1) + ghi < nrows) {
      n = (uint32_t)nch * (uint32_t)f;
    } else {
      n = 0;
      const int32_t* dl = KIND ? dly + (size_t)d * p.nchan : dly + (size_t)(r0 + d) * p.cpb;
      for (int c = 0; c < nch; ++c) {
        const long long lo = max(t + dl[c], 0ll), hi = min(t + dl[c] + f, nrows);
        if (hi > lo) n += (uint32_t)(hi - lo);
      }
    }
    const size_t o = ((size_t)cand * nrow + r0 + d) * p.nt + j0 + jb;
    p.out[o] = (float)(double)s;
    p.hits[o] = n;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Block statistics for the interference mask (HIP only; frbch_post_rfi_stats of kernels_post.inc stays the emulable form,
// the fallback and the kernel of float rows).  The anchor reads one sample per lane per row with lanes a channel apart --
// the access pattern that made the per-sample dedispersion slow.  Here a workgroup of 256 threads owns one block of rows
// and one tile of `tile_bytes` of the row (the host takes the largest of 1024 .. 64 that divides the row piece).  The
// tile_bytes / 16 lanes of a row piece sit side by side and take 16 bytes each (16 / 8 channels of 8- / 16-bit samples),
// coalesced across the tile; the 256 / that many lane groups take interleaved rows (group g: rows g, g + G, ...), with
// kRfiUnroll 16-byte non-temporal loads in flight per lane.  Sums stay in registers: uint32 for S, and for Q at 8 bit,
// over runs of kRfiRun rows per lane (4096 x 65025 and 4096 x 65535 < 2^32); Q at 16 bit is uint64 throughout.  After
// every run the partials of the G lane groups go through the LDS once (word k L + l of group g: consecutive lanes on
// consecutive banks, both ways) and ONE thread per channel adds them up in uint64 and stores -- or, for a block of more
// than G kRfiRun rows, adds to what it stored itself a run earlier: every (block, channel) is written by exactly one
// thread, there are no global atomics.  Integer sums are exact in any order: the result equals the anchor's to the bit.
constexpr int kRfiThreads = 256, kRfiUnroll = 4, kRfiRun = 4096;

template <int BPV>
__global__ void __launch_bounds__(kRfiThreads) frbch_post_rfi_stats_fast(RfiParams p) {
  constexpr int VPL = 16 / BPV;                                           // values per lane (one 16-byte piece)
  constexpr int NRED = kRfiThreads * VPL;                                 // partial sums of a workgroup
  __shared__ uint32_t red_s[NRED];
  __shared__ unsigned long long red_q[BPV == 1 ? NRED / 2 : NRED];       // 8 bit: NRED uint32
  const int tid = threadIdx.x;
  const int L = p.tile_bytes / 16, G = kRfiThreads / L, nch = p.tile_bytes / BPV;
  const int l = tid & (L - 1), g = tid / L;
  const int tile = blockIdx.x;
  const uint64_t b = (uint64_t)p.blk0 + blockIdx.y;
  const uint64_t r0 = b * p.block_rows;
  const uint64_t r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;
  const size_t stride = (size_t)p.nifs * p.nchan * BPV;                   // bytes between rows of the file
  const unsigned char* src = p.rows + (size_t)p.prod * p.nchan * BPV + (size_t)tile * p.tile_bytes + (size_t)l * 16;
  unsigned long long* dst = p.stats_i + ((size_t)b * p.nchan + (size_t)tile * nch) * 2;
  const uint64_t span = (uint64_t)G * kRfiRun;
  for (uint64_t s0 = r0; s0 < r1; s0 += span) {
    const uint64_t s1 = s0 + span < r1 ? s0 + span : r1;
    uint32_t as[VPL];
    uint32_t aq8[BPV == 1 ? VPL : 1];
    unsigned long long aq16[BPV == 2 ? VPL : 1];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      as[k] = 0u;
      if constexpr (BPV == 1) aq8[k] = 0u; else aq16[k] = 0ull;
    }
    for (uint64_t t = s0 + (uint64_t)g; t < s1; t += (uint64_t)G * kRfiUnroll) {
      uint32_t w[kRfiUnroll][4];
#pragma unroll
      for (int u = 0; u < kRfiUnroll; ++u) {
        const uint64_t tu = t + (uint64_t)u * G;
        if (tu < s1) {
          const frbch_nf4 v = __builtin_nontemporal_load(reinterpret_cast<const frbch_nf4*>(src + tu * stride));
          w[u][0] = __float_as_uint(v.x); w[u][1] = __float_as_uint(v.y); w[u][2] = __float_as_uint(v.z); w[u][3] = __float_as_uint(v.w);
        } else {
          w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0u;                     // adds nothing
        }
      }
#pragma unroll
      for (int u = 0; u < kRfiUnroll; ++u)
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          if constexpr (BPV == 1) {
            const uint32_t x = (w[u][k >> 2] >> (8 * (k & 3))) & 0xFFu;
            as[k] += x;
            aq8[k] += x * x;
          } else {
            const uint32_t x = (w[u][k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            as[k] += x;
            aq16[k] += (unsigned long long)(x * x);
          }
        }
    }
    __syncthreads();                                                      // the previous run's partials are consumed
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int i = g * nch + k * L + l;
      red_s[i] = as[k];
      if constexpr (BPV == 1) reinterpret_cast<uint32_t*>(red_q)[i] = aq8[k]; else red_q[i] = aq16[k];
    }
    __syncthreads();
    for (int pos = tid; pos < nch; pos += kRfiThreads) {                  // word pos = k L + l holds channel l VPL + k
      unsigned long long S = 0, Q = 0;
      for (int gg = 0; gg < G; ++gg) {
        S += red_s[gg * nch + pos];
        if constexpr (BPV == 1) Q += reinterpret_cast<const uint32_t*>(red_q)[gg * nch + pos]; else Q += red_q[gg * nch + pos];
      }
      const int ch = (pos & (L - 1)) * VPL + pos / L;
      if (s0 != r0) {
        S += dst[(size_t)ch * 2];
        Q += dst[(size_t)ch * 2 + 1];
      }
      dst[(size_t)ch * 2] = S;
      dst[(size_t)ch * 2 + 1] = Q;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Periodicity: the spectral peak of every (block, channel) cell (HIP only; frbch_post_rfi_peaks of kernels_post.inc stays the
// emulable form, the fallback and the kernel of float rows; both call rfi_bfly and rfi_bins, so they differ in schedule only).
// A workgroup of 256 threads owns one block of n = 2^L rows and a piece of pk_piece(L) bytes of the row (64 bytes up to
// n = 512, 32 at 1024, 16 at 2048: the raw columns take at most 40 KB of the LDS, so that two workgroups share a CU).
//  1. The piece of every row goes to the LDS as raw bytes: the piece / 16 lanes of a row side by side with 16 bytes each,
//     coalesced across the tile, four loads in flight per lane; rows padded by one word against bank conflicts.
//  2. pk_np(L) channel pairs at a time are transformed side by side in a second LDS buffer (NP n = 4096 complex values; one
//     pair at n = 2048).  The transform is two or three register passes of radix 16 or 8 (R0 + R1 + R2 = L stages), each a
//     network of the radix-2 butterflies of include/frbch.h on 2^R values a thread holds: the first pass converts the raw
//     samples (minus the cell's mean, in double) straight from the bit-reversed rows it needs, the others exchange through
//     the buffer, whose index i sits at i + i / 16 (a stride of 16 complex values would otherwise stay on two banks).
//  3. 256 / NP threads per pair walk the bins in ascending k; a shuffle reduction per wave segment and ONE thread per
//     (pair, channel) keep the largest value, the lowest k among equals, and store the cell: no global atomics.
constexpr int kPkThreads = 256;
constexpr int pk_np(int L) { return L >= 11 ? 1 : 4096 >> L; }
constexpr int pk_piece(int L) { return (32768 >> L) > 64 ? 64 : (32768 >> L); }
constexpr int pk_pad(int i) { return i + (i >> 4); }
constexpr size_t kPkHead = 1280;           // means (64 doubles), tested flags (64 words), partial peaks (32)
constexpr size_t pk_lds(int L) {
  return kPkHead + (size_t)(4 << L) + (size_t)pk_np(L) * pk_pad(1 << L) * 8 + ((size_t)4 << L) * (pk_piece(L) / 4 + 1);
}
constexpr int pk_brev(int m, int bits) {
  int r = 0;
  for (int q = 0; q < bits; ++q) r |= ((m >> q) & 1) << (bits - 1 - q);
  return r;
}

// stages S0 + 1 .. S0 + R on the 2^R values of index lo + (m << S0) + (hi << (S0 + R)), m = 0 .. 2^R - 1
template <int L, int S0, int R>
__device__ __forceinline__ void pk_pass(float (&vr)[1 << R], float (&vi)[1 << R], int lo, const float2* tw) {
#pragma unroll
  for (int q = 1; q <= R; ++q) {
    const int hq = 1 << (q - 1);
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) {
      if (m & hq) continue;
      const int j = lo + ((m & (hq - 1)) << S0);
      const float2 w = tw[j << (L - S0 - q)];
      rfi_bfly(vr[m], vi[m], vr[m + hq], vi[m + hq], w.x, w.y);
    }
  }
}

// a pass that exchanges through the buffer: every value is read and written by the one thread that owns it in this pass
template <int L, int S0, int R, int NP>
__device__ __forceinline__ void pk_pass_lds(float2* buf, const float2* tw, int tid) {
  constexpr int N = 1 << L, NPAD = pk_pad(N), G = N >> R;
  for (int w = tid; w < NP * G; w += kPkThreads) {
    const int q = w / G, g = w & (G - 1);
    const int lo = g & ((1 << S0) - 1), hi = g >> S0;
    float2* z = buf + q * NPAD;
    const int at = lo + (hi << (S0 + R));
    float vr[1 << R], vi[1 << R];
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) {
      const float2 v = z[pk_pad(at + (m << S0))];
      vr[m] = v.x; vi[m] = v.y;
    }
    pk_pass<L, S0, R>(vr, vi, lo, tw);
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) z[pk_pad(at + (m << S0))] = make_float2(vr[m], vi[m]);
  }
}

template <int L, int BPV, int R0, int R1, int R2>
__global__ void __launch_bounds__(kPkThreads) frbch_post_rfi_peaks_fast(RfiParams p) {
  constexpr int N = 1 << L, NP = pk_np(L), PB = pk_piece(L), CH = PB / BPV, PAIRS = CH / 2, RS = PB / 4 + 1, LANES = PB / 16;
  constexpr int NPAD = pk_pad(N), G0 = N >> R0;
  constexpr int TPP = kPkThreads / NP, W = TPP < 64 ? TPP : 64, PARTS = TPP / W;
  static_assert(R0 + R1 + R2 == L && R0 >= 1 && R1 >= 1 && PAIRS % NP == 0 && CH <= 64 && NP * PARTS * 2 <= 32, "plan");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* mean = reinterpret_cast<double*>(smem);
  uint32_t* tested = reinterpret_cast<uint32_t*>(smem + 512);
  RfiPeak* red = reinterpret_cast<RfiPeak*>(smem + 768);
  float2* tw = reinterpret_cast<float2*>(smem + kPkHead);
  float2* buf = tw + N / 2;
  uint32_t* raw = reinterpret_cast<uint32_t*>(buf + NP * NPAD);
  const int tid = threadIdx.x;
  const int ch0 = (int)blockIdx.x * CH;                                   // first channel of the piece
  const uint64_t b = (uint64_t)p.blk0 + blockIdx.y;
  const uint64_t r0 = b * p.block_rows;
  const uint64_t r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;
  const int nbr = (int)(r1 - r0);
  RfiPeak* out = p.peaks + (size_t)b * p.nchan + ch0;
  if (2 * nbr < N) {                                                      // the whole block is not tested (the same in every thread)
    if (tid < CH) { RfiPeak z; z.num = 0.f; z.k = 0u; out[tid] = z; }
    return;
  }
  for (int i = tid; i < N / 2; i += kPkThreads) tw[i] = reinterpret_cast<const float2*>(p.tw)[i];
  if (tid < CH) {
    double m = 0.0;
    tested[tid] = rfi_cell_mean(p, b, ch0 + tid, (double)nbr, &m) ? 1u : 0u;
    mean[tid] = m;
  }
  {
    const size_t stride = (size_t)p.nifs * p.nchan * BPV;                 // bytes between rows of the file
    const unsigned char* src = p.rows + (size_t)p.prod * p.nchan * BPV + (size_t)blockIdx.x * PB + r0 * stride;
    const int total = nbr * LANES;
    for (int i0 = tid; i0 < total; i0 += kPkThreads * 4) {
      frbch_nf4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * kPkThreads;
        if (i < total) v[u] = __builtin_nontemporal_load(reinterpret_cast<const frbch_nf4*>(src + (size_t)(i / LANES) * stride + (size_t)(i % LANES) * 16));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * kPkThreads;
        if (i < total) {
          uint32_t* d = raw + (i / LANES) * RS + (i % LANES) * 4;
          d[0] = __float_as_uint(v[u].x); d[1] = __float_as_uint(v[u].y); d[2] = __float_as_uint(v[u].z); d[3] = __float_as_uint(v[u].w);
        }
      }
    }
  }
  __syncthreads();
  for (int rd = 0; rd < PAIRS / NP; ++rd) {
    for (int w = tid; w < NP * G0; w += kPkThreads) {                     // pass 0: from the raw rows
      const int q = w / G0, base = w & (G0 - 1);
      const int pq = rd * NP + q;                                         // pair of the piece: channels 2 pq, 2 pq + 1
      const double m0 = mean[2 * pq], m1 = mean[2 * pq + 1];
      const bool t0 = tested[2 * pq] != 0u, t1 = tested[2 * pq + 1] != 0u;
      const int jlo = (int)(__brev((unsigned)base) >> (32 - (L - R0)));
      float vr[1 << R0], vi[1 << R0];
#pragma unroll
      for (int m = 0; m < (1 << R0); ++m) {
        const int j = (pk_brev(m, R0) << (L - R0)) + jlo;
        float x0 = 0.f, x1 = 0.f;
        if (j < nbr) {
          uint32_t a, c;
          if constexpr (BPV == 1) {
            const uint32_t word = raw[j * RS + (pq >> 1)] >> (16 * (pq & 1));
            a = word & 0xFFu; c = (word >> 8) & 0xFFu;
          } else {
            const uint32_t word = raw[j * RS + pq];
            a = word & 0xFFFFu; c = word >> 16;
          }
          if (t0) x0 = (float)((double)a - m0);
          if (t1) x1 = (float)((double)c - m1);
        }
        vr[m] = x0; vi[m] = x1;
      }
      pk_pass<L, 0, R0>(vr, vi, 0, tw);
      float2* z = buf + q * NPAD;
#pragma unroll
      for (int m = 0; m < (1 << R0); ++m) z[pk_pad((base << R0) + m)] = make_float2(vr[m], vi[m]);
    }
    __syncthreads();
    pk_pass_lds<L, R0, R1, NP>(buf, tw, tid);
    __syncthreads();
    if constexpr (R2 > 0) {
      pk_pass_lds<L, R0 + R1, R2, NP>(buf, tw, tid);
      __syncthreads();
    }
    {
      const int q = tid / TPP, t = tid & (TPP - 1);
      const float2* z = buf + q * NPAD;
      float num0 = 0.f, num1 = 0.f;
      uint32_t k0 = 0u, k1 = 0u;
      for (int k = 1 + t; k < N / 2; k += TPP) {
        const float2 A = z[pk_pad(k)], B = z[pk_pad(N - k)];
        float n0, n1;
        rfi_bins(A.x, A.y, B.x, B.y, &n0, &n1);
        if (n0 > num0) { num0 = n0; k0 = (uint32_t)k; }
        if (n1 > num1) { num1 = n1; k1 = (uint32_t)k; }
      }
#pragma unroll
      for (int off = W / 2; off >= 1; off >>= 1) {                        // within an aligned segment of W lanes
        const float on0 = __shfl_xor(num0, off), on1 = __shfl_xor(num1, off);
        const uint32_t ok0 = (uint32_t)__shfl_xor((int)k0, off), ok1 = (uint32_t)__shfl_xor((int)k1, off);
        if (on0 > num0 || (on0 == num0 && ok0 < k0)) { num0 = on0; k0 = ok0; }
        if (on1 > num1 || (on1 == num1 && ok1 < k1)) { num1 = on1; k1 = ok1; }
      }
      if ((t & (W - 1)) == 0) {
        RfiPeak* d = red + (q * PARTS + t / W) * 2;
        d[0].num = num0; d[0].k = k0;
        d[1].num = num1; d[1].k = k1;
      }
    }
    __syncthreads();                                                      // (also: every read of buf is behind us)
    if (tid < NP * 2) {
      const int q = tid >> 1, ch = tid & 1;
      RfiPeak best = red[(q * PARTS) * 2 + ch];
#pragma unroll
      for (int part = 1; part < PARTS; ++part) {
        const RfiPeak o = red[(q * PARTS + part) * 2 + ch];
        if (o.num > best.num || (o.num == best.num && o.k < best.k)) best = o;
      }
      out[2 * (rd * NP + q) + ch] = best;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Periodicity search: the transform of n = 2^L points, L = 12 .. 22, in one, two or three LDS-resident passes (HIP only; the
// stage-by-stage kernels of kernels_post.inc stay the emulable form and the fallback; both call rfi_bfly with the same table
// entries, so they differ in schedule only).  A pass owns R consecutive stages of the radix-2 graph and a tile of 2^R points
// times C columns (at most 8192 complex values, 68 KB with the padding: two workgroups share a CU):
//   first pass   stages 1 .. R on runs of 2^R consecutive points of the bit-reversed order.  Run r gathers the samples
//                t = m' 2^(L-R) + bitrev(r): a workgroup takes the C = 16 runs whose bitrev(r) are consecutive, so that every
//                global read is 16 consecutive floats of a series (one 64-byte piece), and stores 16 whole runs.  The mean
//                goes off in double on the way in.  With one pass (L <= 13) the tile is the transform: C = 1, reads contiguous.
//   later passes stages s0 + 1 .. s0 + R on the sets i = hi 2^(s0+R) + m 2^s0 + lo: a workgroup takes 16 consecutive lo, so
//                that every global access is 16 consecutive complex values (128 bytes), and works in place.
// Inside a pass the stages run as register passes of radix 8 or 4 (RR = 3 or 2 stages on 2^RR values a thread holds), as in
// the 256 .. 2048-point kernel above; LDS index i sits at i + i / 16.  Twiddles come from the table in global memory (the
// later passes need a different entry for every column: they do not fit the LDS beside the tile, and the L2 holds them).
constexpr int kPsThreads = 256;
constexpr int kPsTileLog = 13;                      // a tile holds at most 2^13 complex values
__device__ __forceinline__ int ps_pad(int i) { return i + (i >> 4); }
constexpr size_t ps_lds_bytes(int log_points) { return (size_t)((1 << log_points) + (1 << (log_points - 4))) * 8; }

// stages s0 + q0 + 1 .. s0 + q0 + RR of a tile whose point (m, c) sits at ps_pad(m C + c); a thread holds the 2^RR values
// m = mlo + (x << q0) + (mhi << (q0 + RR)).  The low s0 bits of a point's index are lo0 + c (s0 = 0: there are none, the
// columns are runs of their own).
template <int RR>
__device__ __forceinline__ void ps_subpass(float2* buf, const float2* __restrict__ tw, int tid, int logc, int R, int q0, int s0,
                                           int L, int lo0) {
  const int items = (1 << (logc + R)) >> RR;
  for (int w = tid; w < items; w += kPsThreads) {
    const int c = w & ((1 << logc) - 1), g = w >> logc;
    const int mlo = g & ((1 << q0) - 1), mhi = g >> q0;
    const int m0 = mlo + (mhi << (q0 + RR));
    const int lo = s0 ? lo0 + c : 0;
    float vr[1 << RR], vi[1 << RR];
#pragma unroll
    for (int x = 0; x < (1 << RR); ++x) {
      const float2 v = buf[ps_pad(((m0 + (x << q0)) << logc) + c)];
      vr[x] = v.x; vi[x] = v.y;
    }
#pragma unroll
    for (int q = 1; q <= RR; ++q) {
      const int hq = 1 << (q - 1);
      const int sh = L - (s0 + q0 + q);
#pragma unroll
      for (int x = 0; x < (1 << RR); ++x) {
        if (x & hq) continue;
        const int j = ((mlo + ((x & (hq - 1)) << q0)) << s0) + lo;
        const float2 t = tw[(size_t)j << sh];
        rfi_bfly(vr[x], vi[x], vr[x + hq], vi[x + hq], t.x, t.y);
      }
    }
#pragma unroll
    for (int x = 0; x < (1 << RR); ++x) buf[ps_pad(((m0 + (x << q0)) << logc) + c)] = make_float2(vr[x], vi[x]);
  }
}

// the R stages of a pass: register passes of 3, 3, ... stages, the last ones 2 where 3 do not divide R; a barrier behind each
__device__ __forceinline__ void ps_stages(float2* buf, const float2* tw, int tid, int logc, int R, int s0, int L, int lo0) {
  int q0 = 0;
  while (q0 < R) {
    const int left = R - q0, chunks = (left + 2) / 3, rr = (left + chunks - 1) / chunks;
    if (rr == 3) ps_subpass<3>(buf, tw, tid, logc, R, q0, s0, L, lo0);
    else if (rr == 2) ps_subpass<2>(buf, tw, tid, logc, R, q0, s0, L, lo0);
    else ps_subpass<1>(buf, tw, tid, logc, R, q0, s0, L, lo0);
    __syncthreads();
    q0 += rr;
  }
}

// grid (2^(L - R - logc), npair), dynamic LDS ps_lds_bytes(R + logc)
__global__ void __launch_bounds__(kPsThreads) frbch_post_ps_fft_first(PsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* buf = reinterpret_cast<float2*>(smem);
  const float2* tw = reinterpret_cast<const float2*>(p.tw);
  const int tid = threadIdx.x, L = p.log2n, R = p.rcur, logc = p.logc;
  const int pair = (int)blockIdx.y, d0 = 2 * pair, d1 = d0 + 1;
  const uint32_t c0 = (uint32_t)blockIdx.x << logc;
  const bool live0 = p.live[d0] != 0u, live1 = d1 < p.ndm && p.live[d1] != 0u;
  const double mean0 = live0 ? p.mean[d0] : 0.0, mean1 = live1 ? p.mean[d1] : 0.0;
  const float* x0 = p.series + (size_t)d0 * p.nout;
  const float* x1 = p.series + (size_t)(live1 ? d1 : d0) * p.nout;
  const int total = 1 << (R + logc);
  for (int e = tid; e < total; e += kPsThreads) {
    const int c = e & ((1 << logc) - 1), mm = e >> logc;
    const uint32_t t = ((uint32_t)mm << (L - R)) + c0 + (uint32_t)c;
    float a = 0.f, b = 0.f;
    if (live0) a = (float)((double)x0[t] - mean0);
    if (live1) b = (float)((double)x1[t] - mean1);
    const int m = (int)(__brev((unsigned)mm) >> (32 - R));
    buf[ps_pad((m << logc) + c)] = make_float2(a, b);
  }
  __syncthreads();
  ps_stages(buf, tw, tid, logc, R, 0, L, 0);
  float2* out = reinterpret_cast<float2*>(p.work) + (size_t)pair * p.n;
  for (int e = tid; e < total; e += kPsThreads) {
    const int m = e & ((1 << R) - 1), c = e >> R;
    const uint32_t hi = L > R ? __brev(c0 + (uint32_t)c) >> (32 - (L - R)) : 0u;
    out[((size_t)hi << R) + m] = buf[ps_pad((m << logc) + c)];
  }
}

// grid (2^(L - R - 4), npair), dynamic LDS ps_lds_bytes(R + 4): stages s0 + 1 .. s0 + R in place, 16 columns a tile (2^s0 >= 16)
__global__ void __launch_bounds__(kPsThreads) frbch_post_ps_fft_later(PsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* buf = reinterpret_cast<float2*>(smem);
  const float2* tw = reinterpret_cast<const float2*>(p.tw);
  const int tid = threadIdx.x, L = p.log2n, R = p.rcur, s0 = p.s0;
  const uint32_t tile = blockIdx.x, cols = 1u << (s0 - 4);
  const int lo0 = (int)((tile & (cols - 1)) << 4);
  const size_t hi = tile >> (s0 - 4);
  float2* z = reinterpret_cast<float2*>(p.work) + (size_t)blockIdx.y * p.n + (hi << (s0 + R)) + (size_t)lo0;
  const int total = 1 << (R + 4);
  for (int e = tid; e < total; e += kPsThreads) buf[ps_pad(e)] = z[((size_t)(e >> 4) << s0) + (e & 15)];
  __syncthreads();
  ps_stages(buf, tw, tid, 4, R, s0, L, lo0);
  for (int e = tid; e < total; e += kPsThreads) z[((size_t)(e >> 4) << s0) + (e & 15)] = buf[ps_pad(e)];
}

// The block levels and the normalisation from an LDS tile: a workgroup owns kPsNormTile / B consecutive blocks of one series
// (the last workgroup also the short or long last block), loads their powers once, coalesced; one thread per block adds its
// block in ascending k from the LDS (the order the rule fixes; block b's bins sit one word further on than block b - 1's, so
// that the threads of a wave read 64 banks); then all threads divide and store, coalesced.  grid (ceil(nblk / G), ndm).
constexpr int kPsNormTile = 8192;
constexpr int kPsNormLds = kPsNormTile + 1024 + (kPsNormTile + 1024) / 32;      // tile, the longest last block, a word a block
__global__ void __launch_bounds__(kPsThreads) frbch_post_ps_norm_lds(PsParams p) {
  __shared__ float tile[kPsNormLds];
  __shared__ double level[kPsNormTile / 32];
  const int tid = threadIdx.x, logb = p.logb;
  const uint32_t B = p.wblock, G = (uint32_t)kPsNormTile >> logb, nh = p.n / 2;
  const uint32_t b0 = blockIdx.x * G, b1 = b0 + G < p.nblk ? b0 + G : p.nblk;
  const uint32_t k0 = 1u + b0 * B, k1 = b1 == p.nblk ? nh : 1u + b1 * B;
  const int cnt = (int)(k1 - k0), nb = (int)(b1 - b0);
  float* x = p.pw + (size_t)blockIdx.y * nh + k0;
  for (int i = tid; i < cnt; i += kPsThreads) tile[i + (i >> logb)] = x[i];
  __syncthreads();
  if (tid < nb) {
    POST_NO_CONTRACT
    const int s0 = tid << logb, s1 = tid + 1 == nb ? cnt : s0 + (int)B;
    double S = 0.0;
    float mx = 0.f;
    for (int i = s0; i < s1; ++i) {
      const float v = tile[i + (i >> logb)];
      S = S + (double)v;
      if (v > mx) mx = v;
    }
    const double num = S - (double)mx;
    const double m = num / (double)(s1 - s0 - 1);
    level[tid] = rfi_finite(m) && m > 0.0 ? m : 0.0;
  }
  __syncthreads();
  for (int i = tid; i < cnt; i += kPsThreads) {
    POST_NO_CONTRACT
    int b = i >> logb;
    if (b >= nb) b = nb - 1;
    const double m = level[b];
    float q = 0.f;
    if (m > 0.0 && k0 + (uint32_t)i >= p.kmin) { const double r = (double)tile[i + (i >> logb)] / m; q = (float)r; }
    x[i] = q;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Resampling for the acceleration search, fast form (HIP only; frbch_post_resample of kernels_post.inc is the emulable form
// and the fallback, and both evaluate res_index: the same bytes).  A workgroup owns kResTile consecutive outputs of one row
// of one trial, four a thread.  u(t) never steps back and never by more than 2, so the inputs of the tile are the contiguous
// window [u(first), u(last)] of at most 2 kResTile - 1 samples: it is staged through the LDS with 16-byte loads (from the
// 16-byte boundary at or below its start; rows are 16-byte aligned, so the last load ends inside the row), the threads pick
// their four values from the LDS and store them with one 16-byte store.  The index rule is evaluated once per output: the
// first and the last thread leave their outer indices in the LDS for the others.  grid (n / kResTile, trials * rows_per_trial).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kResThreads = 256, kResTile = 4 * kResThreads;
constexpr int kResWin = 2 * kResTile + 8;           // floats: the window, and the up to 3 + 3 samples of the alignment
__global__ void __launch_bounds__(kResThreads) frbch_post_resample_lds(ResParams p) {
  __shared__ __attribute__((aligned(16))) float win[kResWin];
  __shared__ uint32_t ends[2];
  const int tid = threadIdx.x, row = (int)blockIdx.y;
  const int trial = row / p.rows_per_trial, dm = row - trial * p.rows_per_trial;
  const uint32_t t0 = blockIdx.x * (uint32_t)kResTile + 4u * (uint32_t)tid;
  float4* dst = (float4*)(p.out + (size_t)row * p.n + t0);
  if (dm >= p.ndm) {                                // the zero partner of an odd last series (the whole workgroup)
    *dst = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const double q = p.q[trial];
  uint32_t u[4];
  for (int j = 0; j < 4; ++j) u[j] = res_index(q, t0 + (uint32_t)j, p.n);
  if (tid == 0) ends[0] = u[0];
  if (tid == kResThreads - 1) ends[1] = u[3];
  __syncthreads();
  const uint32_t lo = ends[0] & ~3u, hi = ends[1];
  uint32_t nvec = hi >= lo ? ((hi - lo) >> 2) + 1u : 0u;
  if (nvec > (uint32_t)(kResWin / 4)) nvec = (uint32_t)(kResWin / 4);      // (never: the window bound above)
  const float4* src = (const float4*)(p.series + (size_t)dm * p.nout + lo);
  for (uint32_t i = (uint32_t)tid; i < nvec; i += (uint32_t)kResThreads) ((float4*)win)[i] = src[i];
  __syncthreads();
  float v[4];
  for (int j = 0; j < 4; ++j) {
    uint32_t i = u[j] - lo;
    if (i > (uint32_t)(kResWin - 1)) i = (uint32_t)(kResWin - 1);          // (never, for the same reason)
    v[j] = win[i];
  }
  *dst = make_float4(v[0], v[1], v[2], v[3]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Burst sums (HIP only; frbch_post_burst_sums of kernels_post.inc stays the emulable form, the fallback and the kernel of
// float rows).  A workgroup of 256 threads owns one candidate and one 64-byte tile of the row: 4 lanes side by side take the
// 16-byte pieces of a row (16 / 8 channels of 8- / 16-bit samples) of ALL nifs products in one trip, the 64 lane groups
// take interleaved rows (group g: rows g, g + 64, ...), so the rows of a window are split across the four waves.  The
// delays differ per channel: for a window [w0, w0 + len) the workgroup walks the rows w0 + dmin .. w0 + len - 1 + dmax of
// its tile (dmin / dmax over the tile's channels, clipped to the file) and a channel takes a row iff the row minus its own
// delay falls into the window -- one subtraction and one unsigned compare.  Partials are uint32 over runs of kBsRun rows
// per lane (16 lanes x 256 rows x 65535 < 2^32; the squares of 16-bit samples are uint64 throughout); after every run the
// 16 lanes of a wave that share a piece add theirs up by shuffles and one lane per piece adds the 64-bit result to the
// workgroup's totals in the LDS.  At the end ONE thread per (product, channel) computes the hits -- they need no data -- and
// stores the record: no global atomics.  Integer sums are exact in any order: the result equals the generic kernel's.
// All row arithmetic is 64 bit.  grid (row bytes / 64, ncand).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kBsThreads = 256, kBsGroups = 64, kBsRun = 256, kBsMaxIfs = 4;

template <class T> __device__ __forceinline__ T bs_wave_sum(T v) {       // over the 16 lanes of a wave with equal lane & 3
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

template <int BPV>
__global__ void __launch_bounds__(kBsThreads) frbch_post_burst_sums_fast(BurstParams p) {
  constexpr int VPL = 16 / BPV, CT = 64 / BPV;
  __shared__ unsigned long long tot[3][kBsMaxIfs][CT];                     // on_sum, off_sum, off_sumsq
  const int tid = threadIdx.x, l = tid & 3, g = tid >> 2;
  const int tile = blockIdx.x, cand = blockIdx.y;
  for (int i = tid; i < 3 * kBsMaxIfs * CT; i += kBsThreads) (&tot[0][0][0])[i] = 0ull;
  const BurstCand cd = p.cand[cand];
  const int32_t* dly = p.delays + (size_t)cand * p.nchan + (size_t)tile * CT + (size_t)l * VPL;
  int dk[VPL];
  int dmin = INT32_MAX, dmax = 0;
#pragma unroll
  for (int k = 0; k < VPL; ++k) {
    dk[k] = dly[k];
    dmin = min(dmin, dk[k]);
    dmax = max(dmax, dk[k]);
  }
  dmin = min(dmin, __shfl_xor(dmin, 1)); dmin = min(dmin, __shfl_xor(dmin, 2));      // over the four pieces of the tile:
  dmax = max(dmax, __shfl_xor(dmax, 1)); dmax = max(dmax, __shfl_xor(dmax, 2));      // the same in every thread
#pragma unroll
  for (int k = 0; k < VPL; ++k) dk[k] -= dmin;
  const size_t stride = (size_t)p.nifs * p.nchan * BPV, pstride = (size_t)p.nchan * BPV;
  const unsigned char* src = p.rows + (size_t)tile * 64 + (size_t)l * 16;
  const long long nrows = (long long)p.nrows;
  __syncthreads();
  for (int w = 0; w < 3; ++w) {
    long long w0;
    uint32_t len;
    burst_window(cd, w, &w0, &len);
    const long long base = w0 + dmin;
    const long long first = base < 0 ? 0 : base;
    long long last = base + (long long)len - 1 + (long long)(dmax - dmin);
    if (last > nrows - 1) last = nrows - 1;
    const int qa = w == 1 ? 0 : 1;
    for (long long ch0 = first; ch0 <= last; ch0 += (long long)kBsGroups * kBsRun) {
      long long ce = ch0 + (long long)kBsGroups * kBsRun - 1;
      if (ce > last) ce = last;
      uint32_t s[kBsMaxIfs][VPL];
      uint32_t q8[kBsMaxIfs][BPV == 1 ? VPL : 1];
      unsigned long long q16[kBsMaxIfs][BPV == 2 ? VPL : 1];
#pragma unroll
      for (int pr = 0; pr < kBsMaxIfs; ++pr)
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          s[pr][k] = 0u;
          if constexpr (BPV == 1) q8[pr][k] = 0u; else q16[pr][k] = 0ull;
        }
      for (long long r = ch0 + g; r <= ce; r += kBsGroups) {
        const int rr = (int)(r - base);
        uint32_t wv[kBsMaxIfs][4];
#pragma unroll
        for (int pr = 0; pr < kBsMaxIfs; ++pr)
          if (pr < p.nifs) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)r * stride + (size_t)pr * pstride);
            wv[pr][0] = v.x; wv[pr][1] = v.y; wv[pr][2] = v.z; wv[pr][3] = v.w;
          }
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
          const bool in = (uint32_t)(rr - dk[k]) < len;
#pragma unroll
          for (int pr = 0; pr < kBsMaxIfs; ++pr)
            if (pr < p.nifs) {
              if constexpr (BPV == 1) {
                const uint32_t x = in ? (wv[pr][k >> 2] >> (8 * (k & 3))) & 0xFFu : 0u;
                s[pr][k] += x;
                q8[pr][k] += x * x;
              } else {
                const uint32_t x = in ? (wv[pr][k >> 1] >> (16 * (k & 1))) & 0xFFFFu : 0u;
                s[pr][k] += x;
                q16[pr][k] += (unsigned long long)(x * x);
              }
            }
        }
      }
      // (every thread of the workgroup makes the same trips through both outer loops: the shuffles meet whole waves)
#pragma unroll
      for (int pr = 0; pr < kBsMaxIfs; ++pr)
        if (pr < p.nifs) {
#pragma unroll
          for (int k = 0; k < VPL; ++k) {
            const unsigned long long ss = (unsigned long long)bs_wave_sum(s[pr][k]);
            unsigned long long qq;
            if constexpr (BPV == 1) qq = (unsigned long long)bs_wave_sum(q8[pr][k]); else qq = bs_wave_sum(q16[pr][k]);
            if ((tid & 63) < 4) {
              atomicAdd(&tot[qa][pr][l * VPL + k], ss);
              if (qa) atomicAdd(&tot[2][pr][l * VPL + k], qq);
            }
          }
        }
    }
  }
  __syncthreads();
  for (int i = tid; i < p.nifs * CT; i += kBsThreads) {
    const int pr = i / CT, ch = i - pr * CT, c = tile * CT + ch;
    const long long n = (long long)p.delays[(size_t)cand * p.nchan + c];
    uint32_t hits[2] = {0u, 0u};
    for (int w = 0; w < 3; ++w) {
      long long w0, lo, hi;
      uint32_t len;
      burst_window(cd, w, &w0, &len);
      burst_clip(w0, len, n, nrows, &lo, &hi);
      hits[w == 1 ? 0 : 1] += (uint32_t)(hi - lo);
    }
    BurstSums o;
    o.on_sum = (double)tot[0][pr][ch];
    o.off_sum = (double)tot[1][pr][ch];
    o.off_sumsq = (double)tot[2][pr][ch];
    o.on_hits = hits[0];
    o.off_hits = hits[1];
    p.sums[((size_t)cand * p.nifs + pr) * p.nchan + c] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// RM synthesis (HIP only; frbch_post_rm of kernels_post.inc stays the emulable form and the fallback; both call rm_term, so
// they differ in schedule only).  The 64 KiB table lies in the LDS once per workgroup; lanes run along k, kRmKpt trials
// 256 apart per thread, so that a record -- staged through the LDS in tiles of kRmTile, read at one address by the whole
// wave -- serves 1024 terms: one 64 x 32 bit product for the first phase, then an addition of 256 D per further trial, two
// table reads and four 32 x 32 + 64 bit multiply-adds per term.  blockIdx.y splits a candidate's records in pieces of
// `chunk`; with nsplit > 1 the int64 partials go to p.part and frbch_post_rm_join adds them up (exact in any order), with
// nsplit = 1 the kernel stores F itself.  grid (ceil(nphi / 1024), nsplit, ncand).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kRmThreads = 256, kRmKpt = 4, kRmTile = 256;
constexpr size_t kRmLds = 65536 + (size_t)kRmTile * sizeof(RmRec);

// rm_store's values as one 8-byte store (the host takes this kernel for an 8-byte aligned F only)
__device__ __forceinline__ void rm_store2(float* out, long long re, long long im, double inv) {
  POST_NO_CONTRACT
  float2 v;
  v.x = (float)((double)re * inv);
  v.y = (float)((double)im * inv);
  *reinterpret_cast<float2*>(out) = v;
}

__global__ void __launch_bounds__(kRmThreads) frbch_post_rm_fast(RmParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* tab = reinterpret_cast<int32_t*>(smem);
  RmRec* recs = reinterpret_cast<RmRec*>(smem + 65536);
  const int tid = threadIdx.x, cand = blockIdx.z, split = blockIdx.y;
  const int k0 = (int)blockIdx.x * (kRmThreads * kRmKpt) + tid;
  for (int i = tid; i < 4096; i += kRmThreads) reinterpret_cast<int4*>(tab)[i] = reinterpret_cast<const int4*>(p.table)[i];
  const RmCand cd = p.cand[cand];
  const int r0 = split * p.chunk;
  const int r1 = min(r0 + p.chunk, (int)cd.nrec);
  long long re[kRmKpt], im[kRmKpt];
#pragma unroll
  for (int j = 0; j < kRmKpt; ++j) re[j] = im[j] = 0;
  for (int t0 = r0; t0 < r1; t0 += kRmTile) {
    const int n = min(kRmTile, r1 - t0);
    __syncthreads();                                                       // the previous tile is consumed
    const uint32_t* srcw = reinterpret_cast<const uint32_t*>(p.rec + (size_t)cand * p.nchan + t0);
    for (int i = tid; i < n * 6; i += kRmThreads) reinterpret_cast<uint32_t*>(recs)[i] = srcw[i];
    __syncthreads();                                                       // (the first one covers the table as well)
    for (int r = 0; r < n; ++r) {
      const RmRec rc = recs[r];
      unsigned long long ph = rc.p0 + rc.d * (unsigned long long)(uint32_t)k0;
      const unsigned long long step = rc.d << 8;                           // kRmThreads D
#pragma unroll
      for (int j = 0; j < kRmKpt; ++j) {
        rm_term(tab, ph, rc.qi, rc.ui, &re[j], &im[j]);
        ph += step;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kRmKpt; ++j) {
    const int k = k0 + j * kRmThreads;
    if (k < p.nphi) {
      if (p.nsplit == 1) {
        rm_store2(p.out + ((size_t)cand * p.nphi + k) * 2, re[j], im[j], cd.inv);
      } else {
        long long* o = p.part + (((size_t)split * p.ncand + cand) * p.nphi + k) * 2;
        o[0] = re[j];
        o[1] = im[j];
      }
    }
  }
}

// grid (ceil(nphi / 256), ncand): the partials of the splits, added in ascending split
__global__ void __launch_bounds__(kRmThreads) frbch_post_rm_join(RmParams p) {
  const int k = (int)blockIdx.x * kRmThreads + (int)threadIdx.x, cand = blockIdx.y;
  if (k >= p.nphi) return;
  long long re = 0, im = 0;
  for (int s = 0; s < p.nsplit; ++s) {
    const long long* o = p.part + (((size_t)s * p.ncand + cand) * p.nphi + k) * 2;
    re += o[0];
    im += o[1];
  }
  rm_store2(p.out + ((size_t)cand * p.nphi + k) * 2, re, im, p.cand[cand].inv);
}

// ---------------------------------------------------------------------------------------------------------------------
// The delay x RM transform (HIP only; frbch_post_rmd of kernels_post.inc stays the emulable form and the fallback; both call
// rm_term).  frbch_post_rm_fast with a second axis in registers: a thread carries T consecutive tau trials next to its
// kRmKpt phi trials, so that one staged record and one first-phase product (p0 + k0 d + m0 e) serve kRmKpt x T terms, each
// further one at one 64-bit addition.  The accumulators are 4 kRmKpt T VGPRs, 128 at T = 8; the compiler's counts are 59,
// 56, 90 and 169 VGPRs at T = 1, 2, 4 and 8, none spilled (profiles/polcal_resusage.txt).  The 72 KiB of LDS admit two
// workgroups a CU, that is two waves a SIMD with 256 VGPRs each, so T = 8 costs no occupancy that the LDS had not taken
// already; at T = 16 the accumulators alone would be those 256.  T is the host's choice
// (rmd_plan_rule): a tail tile computes its trials beyond ntau in vain, so short or ragged tau axes take a smaller T.
// blockIdx.y = tau tile x nsplit + split, grid (ceil(nphi / 1024), ceil(ntau / T) nsplit, ncand).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kRmdTile = 256, kRmdTauMax = 8;
constexpr size_t kRmdLds = 65536 + (size_t)kRmdTile * sizeof(RmdRec);

template <int T>
__global__ void __launch_bounds__(kRmThreads) frbch_post_rmd_fast(RmdParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* tab = reinterpret_cast<int32_t*>(smem);
  RmdRec* recs = reinterpret_cast<RmdRec*>(smem + 65536);
  const int tid = threadIdx.x, cand = blockIdx.z;
  const int split = (int)blockIdx.y % p.nsplit, m0 = ((int)blockIdx.y / p.nsplit) * T;
  const int k0 = (int)blockIdx.x * (kRmThreads * kRmKpt) + tid;
  for (int i = tid; i < 4096; i += kRmThreads) reinterpret_cast<int4*>(tab)[i] = reinterpret_cast<const int4*>(p.table)[i];
  const RmCand cd = p.cand[cand];
  const int r0 = split * p.chunk;
  const int r1 = min(r0 + p.chunk, (int)cd.nrec);
  long long re[kRmKpt][T], im[kRmKpt][T];
#pragma unroll
  for (int j = 0; j < kRmKpt; ++j)
#pragma unroll
    for (int m = 0; m < T; ++m) re[j][m] = im[j][m] = 0;
  for (int t0 = r0; t0 < r1; t0 += kRmdTile) {
    const int n = min(kRmdTile, r1 - t0);
    __syncthreads();                                                       // the previous tile is consumed
    const uint32_t* srcw = reinterpret_cast<const uint32_t*>(p.rec + (size_t)cand * p.nchan + t0);
    for (int i = tid; i < n * 8; i += kRmThreads) reinterpret_cast<uint32_t*>(recs)[i] = srcw[i];
    __syncthreads();                                                       // (the first one covers the table as well)
    for (int r = 0; r < n; ++r) {
      const RmdRec rc = recs[r];
      unsigned long long ph = rc.p0 + rc.d * (unsigned long long)(uint32_t)k0 + rc.e * (unsigned long long)(uint32_t)m0;
      const unsigned long long step = rc.d << 8;                           // kRmThreads D
#pragma unroll
      for (int j = 0; j < kRmKpt; ++j) {
        unsigned long long pm = ph;
#pragma unroll
        for (int m = 0; m < T; ++m) {
          rm_term(tab, pm, rc.qi, rc.ui, &re[j][m], &im[j][m]);
          pm += rc.e;
        }
        ph += step;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kRmKpt; ++j) {
    const int k = k0 + j * kRmThreads;
#pragma unroll
    for (int m = 0; m < T; ++m) {
      if (k < p.nphi && m0 + m < p.ntau) {
        const size_t o = ((size_t)cand * p.ntau + (size_t)(m0 + m)) * p.nphi + k;
        if (p.nsplit == 1) {
          rm_store2(p.out + o * 2, re[j][m], im[j][m], cd.inv);
        } else {
          long long* q = p.part + ((size_t)split * p.ncand * p.ntau * p.nphi + o) * 2;
          q[0] = re[j][m];
          q[1] = im[j][m];
        }
      }
    }
  }
}

// grid (ceil(ntau nphi / 256), ncand): the partials of the splits, added in ascending split
__global__ void __launch_bounds__(kRmThreads) frbch_post_rmd_join(RmdParams p) {
  const size_t per = (size_t)p.ntau * p.nphi, idx = (size_t)blockIdx.x * kRmThreads + threadIdx.x;
  const int cand = blockIdx.y;
  if (idx >= per) return;
  const size_t o = (size_t)cand * per + idx;
  long long re = 0, im = 0;
  for (int s = 0; s < p.nsplit; ++s) {
    const long long* q = p.part + ((size_t)s * p.ncand * per + o) * 2;
    re += q[0];
    im += q[1];
  }
  rm_store2(p.out + o * 2, re, im, p.cand[cand].inv);
}

// ---------------------------------------------------------------------------------------------------------------------
// Polarisation profile (HIP only; frbch_post_polprof of kernels_post.inc stays the emulable form and the fallback; both call
// pp_term).  A workgroup of 256 threads owns one candidate, one 64-byte tile of the row (CT = 64 / 32 channels of 8- / 16-bit
// samples) and a run of `brun` bins.  It stages the rows the run needs -- from its first bin's first row at the tile's
// smallest delay (tile_delay_range) to its last bin's last row at the largest: nb tfactor + (dmax - dmin) <= kPpSpan rows,
// the host's plan rule sees to that -- of all four products (tile_stage).  Then one thread per (channel, bin), 256 / CT bins
// per trip, sums its tfactor samples at its own delay from the LDS (tile_row_add), forms its term, and the CT lanes of a bin
// add theirs up by shuffles; lane 0 stores the tile's int64 partial.  Rows outside the file are neither loaded nor read.
// frbch_post_polprof_join adds the tiles in ascending order.  All row arithmetic is 64 bit.
// grid (row bytes / 64, ceil(nbin / brun), ncand).
// ---------------------------------------------------------------------------------------------------------------------
// The three blocks that the profile, DM scan and dynamic spectrum kernels share: a workgroup of kTileThreads threads on one
// 64-byte tile of the row, CT = 64 / BPV channels, lanes along the channels.
constexpr int kTileThreads = 256;

// the smallest and largest delay over the CT lanes of a tile, by shuffles: the same in every thread afterwards
template <int BPV> __device__ __forceinline__ void tile_delay_range(int& dmin, int& dmax) {
#pragma unroll
  for (int m = 1; m < 64 / BPV; m <<= 1) {
    dmin = min(dmin, __shfl_xor(dmin, m));
    dmax = max(dmax, __shfl_xor(dmax, m));
  }
}

// `span` rows from file row `base` on, NP products of each, into the LDS as [row][product][64 bytes] in 16-byte pieces, four
// lanes side by side on the 64 bytes of a product (src: the tile's bytes of the first product read in row 0; stride, pstride:
// the bytes of a row and of a product).  Rows outside the file are not loaded.  The caller synchronises.
template <int NP>
__device__ __forceinline__ void tile_stage(unsigned char* smem, const unsigned char* src, size_t stride, size_t pstride, long long base,
                                           int span, long long nrows, int tid) {
  constexpr int PIECES = 4 * NP;                                           // of a staged row
  for (int i = tid; i < span * PIECES; i += kTileThreads) {
    const long long row = base + (long long)(i / PIECES);
    if (row >= 0 && row < nrows)
      *reinterpret_cast<uint4*>(smem + (size_t)i * 16) =
          *reinterpret_cast<const uint4*>(src + (size_t)row * stride + (size_t)((i >> 2) % NP) * pstride + (size_t)(i & 3) * 16);
  }
}

// The window sum, one staged row of it: a channel's samples of the NP products (q: its sample of the first) added to NS = NP
// sums, one a product, or to NS = 1, the products together.  The loop over the rows of a window stays in the kernels: inside
// this function it changes how the compiler unrolls the profile kernel's (64 VGPRs against 56).
template <int BPV, int NP, int NS>
__device__ __forceinline__ void tile_row_add(const unsigned char* q, uint32_t (&S)[NS]) {
  static_assert(NS == 1 || NS == NP, "one sum, or one a product");
#pragma unroll
  for (int pr = 0; pr < NP; ++pr) {
    if constexpr (BPV == 1) S[pr % NS] += (uint32_t)q[pr * 64];
    else S[pr % NS] += (uint32_t)*reinterpret_cast<const uint16_t*>(q + pr * 64);
  }
}

constexpr int kPpThreads = kTileThreads, kPpSpan = 256;
constexpr size_t kPpLds = (size_t)kPpSpan * 256;                           // 64 KiB: two workgroups per CU

template <int BPV>
__global__ void __launch_bounds__(kPpThreads) frbch_post_polprof_fast(PolParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CT = 64 / BPV, BPP = kPpThreads / CT;
  const int tid = threadIdx.x, ch = tid % CT, jl = tid / CT;
  const int tile = blockIdx.x, cand = blockIdx.z;
  const int j0 = (int)blockIdx.y * p.brun;
  const int nb = min(p.brun, p.nbin - j0);
  const PolCand cd = p.cand[cand];
  const PolRec r = p.rec[(size_t)cand * p.nchan + (size_t)tile * CT + ch];
  int dmin = r.delay, dmax = r.delay;
  tile_delay_range<BPV>(dmin, dmax);
  const long long nrows = (long long)p.nrows;
  const long long base = cd.t0 + (long long)j0 * (long long)p.tfactor + (long long)dmin;     // the file row of LDS row 0
  const int span = nb * p.tfactor + (dmax - dmin);
  const size_t stride = (size_t)4 * p.nchan * BPV, pstride = (size_t)p.nchan * BPV;
  tile_stage<4>(smem, p.rows + (size_t)tile * 64, stride, pstride, base, span, nrows, tid);
  __syncthreads();
  for (int jb0 = 0; jb0 < nb; jb0 += BPP) {                                // (the same trips in every thread: the shuffles meet whole waves)
    const int jb = jb0 + jl;
    long long a[4] = {0, 0, 0, 0};
    uint32_t h = 0;
    if (jb < nb && r.used) {
      const long long b0 = cd.t0 + (long long)(j0 + jb) * (long long)p.tfactor;
      long long lo, hi;
      burst_clip(b0, (uint32_t)p.tfactor, (long long)r.delay, nrows, &lo, &hi);
      if (hi > lo) {
        uint32_t S[4] = {0, 0, 0, 0};
        const unsigned char* q = smem + (size_t)(lo - base) * 256 + (size_t)ch * BPV;
        for (long long t = lo; t < hi; ++t, q += 256) tile_row_add<BPV, 4>(q, S);
        h = (uint32_t)(hi - lo);
        pp_term(r, p.coh, cd.scale, S, h, a);
      }
    }
#pragma unroll
    for (int m = 1; m < CT; m <<= 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] += __shfl_xor(a[k], m);
      h += __shfl_xor(h, m);
    }
    if (ch == 0 && jb < nb) {
      const size_t o = ((size_t)cand * p.ntile + tile) * p.nbin + (size_t)(j0 + jb);
      p.part[o * 4 + 0] = a[0]; p.part[o * 4 + 1] = a[1]; p.part[o * 4 + 2] = a[2]; p.part[o * 4 + 3] = a[3];
      p.hpart[o] = h;
    }
  }
}

// grid (ceil(nbin / 256), ncand): the partials of the tiles, added in ascending tile
__global__ void __launch_bounds__(kPpThreads) frbch_post_polprof_join(PolParams p) {
  const int j = (int)blockIdx.x * kPpThreads + (int)threadIdx.x, cand = blockIdx.y;
  if (j >= p.nbin) return;
  long long a[4] = {0, 0, 0, 0};
  uint32_t h = 0;
  for (int t = 0; t < p.ntile; ++t) {
    const size_t o = ((size_t)cand * p.ntile + t) * p.nbin + (size_t)j;
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += p.part[o * 4 + k];
    h += p.hpart[o];
  }
  long long* out = p.acc + ((size_t)cand * p.nbin + j) * 4;
  out[0] = a[0]; out[1] = a[1]; out[2] = a[2]; out[3] = a[3];
  p.hits[(size_t)cand * p.nbin + j] = h;
}

// ---------------------------------------------------------------------------------------------------------------------
// DM of a burst (HIP only; frbch_post_dmscan of kernels_post.inc stays the emulable form and the fallback; both call dm_term).
// What is new against the profile kernel above is reuse: a staged row serves every trial of a run, not one.  A workgroup of 256
// threads owns one candidate, one 64-byte tile of the row (CT = 64 / 32 channels of 8- / 16-bit samples), a run of `trun`
// trials and a run of `brun` bins.  It stages the rows the bins need over the delay range of its tile over its trials -- from
// its first bin's first row at the smallest delay to its last bin's last row at the largest: nb tfactor + (dmax - dmin) <=
// kDmLds / (64 NP) rows, the host's plan rule sees to that -- of the NP products read (tile_stage).  Then, trial after
// trial, one thread per (channel, bin), 256 / CT bins per trip, sums its tfactor samples at its channel's delay of that
// trial from the LDS (tile_row_add) and forms its term; the CT lanes of a bin add theirs up by
// shuffles and lane 0 stores the tile's int64 partial.  Lanes run along the channels, so a wave reads neighbouring bytes of
// one or two LDS rows: no bank collides (lanes along the bins would, at a row stride of 64 bytes).  Rows outside the file are
// neither loaded nor read.  frbch_post_dmscan_join adds the tiles in ascending order.  All row arithmetic is 64 bit.
// grid (tiles x ceil(nbin / brun), ceil(ntrial / trun), ncand).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kDmThreads = kTileThreads, kDmTrun = 16, kDmMaxT = 256;
constexpr size_t kDmLds = 65536;                                           // 64 KiB: two workgroups per CU

template <int BPV, int NP>
__global__ void __launch_bounds__(kDmThreads) frbch_post_dmscan_fast(DmParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CT = 64 / BPV, BPP = kDmThreads / CT, ROWB = 64 * NP, CAP = (int)(kDmLds / ROWB);
  const int tid = threadIdx.x, ch = tid % CT, jl = tid / CT;
  const int tile = (int)blockIdx.x % p.ntile, cand = blockIdx.z;
  const int j0 = ((int)blockIdx.x / p.ntile) * p.brun, k0 = (int)blockIdx.y * p.trun;
  const int nb = min(p.brun, p.nbin - j0), nk = min(p.trun, p.ntrial - k0);
  const DmCand cd = p.cand[cand];
  const DmRec r = p.rec[(size_t)cand * p.nchan + (size_t)tile * CT + ch];
  const int32_t* dl = p.delays + ((size_t)cand * p.ntrial + k0) * p.nchan + (size_t)tile * CT + ch;
  int dmin = dl[0], dmax = dl[0];
  for (int k = 1; k < nk; ++k) {
    const int d = dl[(size_t)k * p.nchan];
    dmin = min(dmin, d);
    dmax = max(dmax, d);
  }
  tile_delay_range<BPV>(dmin, dmax);
  const long long nrows = (long long)p.nrows;
  const long long base = cd.t0 + (long long)j0 * (long long)p.tfactor + (long long)dmin;     // the file row of LDS row 0
  const long long span = (long long)nb * p.tfactor + ((long long)dmax - (long long)dmin);
  if (span > CAP) return;                                                  // (the plan rule never launches such a run)
  const size_t stride = (size_t)p.nifs * p.nchan * BPV, pstride = (size_t)p.nchan * BPV;
  tile_stage<NP>(smem, p.rows + (size_t)p.p0 * pstride + (size_t)tile * 64, stride, pstride, base, (int)span, nrows, tid);
  __syncthreads();
  for (int k = 0; k < nk; ++k) {                                           // (the same trips in every thread: the shuffles meet whole waves)
    const long long delay = (long long)dl[(size_t)k * p.nchan];
    for (int jb0 = 0; jb0 < nb; jb0 += BPP) {
      const int jb = jb0 + jl;
      long long a = 0;
      uint32_t h = 0;
      if (jb < nb && r.used) {
        const long long b0 = cd.t0 + (long long)(j0 + jb) * (long long)p.tfactor;
        long long lo, hi;
        burst_clip(b0, (uint32_t)p.tfactor, delay, nrows, &lo, &hi);
        if (hi > lo) {
          uint32_t S[1] = {0};
          const unsigned char* q = smem + (size_t)(lo - base) * ROWB + (size_t)ch * BPV;
          for (long long t = lo; t < hi; ++t, q += ROWB) tile_row_add<BPV, NP>(q, S);
          h = (uint32_t)(hi - lo);
          a = dm_term(r.mean, r.w, cd.scale, S[0], h);
        }
      }
#pragma unroll
      for (int m = 1; m < CT; m <<= 1) {
        a += __shfl_xor(a, m);
        h += __shfl_xor(h, m);
      }
      if (ch == 0 && jb < nb) {
        const size_t o = (((size_t)cand * p.ntile + tile) * p.ntrial + (size_t)(k0 + k)) * p.nbin + (size_t)(j0 + jb);
        p.part[o] = a;
        p.hpart[o] = h;
      }
    }
  }
}

// grid (ceil(ncand ntrial nbin / 256)): the partials of the tiles, added in ascending tile
__global__ void __launch_bounds__(kDmThreads) frbch_post_dmscan_join(DmParams p) {
  const size_t per = (size_t)p.ntrial * p.nbin, idx = (size_t)blockIdx.x * kDmThreads + threadIdx.x;
  if (idx >= (size_t)p.ncand * per) return;
  const size_t cand = idx / per, kj = idx % per;
  long long a = 0;
  uint32_t h = 0;
  for (int t = 0; t < p.ntile; ++t) {
    const size_t o = (cand * p.ntile + t) * per + kj;
    a += p.part[o];
    h += p.hpart[o];
  }
  p.acc[idx] = a;
  p.hits[idx] = h;
}

// ---------------------------------------------------------------------------------------------------------------------
// Structure of a burst, the dynamic spectrum (HIP only; frbch_post_dynspec of kernels_post.inc stays the emulable form and the
// fallback; both call dm_term).  frbch_post_dmscan_fast at one trial, built from the same three blocks: a workgroup of 256
// threads owns one candidate, one 64-byte tile of the row (CT = 64 / 32 channels) and a run of `brun` bins, and stages the rows
// those bins need over the delay range of its tile -- nb tfactor + (dmax - dmin) <= kDmLds / (64 NP) rows, the host's plan rule
// (dm_stage_brun at one trial) sees to that.
// One thread per (channel, bin) forms its term; then only the gl = min(ffactor, CT) neighbouring lanes of a subband add theirs
// up by shuffles (gl is a power of two).  ffactor <= CT: the leading lane of every group stores the cell of its subband, no
// join.  ffactor a multiple of CT: gl = CT, the tile's sum is a partial and frbch_post_dynspec_join adds the ffactor / CT tiles
// of a subband in ascending order.  grid (tiles x ceil(nbin / brun), 1, ncand).
// ---------------------------------------------------------------------------------------------------------------------
template <int BPV, int NP>
__global__ void __launch_bounds__(kDmThreads) frbch_post_dynspec_fast(DynParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int CT = 64 / BPV, BPP = kDmThreads / CT, ROWB = 64 * NP, CAP = (int)(kDmLds / ROWB);
  const int tid = threadIdx.x, ch = tid % CT, jl = tid / CT;
  const int tile = (int)blockIdx.x % p.ntile, cand = blockIdx.z;
  const int j0 = ((int)blockIdx.x / p.ntile) * p.brun;
  const int nb = min(p.brun, p.nbin - j0);
  const DmCand cd = p.cand[cand];
  const DmRec r = p.rec[(size_t)cand * p.nchan + (size_t)tile * CT + ch];
  const int delay = p.delays[(size_t)cand * p.nchan + (size_t)tile * CT + ch];
  int dmin = delay, dmax = delay;
  tile_delay_range<BPV>(dmin, dmax);
  const long long nrows = (long long)p.nrows;
  const long long base = cd.t0 + (long long)j0 * (long long)p.tfactor + (long long)dmin;     // the file row of LDS row 0
  const long long span = (long long)nb * p.tfactor + ((long long)dmax - (long long)dmin);
  if (span > CAP) return;                                                  // (the plan rule never launches such a run)
  const size_t stride = (size_t)p.nifs * p.nchan * BPV, pstride = (size_t)p.nchan * BPV;
  tile_stage<NP>(smem, p.rows + (size_t)p.p0 * pstride + (size_t)tile * 64, stride, pstride, base, (int)span, nrows, tid);
  __syncthreads();
  for (int jb0 = 0; jb0 < nb; jb0 += BPP) {                                // (the same trips in every thread: the shuffles meet whole waves)
    const int jb = jb0 + jl;
    long long a = 0;
    uint32_t h = 0;
    if (jb < nb && r.used) {
      const long long b0 = cd.t0 + (long long)(j0 + jb) * (long long)p.tfactor;
      long long lo, hi;
      burst_clip(b0, (uint32_t)p.tfactor, (long long)delay, nrows, &lo, &hi);
      if (hi > lo) {
        uint32_t S[1] = {0};
        const unsigned char* q = smem + (size_t)(lo - base) * ROWB + (size_t)ch * BPV;
        for (long long t = lo; t < hi; ++t, q += ROWB) tile_row_add<BPV, NP>(q, S);
        h = (uint32_t)(hi - lo);
        a = dm_term(r.mean, r.w, cd.scale, S[0], h);
      }
    }
    for (int m = 1; m < p.gl; m <<= 1) {
      a += __shfl_xor(a, m);
      h += __shfl_xor(h, m);
    }
    if (ch % p.gl == 0 && jb < nb) {
      if (p.ffactor <= CT) {
        const size_t o = ((size_t)cand * p.nsub + (size_t)(tile * CT + ch) / p.ffactor) * p.nbin + (size_t)(j0 + jb);
        p.Y[o] = a;
        p.yhits[o] = h;
      } else {
        const size_t o = ((size_t)cand * p.ntile + tile) * p.nbin + (size_t)(j0 + jb);
        p.part[o] = a;
        p.hpart[o] = h;
      }
    }
  }
}

// grid (ceil(ncand nsub nbin / 256)): the ffactor / CT tiles of a subband, added in ascending tile (tps = tiles per subband)
__global__ void __launch_bounds__(kDmThreads) frbch_post_dynspec_join(DynParams p, int tps) {
  const size_t idx = (size_t)blockIdx.x * kDmThreads + threadIdx.x;
  if (idx >= (size_t)p.ncand * p.nsub * p.nbin) return;
  const size_t j = idx % p.nbin, is = idx / p.nbin, cand = is / p.nsub, s = is % p.nsub;
  long long a = 0;
  uint32_t h = 0;
  for (int t = 0; t < tps; ++t) {
    const size_t o = (cand * p.ntile + s * tps + t) * p.nbin + j;
    a += p.part[o];
    h += p.hpart[o];
  }
  p.Y[idx] = a;
  p.yhits[idx] = h;
}

// ---------------------------------------------------------------------------------------------------------------------
// Structure of a burst, the two-dimensional autocorrelation (HIP only; frbch_post_acf2d of kernels_post.inc stays the emulable
// form and the fallback).  A[df][dt] = sum over s, j of y[s][j] y[s + df][j + dt], int64, exact in any order.
// A workgroup owns one plane, a run of `dfr` frequency lags from df0 and a slab of `sb` subbands from s0.  It stages
//   a: the slab's rows, [sb][nbin8] int32, nbin8 = nbin rounded up to 8, zero behind the row's end and behind the plane's, and
//   b: the rows s0 + df0 .. s0 + df0 + sb + dfr - 2, each as positions x = bin + (nlagt - 1) of a line of nbin8 + 8 nrun
//      words with zeros wherever the bin lies outside the row or the row outside the plane -- so the inner loop has no bounds.
// Thread (dfi, run) owns df = df0 + dfi and the eight time lags dt = 8 run - (nlagt - 1) + i, i < 8, in eight int64
// accumulators.  Walking j it keeps the eight b values at positions j + 8 run .. + 7 in registers: every step loads ONE new b
// word and multiplies a[j] -- read 8 bins at a time as two 16-byte broadcasts, the same address in every lane -- into all eight:
// 10 LDS reads per 64 multiply-adds, against 128 with one thread per lag.  The window rotates by renaming: the loop over eight
// steps is unrolled and position x lives in register x mod 8.
// Banks (ds_read_b32: 32 lanes a group, bank = word mod 32): the lanes of a group differ in `run`, i.e. by 8 words, which would
// put four lanes on every bank; b is therefore stored skewed, position x at word x + x / 8, which makes the lane stride 9 words,
// and the row stride bw is chosen = 9 nrunp (mod 32) so that the rows of the dfi of one group interleave as well: no conflict.
// The partial of every (plane, slab, df, dt) goes to `part`; frbch_post_acf2d_join adds the slabs in ascending order.
// grid (nslab, ceil(nlagf / dfr), n), max(64, dfr nrunp) threads, (sb nbin8 + (sb + dfr - 1) bw) 4 <= kAcfLds bytes of LDS.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kAcfThreads = 256, kAcfRun = 8, kAcfMaxDfr = 8;
constexpr size_t kAcfLds = 65536;                                          // 64 KiB: two workgroups per CU

__global__ void __launch_bounds__(kAcfThreads) frbch_post_acf2d_fast(Acf2Params p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nbin8 = (p.nbin + 7) & ~7, L = p.nlagt - 1, bwl = nbin8 + 8 * p.nrun, nbr = p.sb + p.dfr - 1;
  int32_t* sa = reinterpret_cast<int32_t*>(smem);
  int32_t* sb = sa + p.sb * nbin8;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int s0 = (int)blockIdx.x * p.sb, df0 = (int)blockIdx.y * p.dfr;
  const int ns = min(p.sb, p.nsub - s0), ndt = 2 * p.nlagt - 1;
  const int32_t* y = p.y + (size_t)blockIdx.z * p.nsub * p.nbin;
  for (int i = tid; i < p.sb * nbin8; i += nthr) {
    const int s = i / nbin8, j = i % nbin8;
    sa[i] = (s < ns && j < p.nbin) ? y[(size_t)(s0 + s) * p.nbin + j] : 0;
  }
  for (int i = tid; i < nbr * bwl; i += nthr) {
    const int q = i / bwl, x = i % bwl, s = s0 + df0 + q, j = x - L;
    sb[q * p.bw + x + (x >> 3)] = (s < p.nsub && j >= 0 && j < p.nbin) ? y[(size_t)s * p.nbin + j] : 0;
  }
  __syncthreads();
  const int run = tid % p.nrunp, dfi = tid / p.nrunp;
  if (dfi >= p.dfr || run >= p.nrun || df0 + dfi >= p.nlagf) return;
  long long acc[kAcfRun];
#pragma unroll
  for (int i = 0; i < kAcfRun; ++i) acc[i] = 0;
  for (int s = 0; s < ns; ++s) {
    const int32_t* a = sa + s * nbin8;
    const int32_t* b = sb + (s + dfi) * p.bw + 9 * run;                    // position 8 run lives at word 9 run
    int32_t w[kAcfRun];
#pragma unroll
    for (int i = 0; i < kAcfRun - 1; ++i) w[i] = b[i];
    for (int m = 0; m < nbin8 / 8; ++m, b += 9, a += 8) {
      const int4 a0 = *reinterpret_cast<const int4*>(a), a1 = *reinterpret_cast<const int4*>(a + 4);
      const int32_t av[kAcfRun] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int jj = 0; jj < kAcfRun; ++jj) {
        w[(jj + 7) & 7] = b[jj == 0 ? 7 : 8 + jj];                         // position 8 (run + m) + 7 + jj (word 9 (run + m) + 8 is the skew's gap)
#pragma unroll
        for (int i = 0; i < kAcfRun; ++i) acc[i] += (long long)av[jj] * (long long)w[(jj + i) & 7];
      }
    }
  }
  long long* out = p.part + (((size_t)blockIdx.z * p.nslab + blockIdx.x) * p.nlagf + (size_t)(df0 + dfi)) * ndt;
#pragma unroll
  for (int i = 0; i < kAcfRun; ++i)
    if (8 * run + i < ndt) out[8 * run + i] = acc[i];
}

// grid (ceil(n nlagf (2 nlagt - 1) / 256)): the partials of the slabs, added in ascending slab
__global__ void __launch_bounds__(kAcfThreads) frbch_post_acf2d_join(Acf2Params p) {
  const size_t per = (size_t)p.nlagf * (2 * p.nlagt - 1), idx = (size_t)blockIdx.x * kAcfThreads + threadIdx.x;
  if (idx >= (size_t)p.n * per) return;
  const size_t plane = idx / per, l = idx % per;
  long long a = 0;
  for (int t = 0; t < p.nslab; ++t) a += p.part[(plane * p.nslab + t) * per + l];
  p.A[idx] = a;
}

// ---------------------------------------------------------------------------------------------------------------------
// Scattering of a burst, the template-bank stage (HIP only; frbch_post_tbank of kernels_post.inc stays the emulable form and
// the fallback).  C[s][k][u] = sum over the taps m of y[s][shift0 + u - lead + m] P[k][m], int64, exact in any order.
// A workgroup owns one plane, `sw` subbands from s0 and a run of `kr` templates from k0.  It stages
//   t: the templates of its run, [kr][ntap8] int32, ntap8 = ntap rounded up to 8, zero behind the last tap and the last template,
//   l: per subband a line of 8 nrun + ntap8 positions, position x = bin shift0 - lead + x, zero wherever the bin lies outside
//      the row or the row outside the plane -- so the inner loop has no bounds.
// The 256 threads are 256 / (sw nrunp) template lanes times sw nrunp items; item (si, run) owns subband s0 + si and the eight
// shifts u = 8 run + i, i < 8, in eight int64 accumulators, and takes the templates k0 + kp, k0 + kp + 256 / (sw nrunp), ...
// Walking the taps it keeps the eight line values at positions m + 8 run .. + 7 in registers: every tap loads ONE new line
// word and multiplies P[k][m] -- read 8 taps at a time as two 16-byte reads, the same address in every lane that shares k, and
// with sw nrunp >= 64 that is the whole wave -- into all eight: 10 LDS reads per 64 multiply-adds.  The window rotates by
// renaming: the loop over eight taps is unrolled and position x lives in register x mod 8 (the scheme of
// frbch_post_acf2d_fast, with the template in the place of the slab row).
// Banks: the lanes of a wave differ in `run`, i.e. by 8 positions; a line is stored skewed, position x at word x + x / 8, which
// makes the lane stride 9 words, and the line stride lw is chosen = 9 nrunp (mod 32) so that the subbands of one wave
// interleave as well.  Nothing is reduced across workgroups: every thread stores its own eight sums, no join.
// grid (ceil(nsub / sw), ceil(ntemp / kr), n), 256 threads, (kr ntap8 + sw lw) 4 <= kTbLds bytes of LDS.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kTbThreads = 256, kTbRun = 8, kTbMaxSw = 8;
constexpr size_t kTbLds = 65536;                                           // 64 KiB: two workgroups per CU

__global__ void __launch_bounds__(kTbThreads) frbch_post_tbank_fast(TbankParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lwl = 8 * p.nrun + p.ntap8, items = p.sw * p.nrunp;
  int32_t* st = reinterpret_cast<int32_t*>(smem);
  int32_t* sl = st + p.kr * p.ntap8;
  const int tid = threadIdx.x;
  const int s0 = (int)blockIdx.x * p.sw, k0 = (int)blockIdx.y * p.kr;
  const int nk = min(p.kr, p.ntemp - k0);
  const int32_t* y = p.y + (size_t)blockIdx.z * p.nsub * p.nbin;
  for (int i = tid; i < p.kr * p.ntap8; i += kTbThreads) {
    const int kk = i / p.ntap8, m = i % p.ntap8;
    st[i] = (kk < nk && m < p.ntap) ? p.P[(size_t)(k0 + kk) * p.ntap + m] : 0;
  }
  for (int i = tid; i < p.sw * lwl; i += kTbThreads) {
    const int q = i / lwl, x = i % lwl, s = s0 + q, j = p.shift0 - p.lead + x;
    sl[q * p.lw + x + (x >> 3)] = (s < p.nsub && j >= 0 && j < p.nbin) ? y[(size_t)s * p.nbin + j] : 0;
  }
  __syncthreads();
  const int item = tid % items, kp = tid / items, kpar = kTbThreads / items;
  const int run = item % p.nrunp, si = item / p.nrunp;
  if (run >= p.nrun || s0 + si >= p.nsub) return;
  const int32_t* line = sl + si * p.lw + 9 * run;                          // position 8 run lives at word 9 run
  for (int kk = kp; kk < nk; kk += kpar) {
    long long acc[kTbRun];
#pragma unroll
    for (int i = 0; i < kTbRun; ++i) acc[i] = 0;
    const int32_t* a = st + kk * p.ntap8;
    const int32_t* b = line;
    int32_t w[kTbRun];
#pragma unroll
    for (int i = 0; i < kTbRun - 1; ++i) w[i] = b[i];
    for (int m = 0; m < p.ntap8 / 8; ++m, b += 9, a += 8) {
      const int4 a0 = *reinterpret_cast<const int4*>(a), a1 = *reinterpret_cast<const int4*>(a + 4);
      const int32_t av[kTbRun] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int jj = 0; jj < kTbRun; ++jj) {
        w[(jj + 7) & 7] = b[jj == 0 ? 7 : 8 + jj];                         // position 8 (run + m) + 7 + jj (word 9 (run + m) + 8 is the skew's gap)
#pragma unroll
        for (int i = 0; i < kTbRun; ++i) acc[i] += (long long)av[jj] * (long long)w[(jj + i) & 7];
      }
    }
    long long* out = p.C + (((size_t)blockIdx.z * p.nsub + (size_t)(s0 + si)) * p.ntemp + (size_t)(k0 + kk)) * p.nshift;
#pragma unroll
    for (int i = 0; i < kTbRun; ++i)
      if (8 * run + i < p.nshift) out[8 * run + i] = acc[i];
  }
}
}  // namespace fast

// ---------------------------------------------------------------------------------------------------------------------
// Refinement of a fold (HIP only; frbch_post_ff_dm / frbch_post_ff_spin of kernels_post.inc stay the emulable forms and the
// fallback; the sums are exact integers and the score goes through ff_term, ff_mean and the 64 partial sums of the header).
//
// Stage 1, frbch_post_ff_dm_fast: per sub-integration a dedispersion with circular time.  A workgroup owns (a run of
// kFfTileRun channel tiles, kFfND consecutive DMs, one sub-integration).  A tile is 8 channels -- 64 bytes of every cube row
// -- of all nbin bins, read coalesced along the channels, the masked products added and converted to uint32 on the way,
// transposed into the LDS as val[channel][bin] and hit[channel][bin] with rows lstride = 32 ceil(nbin / 32) + 4 words apart:
// the 32 lanes of a ds_write group (4 bins x 8 channels) land on 32 banks, and in the main loop consecutive lanes read
// consecutive words (65792 bytes at 1024 bins: a little above 64 KiB, so the launch asks for its dynamic LDS).  A thread keeps BPT bins x kFfND DMs in registers (3 VGPRs each: 96 at BPT = 4).  The host's plan rule
// (ff_plan_rule) holds the sums to uint32: (2^nbits - 1) products L < 2^32 and L nchan < 2^32, L the rows of a
// sub-integration -- a cube of frbch_foldp_* has 0 <= P <= (2^nbits - 1) hits and hits <= L.  With more than one run of
// tiles the partial sums go to part / hpart and frbch_post_ff_dm_join adds them: no global atomics.
//
// Stage 2, frbch_post_ff_spin_fast: a workgroup owns (one DM, a run of R = 32 / BPT spin trials) and walks the
// sub-integrations in chunks of p.sc, whose A (int64) and HA (uint32, the same bound) lie in 64 KiB of LDS; a thread keeps
// BPT bins x R trials of B and H in registers (4 VGPRs each: 128).  Then the stage is reused for the terms of the score,
// term[trial][bin], which 64 threads a trial add into the partial sums in the order of the header, and one thread a trial
// adds those: only the score leaves the chip (and the profiles, where the caller asked for them).
// ---------------------------------------------------------------------------------------------------------------------
namespace fast {
constexpr int kFfThreads = 256, kFfCT = 8, kFfND = 8, kFfTileRun = 32, kFfMaxBin1 = 1024, kFfElems = 32;
constexpr size_t kFfStage2 = 64 * 1024;                                    // the sub-integration chunk, then the terms
constexpr size_t kFfLds2 = kFfStage2 + (size_t)kFfElems * 64 * sizeof(double) + kFfElems * sizeof(int);

template <int BPT>
__global__ void __launch_bounds__(kFfThreads) frbch_post_ff_dm_fast(FfParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* val = reinterpret_cast<uint32_t*>(smem);                       // [kFfCT][lstride]
  uint32_t* hit = val + kFfCT * p.lstride;                                 // [kFfCT][lstride]
  const int tid = threadIdx.x, s = blockIdx.z, k0 = blockIdx.x * kFfND, grp = blockIdx.y;      // grid (DM runs, tile runs, nsub)
  const int ntile = p.nchan / kFfCT;
  const int t0 = grp * kFfTileRun, t1 = min(ntile, t0 + kFfTileRun);
  unsigned long long a[kFfND][BPT];
  uint32_t h[kFfND][BPT];
#pragma unroll
  for (int d = 0; d < kFfND; ++d)
#pragma unroll
    for (int m = 0; m < BPT; ++m) { a[d][m] = 0; h[d][m] = 0; }
  for (int tile = t0; tile < t1; ++tile) {
    const int c0 = tile * kFfCT;
    __syncthreads();                                                       // the previous tile is consumed
    for (int i = tid; i < p.nbin * kFfCT; i += kFfThreads) {
      const int c = i & (kFfCT - 1), b = i / kFfCT;
      uint32_t v = 0, hh = 0;
      if (p.use[c0 + c]) {
        for (int q = 0; q < p.nifs; ++q)
          if ((p.products >> q) & 1) v += (uint32_t)(long long)p.cube[(((size_t)s * p.nifs + q) * p.nbin + b) * p.nchan + c0 + c];
        hh = p.chits[((size_t)s * p.nbin + b) * p.nchan + c0 + c];
      }
      val[c * p.lstride + b] = v;
      hit[c * p.lstride + b] = hh;
    }
    __syncthreads();
    for (int c = 0; c < kFfCT; ++c) {
      const uint32_t* vr = val + c * p.lstride;
      const uint32_t* hr = hit + c * p.lstride;
#pragma unroll
      for (int d = 0; d < kFfND; ++d) {
        const int k = min(k0 + d, p.ndm - 1);                              // (a run past ndm repeats the last DM, never stored)
        const int sh = p.shd[(size_t)k * p.nchan + c0 + c];
#pragma unroll
        for (int m = 0; m < BPT; ++m) {
          const int b = tid + m * kFfThreads;
          if (b < p.nbin) {
            int j = b + sh;
            if (j >= p.nbin) j -= p.nbin;
            a[d][m] += vr[j];
            h[d][m] += hr[j];
          }
        }
      }
    }
  }
  const size_t plane = (size_t)p.ndm * p.nsub * p.nbin;
#pragma unroll
  for (int d = 0; d < kFfND; ++d)
#pragma unroll
    for (int m = 0; m < BPT; ++m) {
      const int b = tid + m * kFfThreads;
      if (k0 + d < p.ndm && b < p.nbin) {
        const size_t at = ((size_t)(k0 + d) * p.nsub + s) * p.nbin + b;
        if (p.ngrp == 1) {
          p.A[at] = (long long)a[d][m];
          p.HA[at] = h[d][m];
        } else {
          p.part[(size_t)grp * plane + at] = (long long)a[d][m];
          p.hpart[(size_t)grp * plane + at] = h[d][m];
        }
      }
    }
}

// grid (ceil(ndm nsub nbin / 256)), one thread per element of A: the runs of tiles ascending
__global__ void __launch_bounds__(kFfThreads) frbch_post_ff_dm_join(FfParams p) {
  const size_t plane = (size_t)p.ndm * p.nsub * p.nbin;
  const size_t at = (size_t)blockIdx.x * kFfThreads + threadIdx.x;
  if (at >= plane) return;
  long long a = 0;
  unsigned long long h = 0;
  for (int g = 0; g < p.ngrp; ++g) { a += p.part[(size_t)g * plane + at]; h += p.hpart[(size_t)g * plane + at]; }
  p.A[at] = a;
  p.HA[at] = h;
}

template <int BPT>
__global__ void __launch_bounds__(kFfThreads) frbch_post_ff_spin_fast(FfParams p) {
  POST_NO_CONTRACT
  constexpr int R = kFfElems / BPT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  long long* As = reinterpret_cast<long long*>(smem);                      // [sc][nbin]
  uint32_t* Hs = reinterpret_cast<uint32_t*>(As + (size_t)p.sc * p.nbin);  // [sc][nbin]
  double* term = reinterpret_cast<double*>(smem);                          // [R][nbin], once the sums are done
  double* parts = reinterpret_cast<double*>(smem + kFfStage2);             // [R][64]
  int* cnt = reinterpret_cast<int*>(parts + kFfElems * 64);                // [R]: bins with hits
  const int tid = threadIdx.x, k = blockIdx.x / p.nrun, r0 = (blockIdx.x % p.nrun) * R;       // grid (ndm * runs of trials)
  long long B[R][BPT];
  unsigned long long H[R][BPT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < BPT; ++m) { B[r][m] = 0; H[r][m] = 0; }
  for (int s0 = 0; s0 < p.nsub; s0 += p.sc) {
    const int ns = min(p.sc, p.nsub - s0);
    const size_t base = ((size_t)k * p.nsub + s0) * p.nbin;
    __syncthreads();                                                       // the previous chunk is consumed
    for (int i = tid; i < ns * p.nbin; i += kFfThreads) {
      As[i] = p.A[base + i];
      Hs[i] = (uint32_t)p.HA[base + i];
    }
    __syncthreads();
    for (int si = 0; si < ns; ++si) {
      const long long* ar = As + (size_t)si * p.nbin;
      const uint32_t* hr = Hs + (size_t)si * p.nbin;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int sp = min(r0 + r, p.nspin - 1);                           // (a run past nspin repeats the last trial, never stored)
        const int sh = p.shp[(size_t)sp * p.nsub + s0 + si];
#pragma unroll
        for (int m = 0; m < BPT; ++m) {
          const int b = tid + m * kFfThreads;
          if (b < p.nbin) {
            int j = b + sh;
            if (j >= p.nbin) j -= p.nbin;
            B[r][m] += ar[j];
            H[r][m] += hr[j];
          }
        }
      }
    }
  }
  __syncthreads();                                                         // the stage is consumed: it holds the terms from here
  if (tid < R) cnt[tid] = 0;
  __syncthreads();
  int any = 0;
  const double M = ff_mean(p, k, &any);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int n = 0;
#pragma unroll
    for (int m = 0; m < BPT; ++m) {
      const int b = tid + m * kFfThreads;
      if (b < p.nbin) {
        term[(size_t)r * p.nbin + b] = ff_term(B[r][m], H[r][m], M);
        if (H[r][m]) ++n;
        if (p.pacc && r0 + r < p.nspin) {
          const size_t at = ((size_t)k * p.nspin + r0 + r) * p.nbin + b;
          p.pacc[at] = B[r][m];
          p.phits[at] = H[r][m];
        }
      }
    }
    if (n) atomicAdd(&cnt[r], n);                                          // (an LDS counter)
  }
  __syncthreads();
  for (int job = tid; job < R * 64; job += kFfThreads) {
    const int r = job >> 6, q = job & 63;
    double part = 0.0;
    for (int b = q; b < p.nbin; b += 64) part = part + term[(size_t)r * p.nbin + b];
    parts[job] = part;
  }
  __syncthreads();
  if (tid < R && r0 + tid < p.nspin) {
    double sum = 0.0;
    for (int q = 0; q < 64; ++q) sum = sum + parts[tid * 64 + q];
    p.score[(size_t)k * p.nspin + r0 + tid] = any && cnt[tid] >= 2 ? sum : 0.0;
  }
}
}  // namespace fast
