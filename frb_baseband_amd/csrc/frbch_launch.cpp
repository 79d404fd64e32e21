// libfrbch: plan -> kernel launches.  The only translation unit that includes the kernel sources: every HIP kernel of the library is
// instantiated and launched here (frbch_internal.h lists the units).
#include "frbch_internal.h"

#include "kernels_generic.inc"
#ifndef FRBCH_NO_FAST
#include "kernels_fast.inc"
#include "kernels_k2priv.inc"
#endif

namespace frbchi {

int upload_table(frbch_handle* h, cf** dst, uint64_t n, uint64_t count, uint64_t step) {
  std::vector<float> tmp(2 * count);
  fill_twiddles(tmp.data(), n, count, step);
  CHECK_DEV(h, dev_malloc((void**)dst, count * sizeof(cf)), "hipMalloc(twiddles)");
  CHECK_DEV(h, dev_h2d(*dst, tmp.data(), count * sizeof(cf), h->stream), "upload twiddles");
  CHECK_DEV(h, dev_sync(h->stream), "sync");
  return FRBCH_OK;
}

KParams base_params(const frbch_handle* h) {
  const Plan& pl = h->pl;
  KParams p;
  memset(&p, 0, sizeof p);
  p.log2_c2 = pl.log2_c2;
  p.log2_r = pl.log2_r;
  p.c = pl.c;
  p.c2 = pl.c2;
  p.r = pl.r;
  p.g = pl.g;
  p.log2_g = 0;
  while ((1 << p.log2_g) < pl.g) ++p.log2_g;
  p.tt = pl.tt;
  p.tscr = pl.tscr;
  p.nif = pl.nif;
  p.pol_mode = h->cfg.pol_mode;
  p.nbit = h->cfg.nbit_out;
  p.flip = pl.flip;
  p.log2_nlo = pl.log2_nlo;
  p.in_bits = pl.in_bits;
  p.spill = h->spill;
  p.gs = pl.gs;
  p.s_dc = h->s_dc;
  p.p0 = h->p0;
  p.tw_r = h->tw_r;
  p.tw_c2 = h->tw_c2;
  p.tw_nhi = h->tw_nhi;
  p.tw_nlo = h->tw_nlo;
  p.ftw1_r = h->ftw1_r;
  p.ftw2_r = h->ftw2_r;
  p.ftw1_c = h->ftw1_c;
  p.ftw2_c = h->ftw2_c;
  p.td1 = h->td1;
  p.td2 = h->td2;
  p.offset = h->offset;
  p.scale = h->scale;
  {   // 2-bit level table: DSPSR's static one unless the configuration brings its own
    const float* lv = h->cfg.levels;
    const bool own = lv[0] != 0.f || lv[1] != 0.f || lv[2] != 0.f || lv[3] != 0.f;
    static const float dflt[4] = {-3.3359f, -1.0f, 1.0f, 3.3359f};
    for (int i = 0; i < 4; ++i) p.lut[i] = own ? lv[i] : dflt[i];
  }
  p.digi_mean = pl.digi_mean;
  p.digi_scale = pl.digi_scale;
  p.digi_max = pl.digi_max;
  p.out_pitch = h->out_pitch ? h->out_pitch : (uint64_t)pl.c;
  p.coherent = pl.coherent;
  p.nfilt_pos = pl.nfilt_pos;
  p.keep = pl.keep;
  p.hop = pl.hop;
  p.spill2 = h->spill2;
  p.chirp = h->chirp;
  p.ptmp = h->ptmp;
  return p;
}

#ifndef FRBCH_NO_FAST
// =============================================================================================
// Kernel selection.  Every family of register-pass kernels with more than one instantiation has ONE selector below: it maps the
// plan and the per-launch inputs to the instantiation and calls its visitor once, f(kernel, KSel).  A launch passes a visitor that
// launches, setup_fast one that raises the kernel's dynamic-LDS limit and names its timing slot, wave_stat_chunks one that reads
// the threads per workgroup -- so an instantiation is added or removed in its selector and nowhere else.
// The selector also spells the instantiation's full name for the launch record (KSel::full: the template arguments the timing-slot
// name drops go in through KSel::with).
// A selector returns false when the plan has no kernel of its family (the caller runs the generic one).
// =============================================================================================
struct KSel {
  int nt;               // threads per workgroup
  size_t lds;           // dynamic LDS bytes
  const char* family;   // timing-slot name = family<targ[0],...> : the integer template arguments, trailing bools dropped
  int ntarg;
  int targ[4];
  const char* tail;     // ... and what follows them inside the brackets (frbch_k2_priv<PM,stats>)
  int nseq;             // frbch_k2_wave: sequences (time samples; x those a wave holds) per workgroup
  // the template arguments the timing-slot name leaves out, for the launch record: integers behind targ[], then bools
  int nxarg = 0, xarg[2] = {0, 0};
  int nbarg = 0;
  bool barg[3] = {false, false, false};
  std::string name() const {
    std::string s = family;
    for (int i = 0; i < ntarg; ++i) s += (i ? "," : "<") + std::to_string(targ[i]);
    return ntarg ? s + tail + ">" : s;
  }
  // the instantiation as the demangled symbol spells it: frbch_k2_wave<3, 8, 4, 2, true>
  std::string full() const {
    std::string s;
    for (int i = 0; i < ntarg; ++i) s += ", " + std::to_string(targ[i]);
    for (int i = 0; i < nxarg; ++i) s += ", " + std::to_string(xarg[i]);
    for (int i = 0; i < nbarg; ++i) s += barg[i] ? ", true" : ", false";
    return s.empty() ? std::string(family) : std::string(family) + "<" + s.substr(2) + ">";
  }
  KSel with(std::initializer_list<int> xs, std::initializer_list<bool> bs = {}) const {
    KSel a = *this;
    for (int x : xs) a.xarg[a.nxarg++] = x;
    for (bool b : bs) a.barg[a.nbarg++] = b;
    return a;
  }
};
inline KSel ksel(int nt, size_t lds, const char* family, std::initializer_list<int> targs = {}, const char* tail = "", int nseq = 0) {
  KSel a{nt, lds, family, 0, {0, 0, 0, 0}, tail, nseq, 0, {0, 0}, 0, {false, false, false}};
  for (int t : targs) a.targ[a.ntarg++] = t;
  return a;
}
// calls f(std::integral_constant<int, V>) for the V among Vs that equals v; false = none does
template <int... Vs, class F>
bool on_value(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>()), true)) || ...);
}
// the visitor of a launch
template <class K>
void launch_sel(frbch_handle* h, K kern, dim3 grid, const KSel& a, dev_stream_t s, const KParams& p) {
  if (h->profiling) note_launch(h, reinterpret_cast<const void*>(kern), [&a] { return a.full(); }, grid.x, grid.y);
  hipLaunchKernelGGL(kern, grid, dim3(a.nt), a.lds, s, p);
}
// product mode as the kernels' template argument PM: 2 = PP+QQ, 4 = four products, 0 = one of the others.  frbch_k2_priv keeps
// the Stokes form (pol_mode 5) apart from the coherency products, the other families fold it into 4
int pm_of(int pol_mode) { return pol_mode == 2 ? 2 : (pol_mode >= 4 ? 4 : 0); }
int pm_priv_of(int pol_mode) { return (pol_mode == 2 || pol_mode == 4 || pol_mode == 5) ? pol_mode : 0; }

// ---- K0: RB = input bytes per row piece, WIDE: 16-byte loads
template <class F>
bool select_k0_stage(uint32_t rb, bool wide, F&& f) {
  return on_value<1, 2, 4, 8, 16>((rb == 1 || rb == 2 || rb == 4 || rb == 8) ? (int)rb : 16, [&](auto RB) {
    // (RB = 16: pieces aligned to 16 bytes are what WIDE asks for -- launch_k0_stage never comes here with wide = false)
    if (wide) f(fast::frbch_k0_stage<RB.value, true>, ksel(256, 0, "frbch_k0_stage").with({RB.value}, {true}));
    else if constexpr (RB.value < 16) f(fast::frbch_k0_stage<RB.value, false>, ksel(256, 0, "frbch_k0_stage").with({RB.value}, {false}));
  });
}
// ---- K1, barrier form: the coherent chain.  (Not R = 4096: make_plan gives every plan whose barrier K1 fits the LDS at that length
// the wave K1, which needs less of it)
template <class F>
bool select_k1_fast(const Plan& pl, F&& f) {
  return on_value<1, 2, 3, 5>(pl.fast_k1_log2m, [&](auto L) {
    f(fast::frbch_k1_fast<L.value>, ksel(1024, pl.k1_fast_lds, "frbch_k1_fast", {L.value}));
  });
}
// ---- K1, wave form.  stg: the batch was corner-turned by frbch_k0_stage; msk (with stg only): frames flagged invalid / fillers are
// masked through one flag per n2 row beside the stage (a byte, at R = 8192 a bit)
size_t k1_wave_lds(const Plan& pl, bool msk) {
  return pl.k1_fast_lds + (msk ? (size_t)(pl.fast_k1_log2m >= 5 ? pl.r / 8 : pl.r) : 0);
}
template <int L, int WPS, bool COH, class F>
void pick_k1_wave(const Plan& pl, bool stg, bool msk, F& f) {
  const KSel a = ksel(512, k1_wave_lds(pl, stg && msk), "frbch_k1_wave", {L, 8, WPS});
  if (stg && msk) f(fast::frbch_k1_wave<L, 8, WPS, true, COH, true>, a.with({}, {true, COH, true}));
  else if (stg) f(fast::frbch_k1_wave<L, 8, WPS, true, COH, false>, a.with({}, {true, COH, false}));
  else f(fast::frbch_k1_wave<L, 8, WPS, false, COH, false>, a.with({}, {false, COH, false}));
}
template <class F>
bool select_k1_wave(const Plan& pl, bool stg, bool msk, F&& f) {
  switch (pl.fast_k1_log2m) {
    case 1: pick_k1_wave<1, 1, false>(pl, stg, msk, f); return true;
    case 2: pick_k1_wave<2, 1, false>(pl, stg, msk, f); return true;
    case 3: pick_k1_wave<3, 1, false>(pl, stg, msk, f); return true;
    case 4:   // R = 4096: two waves per branch; coherent: forward transform + delay only, spectrum spilled (K2c follows)
      if (pl.coherent) pick_k1_wave<4, 2, true>(pl, stg, msk, f);
      else pick_k1_wave<4, 2, false>(pl, stg, msk, f);
      return true;
    case 5: pick_k1_wave<5, 4, false>(pl, stg, msk, f); return true;   // R = 8192: two branches per workgroup, four waves (two virtual threads per lane) each
    default: return false;
  }
}
// ---- Kc: shares the 2C-point tables of the fast K2 (2C = 64: frbch_kc_lane, one lane per block, a single kernel)
bool kc_lane_planned(const Plan& pl) { return pl.fast_k2_lane == 1; }
template <class F>
bool select_kc_fast(const Plan& pl, F&& f) {
  return on_value<1, 2, 3, 4, 5>(pl.fast_k2_log2m, [&](auto L) {
    f(fast::frbch_kc_fast<L.value>, ksel(16 << L.value, ((size_t)pl.c2 + pl.c2 / 8 + 8 + pl.c2) * 8, "frbch_kc_fast", {L.value}));
  });
}
// ---- K2, 2C = 64 / 128: a whole sequence per lane (pair)
template <class F>
bool select_k2_lane(const Plan& pl, int pol_mode, F&& f) {
  const size_t lds = 4 * 64 * (16 * 8 + 16);   // one transposing strip per wave
  return on_value<1, 2>(pl.fast_k2_lane, [&](auto NH) {
    constexpr int nh = decltype(NH)::value;
    on_value<0, 2, 4>(pm_of(pol_mode), [&](auto PM) {
      f(fast::frbch_k2_lane<nh, PM.value>, ksel(256, lds, "frbch_k2_lane", {nh, PM.value}));
    });
  });
}
// ---- K2, 2C = 2048: one wave per time sample (kernels_k2priv.inc)
template <class F>
bool select_k2_priv(const Plan& pl, int pol_mode, int out_mode, F&& f) {
  if (!pl.fast_k2_priv) return false;
  return on_value<0, 2, 4, 5>(pm_priv_of(pol_mode), [&](auto PM) {
    const KSel a = ksel(256, pl.k2_priv_lds, "frbch_k2_priv", {PM.value}, out_mode == FRBCH_OUT_STATS ? ",stats" : "");
    if (out_mode == FRBCH_OUT_CODES) f(fast::frbch_k2_priv<PM.value, fast::K2P_CODES>, a.with({fast::K2P_CODES}));
    else if (out_mode == FRBCH_OUT_STATS) f(fast::frbch_k2_priv<PM.value, fast::K2P_STATS>, a.with({fast::K2P_STATS}));
    else f(fast::frbch_k2_priv<PM.value, fast::K2P_POWER>, a.with({fast::K2P_POWER}));
  });
}
// ---- K2, wave form: frbch_k2_wave<LOG2M, NW waves, PM, WPS waves per sequence, MSTAT>.  cols: the launch sums the rescale
// statistics or digitises (per-thread column registers in the MSTAT instantiations, where there is one)
template <int L, int NW, int PM, int WPS, bool MSTAT = false, class F>
bool pick_k2_wave(const Plan& pl, F& f) {
  f(fast::frbch_k2_wave<L, NW, PM, WPS, MSTAT>, ksel(64 * NW, pl.k2_fast_lds, "frbch_k2_wave", {L, NW, PM, WPS}, "", NW / WPS).with({}, {MSTAT}));
  return true;
}
template <int L, int NW, int WPS, class F>
bool pick_k2_wave_pm(const Plan& pl, int pm, F& f) {
  return pm == 2 ? pick_k2_wave<L, NW, 2, WPS>(pl, f) : (pm == 4 ? pick_k2_wave<L, NW, 4, WPS>(pl, f) : pick_k2_wave<L, NW, 0, WPS>(pl, f));
}
template <int L, class F>
bool pick_k2_wave_nw(const Plan& pl, int pm, F& f) {   // one wave per sequence: 2, 4 or (large tscrunch) 8 (x spw) sequences per workgroup
  return pl.fast_k2_nw == 8 ? pick_k2_wave_pm<L, 8, 1>(pl, pm, f)
                            : (pl.fast_k2_nw == 2 ? pick_k2_wave_pm<L, 2, 1>(pl, pm, f) : pick_k2_wave_pm<L, 4, 1>(pl, pm, f));
}
template <class F>
bool select_k2_wave(const Plan& pl, int pol_mode, bool cols, F&& f) {
  const int pm = pm_of(pol_mode);
  switch (pl.fast_k2_log2m) {
    case 5:
      // 2C = 8192: two time samples per workgroup (32-byte pieces of the spill lines), four waves and two virtual threads per lane
      // each; one workgroup per CU.  The instantiation with the per-thread column registers: the rescale sums while an interval is
      // being measured, the frozen offset / scale when it digitises (loaded in the emit they wait for the whole prefetch: 2.28 vs
      // 2.1 ms); the plain one for float rows without sums (two-stage tscrunch)
      if (pm == 2) return cols ? pick_k2_wave<5, 8, 2, 4, true>(pl, f) : pick_k2_wave<5, 8, 2, 4>(pl, f);
      return cols ? pick_k2_wave<5, 8, 0, 4, true>(pl, f) : pick_k2_wave<5, 8, 0, 4>(pl, f);
    case 4: return pick_k2_wave_pm<4, 8, 2>(pl, pm, f);   // 2C = 4096: two waves per sequence, 4 sequences per workgroup (make_plan: fast_k2_nw = 4)
    case 3:
      if (pl.fast_k2_nw == 8) return pick_k2_wave_pm<3, 8, 1>(pl, pm, f);   // large tscrunch: 8 sequences per workgroup, one wave per sequence
      // M = 8: two waves per sequence (16 points per lane), 2 or 4 sequences per workgroup -> 16 waves per CU
      if (pm == 4 && cols) return pl.fast_k2_nw == 2 ? pick_k2_wave<3, 4, 4, 2, true>(pl, f) : pick_k2_wave<3, 8, 4, 2, true>(pl, f);
      return pl.fast_k2_nw == 2 ? pick_k2_wave_pm<3, 4, 2>(pl, pm, f) : pick_k2_wave_pm<3, 8, 2>(pl, pm, f);
    case 2: return pick_k2_wave_nw<2>(pl, pm, f);
    case 1: return pick_k2_wave_nw<1>(pl, pm, f);
    case 0: return pl.fast_k2_m1 ? pick_k2_wave_nw<0>(pl, pm, f) : false;   // 2C = 256
    default: return false;
  }
}
// ---- K2, barrier form: 2C = 8192 only; 512 threads = one time sample per workgroup (tscrunch 1)
template <class F>
bool select_k2_fast(const Plan& pl, F&& f) {
  if (pl.fast_k2_log2m != 5) return false;
  if (pl.fast_k2_nt == 512) f(fast::frbch_k2_fast<5, 512>, ksel(512, pl.k2_fast_lds, "frbch_k2_fast", {5, 512}));
  else f(fast::frbch_k2_fast<5, 1024>, ksel(1024, pl.k2_fast_lds, "frbch_k2_fast", {5, 1024}));
  return true;
}
// ---- coherent filterbank: K2c, K3 (reported without template arguments)
template <class F>
bool select_k2c_fast(const Plan& pl, F&& f) {
  return on_value<1, 2, 3, 4, 5>(pl.coh_fast_c, [&](auto L) {
    f(fast::frbch_k2c_fast<L.value, 1024>, ksel(1024, pl.k2c_fast_lds, "frbch_k2c_fast").with({L.value, 1024}));
  });
}
// the wave K3 (R = 4096) sums the statistics of its channel: one row of partial sums per persistent workgroup
constexpr uint32_t kK3WaveWgs = 2048;
bool k3_wave_planned(const Plan& pl) {
  return pl.coherent && pl.coh_fast_r == 4 && pl.coh_nt == 512;
}
template <class F>
bool select_k3_fast(const Plan& pl, F&& f) {
  if (pl.coh_nt == 512) {   // R = 4096: the wave form
    if (!k3_wave_planned(pl)) return false;
    f(fast::frbch_k3_wave<4>, ksel(256, pl.k3_fast_lds, "frbch_k3_wave", {4}));
    return true;
  }
  return on_value<1, 2, 3, 5>(pl.coh_fast_r, [&](auto L) {
    f(fast::frbch_k3_fast<L.value, 1024>, ksel(1024, pl.k3_fast_lds, "frbch_k3_fast").with({L.value, 1024}));
  });
}
// K4 of the coherent filterbank: the register-pass transpose (a single kernel) or the generic one
bool k4_fast_planned(const Plan& pl, uint32_t h_flags) {
  return pl.ncol % 64 == 0 && pl.rows_per_block % 2 == 0 && pl.c % 4 == 0 && !(h_flags & kFlagGenericK2);   // (the flag: the generic back end)
}

// =============================================================================================
// Rows of the table of partial rescale sums
// =============================================================================================
constexpr uint32_t kFusedStatWgs = 2048;   // persistent K2 workgroups (= rows of partial sums per thread row) while statistics are fused
// frbch_k2_priv: one row of partial sums per (workgroup, row phase); `grid` = its workgroups (one per CU)
int priv_stat_chunks(const Plan& pl, int grid) { return grid * (pl.ncol / 4 >= 256 ? 1 : (int)(256 / (pl.ncol / 4))); }
// which K2 a launch of a plan with frbch_k2_priv takes: float rows stay on frbch_k2_wave (measured: four products, config 3, 1.87 ms
// per IF against 1.97; one product, config 2, 1.15 - 1.20 against 1.20 - 1.28 -- the two-wave kernel reads whole 128-byte lines,
// frbch_k2_priv halves of them twice, and writing float rows leaves less of the memory pipe to hide that), codes and statistics-only
// passes run frbch_k2_priv (steady state of config 3 + 2.4 %, config 2 + 4 %)
bool pol_mode_no_sums(int pol_mode) { return pol_mode == 3; }   // (PP+QQ)^2: its square overflows the fp32 partial sums (~1e24 squared)
bool priv_takes(const Plan& pl, const KParams& p, int priv_grid) {
  // (the two-wave kernel reads the tile-major spill only in its two-sample form: fast_k2_nw == 2, tscrunch <= 2)
  return pl.fast_k2_priv && p.tile_major == 2 && priv_grid > 0 &&
         !(p.out_mode == FRBCH_OUT_FLOAT_POWER && pl.fast_k2_nw == 2 && pl.fast_k2_log2m == 3);
}
// the frbch_k2_priv launch of `p` over nb blocks, decided here for launch_k2_fast (which launches it) and clear_partial (which tells
// it whose rows of the partial table are cleared): grid = its workgroups, a contiguous run of tiles each (0: the launch takes another
// kernel); sums = it adds into p.stat_partial, rows [0, priv_stat_chunks(pl, grid))
struct PrivLaunch {
  unsigned grid;
  bool sums;
};
PrivLaunch priv_launch(const frbch_handle* h, const KParams& p, uint32_t nb) {
  const Plan& pl = h->pl;
  if (pl.fast_k2_lane || !priv_takes(pl, p, h->priv_grid)) return {0u, false};
  const uint64_t ntiles = (uint64_t)nb * (uint64_t)(pl.r / 4);
  const bool sums = p.stat_partial && k2_wave_planned(pl) && !pl.coherent &&   // (launch_back: only the wave-private K2 sums while it writes)
                    !pol_mode_no_sums(p.pol_mode) && !(h->cfg.flags & kFlagSeparateStats);
  return {(unsigned)std::min<uint64_t>(ntiles, (uint64_t)h->priv_grid), sums};
}
// slots of fp32 sums a workgroup of that launch fills (KParams::stat_slices): one per flush, a flush every 8 trips
// (fast::kK2PFlushMask) and behind the last trip; `grid` workgroups over nb blocks of r / 4 tiles, the longest run rounded up
uint32_t priv_stat_slots(const Plan& pl, uint32_t nb, unsigned grid) {
  if (!grid) return 0;
  const uint64_t ntiles = (uint64_t)nb * (uint64_t)(pl.r / 4);
  const uint64_t trips = (ntiles + grid - 1) / grid;
  return (uint32_t)((trips + fast::kK2PFlushMask) / (fast::kK2PFlushMask + 1u));
}
// rows of partial sums the fused statistics of frbch_k2_wave / frbch_k3_wave use; 0 = this configuration cannot fuse (one column
// group per thread needed)
int wave_stat_chunks(const Plan& pl, uint32_t h_flags, int pol_mode) {
  if (pol_mode_no_sums(pol_mode) || pl.k2_two_stage) return 0;   // (two-stage tscrunch: K2 does not see the output rows)
  if (k3_wave_planned(pl)) return (h_flags & kFlagSeparateStats) ? 0 : (int)kK3WaveWgs;
  if (!k2_wave_planned(pl) || pl.coherent || (h_flags & kFlagSeparateStats)) return 0;
  int nt = 0;   // threads per workgroup of the instantiation the launch will take
  select_k2_wave(pl, pol_mode, false, [&](auto, const KSel& a) { nt = a.nt; });
  const int cg = (int)(pl.ncol / 4);
  if (!nt) return 0;
  if (cg > nt)   // a thread owns cg/nt column groups, one row of sums per workgroup (the MSTAT instantiations: 2C = 2048, two waves per sequence)
    return (cg % nt == 0 && cg / nt <= 4)
               ? (pl.fast_k2_log2m == 5 ? 256 : ((pl.fast_k2_log2m == 3 && pl.fast_k2_nw != 8) ? (int)kFusedStatWgs : 0))   // 2C = 8192: resident workgroups only
               : 0;
  if (nt % cg != 0) return 0;
  return (int)kFusedStatWgs * (nt / cg);
}
// rows of the table of partial rescale sums the kernels of this plan may write (both K2 families add into the same table: whatever
// mix of them ran, frbch_stats_final sums every row)
int fused_stat_chunks(const Plan& pl, uint32_t h_flags, int pol_mode, int priv_grid = 0) {
  const int w = wave_stat_chunks(pl, h_flags, pol_mode);
  if (pol_mode_no_sums(pol_mode) || pl.k2_two_stage || (h_flags & kFlagSeparateStats)) return w;
  return (pl.fast_k2_priv && priv_grid > 0) ? std::max(w, priv_stat_chunks(pl, priv_grid)) : w;
}

// =============================================================================================
// Launches
// =============================================================================================
void set_fastdiv(KParams& p) {
  const uint32_t d = p.payload_bytes;
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  p.div_magic = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
  p.div_shift = l ? l - 1 : 0;
}
bool launch_k1_wave(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s, int ncu) {
  const Plan& pl = h->pl;
  // persistent over blocks: the resident workgroups each keep their branch group and loop over the batch
  p.nblk = nb;
  const int kg = pl.fast_k1_g;            // branches per workgroup (<= pl.g, the layout group)
  {
    static const int ks[6] = {1, 2, 3, 4, 8, 12};
    const int step = 64 / kg;
    for (int i = 0; i < 6; ++i) {
      const double a = -2.0 * M_PI * (double)((step * ks[i]) % pl.r) / (double)pl.r;
      p.rot6[i].x = (float)cos(a);
      p.rot6[i].y = (float)sin(a);
    }
  }
  const uint32_t ngrp = (uint32_t)(pl.c2 / kg);
  const uint32_t resident = (uint32_t)(ncu > 0 ? ncu : 256) * (uint32_t)std::max<size_t>(1, (160 * 1024) / pl.k1_fast_lds);
  uint32_t ny = std::max<uint32_t>(1, std::min<uint32_t>(nb, resident / std::max<uint32_t>(1, ngrp)));
  if (ngrp > resident && ngrp % resident != 0) {
    // more branch groups than resident workgroups and not a whole number of rounds (K1 beside the digitiser, e.g. 256 groups
    // on 176 CUs): split the blocks over ny workgroups per group so that ngrp * ny fills whole rounds
    uint32_t g = ngrp, r = resident;
    while (r) { const uint32_t t = g % r; g = r; r = t; }
    const uint32_t want = resident / g;
    if (want <= nb) ny = want;
  }
  return select_k1_wave(pl, p.stg != nullptr, p.fbad != nullptr, [&](auto kern, const KSel& a) { launch_sel(h, kern, dim3(ngrp, ny), a, s, p); });
}
bool launch_k2_wave(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s, uint32_t h_flags) {
  const Plan& pl = h->pl;
  const int tps = 16 << pl.fast_k2_log2m;
  const int spw = tps < 64 ? 64 / tps : 1;
  // persistent: one wave of workgroups loops over the (tiles per block) x nb tiles of the launch
  p.nblk = nb;
  if (!wave_stat_chunks(pl, h_flags, p.pol_mode)) p.stat_partial = nullptr;
  // measured: 768 (= resident) 1.59 ms, 2048 1.56, 8192 1.49 (shorter tail); 2C = 8192, one workgroup per CU: multiples of 8 (XCD-aware tile order)
  const uint32_t npers = pl.fast_k2_log2m == 5 ? (p.stat_partial ? 256u : 1024u) : (p.stat_partial ? kFusedStatWgs : 8192u);
  const bool cols = p.stat_partial || p.out_mode != FRBCH_OUT_FLOAT_POWER;
  return select_k2_wave(pl, p.pol_mode, cols, [&](auto kern, const KSel& a) {
    const uint64_t tiles_per_block = pl.r / (a.nseq * spw);
    launch_sel(h, kern, dim3((unsigned)std::min<uint64_t>(tiles_per_block * nb, npers)), a, s, p);
  });
}
bool launch_kc_fast(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  if (kc_lane_planned(pl)) {
    p.nblk = nb;
    if (h->profiling) note_launch(h, "frbch_kc_lane", (nb + 63) / 64, 1);
    hipLaunchKernelGGL(fast::frbch_kc_lane, dim3((nb + 63) / 64), dim3(64), 0, s, p);
    return true;
  }
  return select_kc_fast(pl, [&](auto kern, const KSel& a) { launch_sel(h, kern, dim3(1, nb), a, s, p); });
}
// corner-turn of the batch's payload for the wave K1 (own timing slot); same preconditions as launch_k1_fast
void launch_k0_stage(frbch_handle* h, const KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  h->stg_ready = false;
  if (!h->stg || !pl.fast_k1_log2m || pl.c % 256 != 0 || pl.r % 64 != 0) return;
  if (pl.coherent && !h->coh_order_m) return;              // the generic K1 is in use
  const uint32_t rb = (uint32_t)(pl.fast_k1_wave ? pl.fast_k1_g : pl.g) / 2;
  if (rb < 1 || p.payload_off % rb || p.payload_bytes % rb || p.header_bytes % rb || p.frame_bytes % rb || ((uintptr_t)p.frames % 16) ||
      p.payload_bytes < 2 || p.payload_off % 4 || p.payload_bytes % 4 || p.header_bytes % 4 || p.frame_bytes % 4)
    return;
  const uint64_t fr0 = p.payload_off / p.payload_bytes;
  const uint64_t rel0 = p.payload_off - fr0 * p.payload_bytes;
  if (rel0 + (uint64_t)(nb - 1) * pl.block_stride_bytes + pl.block_payload_bytes >= (1ull << 32)) return;
  KParams q = p;
  q.frames = p.frames + fr0 * p.frame_bytes;
  q.rel0 = (uint32_t)rel0;
  set_fastdiv(q);
  q.stg_out = h->stg;
  ProfScope ps(h, s, KID_K0, (double)nb * (double)pl.block_payload_bytes * (1.0 + (double)p.frame_bytes / p.payload_bytes));
  const dim3 grid((pl.r / 64) * (pl.c / 256), nb);
  const bool wide = !(rel0 % 16 || p.payload_bytes % 16 || p.header_bytes % 16 || p.frame_bytes % 16);
  select_k0_stage(rb, wide, [&](auto kern, const KSel& a) { launch_sel(h, kern, grid, a, s, q); });
  h->stg_ready = true;
}
bool launch_k1_fast(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  if (!pl.fast_k1_log2m) return false;
  const uint32_t rb = (uint32_t)(pl.fast_k1_wave ? pl.fast_k1_g : pl.g) / 2;   // input bytes per row piece: alignment of every piece
  if (p.payload_off % rb || p.payload_bytes % rb || p.header_bytes % rb || p.frame_bytes % rb ||
      ((uintptr_t)p.frames % 16))
    return false;
  if (pl.fast_k1_wave) {
    // launch-relative 32-bit addressing: frames pointer moved to the frame holding block 0
    if (p.payload_bytes < 2) return false;
    const uint64_t fr0 = p.payload_off / p.payload_bytes;
    const uint64_t rel0 = p.payload_off - fr0 * p.payload_bytes;
    if (rel0 + (uint64_t)nb * pl.block_payload_bytes >= (1ull << 32)) return false;
    KParams q = p;
    q.frames = p.frames + fr0 * p.frame_bytes;
    q.rel0 = (uint32_t)rel0;
    set_fastdiv(q);
    if (h->stg_ready) q.stg = h->stg;   // launch_k0_stage has corner-turned this batch
    h->stg_ready = false;
    if (p.fbad) {   // flagged frames: the staged wave K1 masks them
      if (!q.stg || k1_wave_lds(pl, true) > h->lds_limit) return false;
      q.fbad_frame0 = p.fbad_frame0 + fr0;
    }
    q.tile_major = p.tile_major = pl.spill_tile_major;   // 2 (R = 2048, paired branches) or 8 (R = 8192) or 0 (K2 of this batch reads what this launch writes)
    return launch_k1_wave(h, q, nb, s, h->lane_cus);
  }
  p.tile_major = pl.spill_tile_major == 8 ? 8 : 0;   // (K2 of this batch reads what this launch writes)
  KParams q = p;
  if (h->stg_ready) q.stg = h->stg;   // launch_k0_stage has corner-turned this batch
  h->stg_ready = false;
  {   // launch-relative 32-bit addressing where the batch fits (else the kernel divides in 64 bits)
    const uint64_t fr0 = p.payload_off / p.payload_bytes;
    const uint64_t rel0 = p.payload_off - fr0 * p.payload_bytes;
    const uint64_t span = rel0 + (uint64_t)(nb - 1) * pl.block_stride_bytes + pl.block_payload_bytes;
    if (p.payload_bytes >= 2 && span < (1ull << 32)) {
      q.frames = p.frames + fr0 * p.frame_bytes;
      q.rel0 = (uint32_t)rel0;
      q.payload_off = rel0;
      set_fastdiv(q);
    } else {
      q.div_magic = 0;
    }
  }
  return select_k1_fast(pl, [&](auto kern, const KSel& a) { launch_sel(h, kern, dim3(pl.c2 / pl.g, nb), a, s, q); });
}
bool launch_k2_fast(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  if (pl.fast_k2_lane) {
    if (p.tile_major) return false;
    const dim3 grid((unsigned)((uint64_t)pl.r * nb * pl.fast_k2_lane / 256));
    return select_k2_lane(pl, p.pol_mode, [&](auto kern, const KSel& a) { launch_sel(h, kern, grid, a, s, p); });
  }
  if (const PrivLaunch pv = priv_launch(h, p, nb); pv.grid) {
    p.nblk = nb;
    if (!pv.sums) p.stat_partial = nullptr;
    if (!p.stat_partial) p.stat_first = 0;
    p.stat_slices = p.stat_partial ? h->stat_slices : nullptr;   // (launch_back has checked that the launch's flushes fit the slots)
    p.stat_slots = p.stat_partial ? h->stat_slots : 0u;
    const dim3 grid(pv.grid);
    return select_k2_priv(pl, p.pol_mode, p.out_mode, [&](auto kern, const KSel& a) { launch_sel(h, kern, grid, a, s, p); });
  }
  if (p.out_mode == FRBCH_OUT_STATS) return false;   // (only frbch_k2_priv has a statistics-only form: the engine asks for it nowhere else)
  if (!pl.fast_k2_wave && pl.fast_k2_log2m != 5) return false;   // (the barrier K2: 2C = 8192 only)
  // tscrunch beyond the kernel's tile: rows of its largest tile into the scratch buffer (q), then the sums (p)
  // (the barrier K2 so with four products at 2C = 8192: two-sample rows)
  KParams q = p;
  if (pl.k2_two_stage) {
    q.tscr = pl.k2_stage1_tscr;
    q.out_mode = FRBCH_OUT_FLOAT_POWER;
    q.power_out = h->scr2;
    q.row0 = 0;
    q.stat_partial = nullptr;
  }
  KParams& k = pl.k2_two_stage ? q : p;
  if (pl.fast_k2_wave) {
    if (!launch_k2_wave(h, k, nb, s, h->cfg.flags)) return false;
  } else {
    select_k2_fast(pl, [&](auto kern, const KSel& a) {   // a workgroup of 1024 threads takes two time samples, or the tscrunch group
      launch_sel(h, kern, dim3(pl.r / (a.nt == 512 ? 1 : std::max(2, k.tscr)), nb), a, s, k);
    });
  }
  if (pl.k2_two_stage) {
    p.scr_in = h->scr2;
    p.scr_fact = (uint32_t)pl.k2_two_stage;
    p.scr_rows = (uint64_t)nb * pl.rows_per_block;
    p.stat_partial = nullptr;
    const uint64_t groups = p.scr_rows * (uint64_t)(pl.ncol / 4);
    const unsigned gx = (unsigned)std::min<uint64_t>((groups + 255) / 256, 8192);
    if (h->profiling) note_launch(h, "frbch_k2_scrunch", gx, 1);
    hipLaunchKernelGGL(fast::frbch_k2_scrunch, dim3(gx), dim3(256), 0, s, p);
  }
  return true;
}
bool launch_k2c_fast(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  if (!pl.coh_fast_c) return false;
  const int tt = 1024 / (16 << pl.coh_fast_c);
  // a workgroup keeps its positions (and their kernel factors, in registers) and walks the blocks of the launch; enough workgroups
  // for a few rounds per CU, else the block index strides too
  p.nblk = nb;
  const uint32_t ntile = (uint32_t)(pl.r / tt);
  const uint32_t want = 4u * (uint32_t)std::max(1, h->lane_ncu);
  const uint32_t gy = std::max<uint32_t>(1, std::min<uint32_t>(nb, (want + ntile - 1) / ntile));
  return select_k2c_fast(pl, [&](auto kern, const KSel& a) { launch_sel(h, kern, dim3(ntile, gy), a, s, p); });
}
bool launch_k3_fast(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  if (!pl.coh_fast_r || !h->coh_order_m) return false;
  if (k3_wave_planned(pl)) {   // persistent over the (block, channel) tiles, next tile prefetched piecewise
    const uint64_t ntiles = (uint64_t)nb * pl.c;
    return select_k3_fast(pl, [&](auto kern, const KSel& a) {
      p.nblk = nb;
      launch_sel(h, kern, dim3((unsigned)std::min<uint64_t>(ntiles, kK3WaveWgs)), a, s, p);
    });
  }
  const int np = pl.coh_nt / (16 << pl.coh_fast_r) / 2;
  return select_k3_fast(pl, [&](auto kern, const KSel& a) { launch_sel(h, kern, dim3(pl.c / np, nb), a, s, p); });
}

// =============================================================================================
// Set-up of the register-pass kernels of the handle's plan: tables, and -- through the selectors, once for every value the
// per-launch inputs can take on this handle -- dynamic-LDS limits and the names of the timing slots.  (The product mode is fixed
// for the life of a handle: base_params copies it from the configuration.)
// =============================================================================================
template <class K>
int allow_lds(frbch_handle* h, K kern, size_t bytes) {
  CHECK_DEV(h, dev_allow_lds(kern, bytes), "LDS size (fast kernel)");
  return FRBCH_OK;
}
int upload_cf(frbch_handle* h, cf** dst, const std::vector<float>& xy) {
  CHECK_DEV(h, dev_malloc((void**)dst, xy.size() * sizeof(float)), "hipMalloc(fast tables)");
  CHECK_DEV(h, dev_h2d(*dst, xy.data(), xy.size() * sizeof(float), h->stream), "upload fast tables");
  CHECK_DEV(h, dev_sync(h->stream), "sync");
  return FRBCH_OK;
}
void fft_tables(int len, std::vector<float>* tw1, std::vector<float>* tw2) {
  const int tps = len / 16, m = len / 256;
  tw1->resize(2 * (size_t)len);
  for (int ka = 0; ka < 16; ++ka)
    for (int q = 0; q < tps; ++q) {
      const double a = -2.0 * M_PI * (double)(((uint64_t)q * ka) % len) / len;
      (*tw1)[2 * ((size_t)ka * tps + q)] = (float)cos(a);
      (*tw1)[2 * ((size_t)ka * tps + q) + 1] = (float)sin(a);
    }
  tw2->resize(2 * (size_t)m * 16);
  for (int kb = 0; kb < m; ++kb)
    for (int c = 0; c < 16; ++c) {
      const double a = -2.0 * M_PI * (double)((c * kb) % tps) / tps;
      (*tw2)[2 * (kb * 16 + c)] = (float)cos(a);
      (*tw2)[2 * (kb * 16 + c) + 1] = (float)sin(a);
    }
}
int setup_fast(frbch_handle* h) {
  const Plan& pl = h->pl;
  const int pol = h->cfg.pol_mode;
  int rc = FRBCH_OK;
  std::vector<float> t1, t2;
  // the visitor of set-up: the kernel may use its LDS, and timing slot `kid` reports under its name
  auto plan_for = [&](int kid) {
    return [&rc, h, kid](auto kern, const KSel& a) {
      if (!rc) rc = allow_lds(h, kern, a.lds);
      h->kname[kid] = a.name();
    };
  };
  if (pl.fast_k1_log2m) {
    fft_tables(pl.r, &t1, &t2);
    if ((rc = upload_cf(h, &h->ftw1_r, t1)) || (rc = upload_cf(h, &h->ftw2_r, t2))) return rc;
    const int tps = pl.r / 16;
    std::vector<float> d1(2 * (size_t)pl.c2 * 16), d2(2 * (size_t)pl.c2 * tps);
    for (int n1 = 0; n1 < pl.c2; ++n1) {
      for (int kc = 0; kc < 16; ++kc) {
        const double a = -2.0 * M_PI * (double)((uint64_t)n1 * kc) / (16.0 * pl.c2);
        d1[2 * ((size_t)n1 * 16 + kc)] = (float)cos(a);
        d1[2 * ((size_t)n1 * 16 + kc) + 1] = (float)sin(a);
      }
      for (int k0 = 0; k0 < tps; ++k0) {
        const double a = -2.0 * M_PI * (double)((uint64_t)n1 * k0) / (double)pl.n;
        d2[2 * ((size_t)n1 * tps + k0)] = (float)cos(a);
        d2[2 * ((size_t)n1 * tps + k0) + 1] = (float)sin(a);
      }
    }
    if ((rc = upload_cf(h, &h->td1, d1)) || (rc = upload_cf(h, &h->td2, d2))) return rc;
    CHECK_DEV(h, dev_malloc((void**)&h->stg, (size_t)pl.maxb * pl.block_payload_bytes), "hipMalloc(staged payload)");
    if (pl.fast_k1_wave) {
      select_k1_wave(pl, false, false, plan_for(KID_K1));
      select_k1_wave(pl, true, false, plan_for(KID_K1));
      if (k1_wave_lds(pl, true) <= h->lds_limit) select_k1_wave(pl, true, true, plan_for(KID_K1));   // (else launch_k1_fast declines masked batches)
    } else {
      select_k1_fast(pl, plan_for(KID_K1));
    }
    if (rc) return rc;
  }
  if (pl.coh_fast_c || pl.fast_k2_log2m || pl.fast_k2_m1) {   // the 2C-point tables (2C = 256: wave-private K2 only, Kc stays generic)
    fft_tables(pl.c2, &t1, &t2);
    if ((rc = upload_cf(h, &h->ftw1_c, t1)) || (rc = upload_cf(h, &h->ftw2_c, t2))) return rc;
  }
  select_k2c_fast(pl, plan_for(KID_K2));
  select_k3_fast(pl, plan_for(KID_K3));
  if (pl.coherent && k4_fast_planned(pl, h->cfg.flags)) h->kname[KID_K4] = "frbch_k4_fast";
  select_kc_fast(pl, plan_for(KID_KC));
  if (kc_lane_planned(pl)) h->kname[KID_KC] = "frbch_kc_lane";
  if (pl.fast_k2_wave) {
    for (const bool cols : {false, true}) select_k2_wave(pl, pol, cols, plan_for(KID_K2));
  } else {
    select_k2_fast(pl, plan_for(KID_K2));
  }
  // (KID_K2 keeps frbch_k2_wave's name beside frbch_k2_priv: float rows of four products and fallen-back launches run it)
  for (const int out_mode : {(int)FRBCH_OUT_CODES, (int)FRBCH_OUT_FLOAT_POWER, (int)FRBCH_OUT_STATS})
    select_k2_priv(pl, pol, out_mode, plan_for(out_mode == FRBCH_OUT_STATS ? KID_K2S : KID_K2P));
  select_k2_lane(pl, pol, plan_for(KID_K2));
  return rc;
}
#else
bool launch_kc_fast(frbch_handle*, KParams&, uint32_t, dev_stream_t) { return false; }
bool launch_k1_fast(frbch_handle*, KParams&, uint32_t, dev_stream_t) { return false; }
bool launch_k2_fast(frbch_handle*, KParams&, uint32_t, dev_stream_t) { return false; }
void launch_k0_stage(frbch_handle*, const KParams&, uint32_t, dev_stream_t) {}
bool launch_k2c_fast(frbch_handle*, KParams&, uint32_t, dev_stream_t) { return false; }
bool launch_k3_fast(frbch_handle*, KParams&, uint32_t, dev_stream_t) { return false; }
int setup_fast(frbch_handle*) { return FRBCH_OK; }
#endif

// dedispersion kernel table in the fine-bin order of the K1 / K3 pair in use (order_m = 0: generic, M: register passes)
int build_chirp(frbch_handle* h, int order_m) {
  const Plan& pl = h->pl;
  ChirpParams cp;
  memset(&cp, 0, sizeof cp);
  cp.chirp = h->chirp;
  cp.c = pl.c; cp.c2 = pl.c2; cp.r = pl.r; cp.log2_r = pl.log2_r;
  cp.usb = h->cfg.bw_mhz > 0 ? 1 : 0;
  cp.order_m = order_m;
  const double abw = fabs(h->cfg.bw_mhz);
  cp.band_edge_mhz = cp.usb ? h->cfg.freq_mhz - abw / 2.0 : h->cfg.freq_mhz + abw / 2.0;
  cp.df_mhz = abw / pl.c;
  cp.dm_over_k = h->cfg.dm / kDmDispersion;
  REC_LAUNCH(h, frbch_chirp_build, (pl.n + 255) / 256, 1, 256, 0, h->stream, cp);
  CHECK_DEV(h, dev_check_launch(), "launch chirp build");
  CHECK_DEV(h, dev_sync(h->stream), "sync");
  h->coh_order_m = order_m;
  return FRBCH_OK;
}

// dynamic level setting: the low-state counts of the windows covering the launch's first `nsamples` samples (a multiple of the window)
int launch_dls_count(frbch_handle* h, KParams& p, uint64_t nsamples, dev_stream_t s) {
  const Plan& pl = h->pl;
  const uint64_t nwin = nsamples >> pl.dls_lg_ns;
  if (!h->dls_tab || (nwin << pl.dls_lg_ns) != nsamples) return fail(h, FRBCH_E_ARG, "dynamic level setting: the sample count is not a multiple of the window");
  if (nwin > h->dls_cap) {
    dev_free(h->dls_nlow);
    h->dls_nlow = nullptr;
    h->dls_cap = 0;
    CHECK_DEV(h, dev_malloc((void**)&h->dls_nlow, nwin * sizeof(uint32_t)), "hipMalloc(window counts)");
    h->dls_cap = nwin;
  }
  p.dls_tab = h->dls_tab;
  p.dls_nlow = h->dls_nlow;
  p.dls_lg_ns = pl.dls_lg_ns;
  KParams q = p;
  q.row0 = nwin;
  REC_LAUNCH(h, frbch_dls_count, (nwin + 3) / 4, 1, 256, 2048, s, q);
  CHECK_DEV(h, dev_check_launch(), "launch window counts");
  return FRBCH_OK;
}

// K0 + K1 + Kc over nb blocks: frames -> spill, P0
int launch_front(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  p.tile_major = 0;   // set by the K1 that writes that layout
  if (pl.dls_lg_ns) {
    const int rc = launch_dls_count(h, p, ((uint64_t)nb - 1) * pl.hop + pl.n, s);
    if (rc) return rc;
  }
  {
    // blocks that touch invalid / filler frames: the staged wave K1 reads their samples as 0 through a flag per row (MSK);
    // where it cannot run (R = 8192, unaligned input, the barrier K1) the generic K1 tests the bitmap per sample
    const bool masked = p.fbad != nullptr;
    if (!masked || pl.fast_k1_wave) launch_k0_stage(h, p, nb, s);
    const double bytes = (double)nb * ((double)pl.block_payload_bytes * p.frame_bytes / p.payload_bytes +
                                       (double)pl.n * 8.0 + (double)pl.c2 * 8.0);
    ProfScope ps(h, s, KID_K1, bytes);
    bool done = false;
    if (masked && !(pl.fast_k1_wave && (!pl.coherent || h->coh_order_m) && (done = launch_k1_fast(h, p, nb, s)))) {
      h->stg_ready = false;
      if (pl.coherent && h->coh_order_m) {   // from here on the generic K1 / K3 and their bin order
        const int rc = build_chirp(h, 0);
        if (rc) return rc;
      }
    } else if (masked) {
      // (the masked wave K1 ran)
    } else if (!pl.coherent) done = launch_k1_fast(h, p, nb, s);
    else if (h->coh_order_m) {
      done = launch_k1_fast(h, p, nb, s);
      if (!done) {   // a start offset the register kernel cannot gather: from here on the generic K1 / K3 and their bin order
        const int rc = build_chirp(h, 0);
        if (rc) return rc;
      }
    }
    if (!done) {
      REC_LAUNCH(h, frbch_k1_branch, pl.c2 / pl.g, nb, pl.nthreads, pl.k1_lds, s, p);
      // the timing report says so when a launch of a handle planned for a register-pass K1 fell back to the generic one
      if (!h->kname[KID_K1].empty() && h->kname[KID_K1].find(kKernelNames[KID_K1]) == std::string::npos)
        h->kname[KID_K1] += std::string("+") + kKernelNames[KID_K1];
    }
  }
  if (!pl.coherent) {
    ProfScope ps(h, s, KID_KC, (double)nb * pl.c2 * 16.0);
    if (!launch_kc_fast(h, p, nb, s)) REC_LAUNCH(h, frbch_kc_dcfix, 1, nb, pl.nthreads, pl.kc_lds, s, p);
  }
  CHECK_DEV(h, dev_check_launch(), "launch K1/Kc");
  return FRBCH_OK;
}

int launch_back(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  const int tile_t = std::max(pl.tt, pl.tscr);
  const double out_b = p.out_mode == FRBCH_OUT_FLOAT_POWER ? (double)pl.ncol * 4.0 : (double)pl.row_bytes;
  const double bytes = (double)nb * ((double)pl.n * 8.0 + (double)pl.rows_per_block * out_b);
#ifndef FRBCH_NO_FAST
  const bool k3_sums = k3_wave_planned(pl) && h->coh_order_m != 0;   // (the generic K3 of a fallen-back launch does not sum)
#else
  const bool k3_sums = false;
#endif
  if ((!k2_wave_planned(pl) || pl.coherent) && !k3_sums) p.stat_partial = nullptr;   // only the wave-private K2 / K3 sum while they write
#ifndef FRBCH_NO_FAST
  // frbch_k2_priv writes one slot of fp32 sums per flush: a launch with more flushes per workgroup than ensure_partial allocated
  // slots (more blocks than the plan's batch) is refused here, it never runs with an index that leaves the buffer
  if (const PrivLaunch pv = priv_launch(h, p, nb); pv.sums && (!h->stat_slices || priv_stat_slots(pl, nb, pv.grid) > h->stat_slots))
    return fail(h, FRBCH_E_CAPACITY, "frbch_k2_priv: " + std::to_string(priv_stat_slots(pl, nb, pv.grid)) + " flushes per workgroup, " +
                                         std::to_string(h->stat_slots) + " slots of rescale sums allocated");
#endif
  if (p.out_mode == FRBCH_OUT_STATS) {   // first pass of the two-pass rescale: the spill is read, nothing but the sums is written
    ProfScope ps(h, s, KID_K2S, (double)nb * (double)pl.n * 8.0);
    if (!launch_k2_fast(h, p, nb, s)) return fail(h, FRBCH_E_STATE, "statistics-only K2 pass without frbch_k2_priv");
    CHECK_DEV(h, dev_check_launch(), "launch K2 (statistics pass)");
    return FRBCH_OK;
  }
  if (pl.coherent) {   // K2c (branches -> channels, x kernel), K3 (back to time, detect), K4 (time-major rows)
    {
      ProfScope ps(h, s, KID_K2, ((double)nb * 16.0 + (pl.coh_fast_c ? 1.0 : (double)nb) * 8.0) * (double)pl.n);   // the register K2c reads the kernel table once per launch
      if (!launch_k2c_fast(h, p, nb, s)) REC_LAUNCH(h, frbch_k2c_chirp, pl.r / pl.tt, nb, pl.nthreads, pl.k2_lds, s, p);
    }
    {
      ProfScope ps(h, s, KID_K3, (double)nb * ((double)pl.n * 8.0 + (double)pl.rows_per_block * pl.ncol * 4.0));
      if (!launch_k3_fast(h, p, nb, s)) REC_LAUNCH(h, frbch_k3_dedisp, pl.c, nb, pl.nthreads, pl.k3_lds, s, p);
    }
    {
      ProfScope ps(h, s, KID_K4, (double)nb * (double)pl.rows_per_block * (pl.ncol * 4.0 + out_b));
      const int tc = pl.ncol < 64 ? (int)pl.ncol : 64;
      const int gx = (int)((pl.rows_per_block + 63) / 64) * (int)(pl.ncol / tc);
#ifndef FRBCH_NO_FAST
      if (k4_fast_planned(pl, h->cfg.flags)) {
        if (h->profiling) note_launch(h, "frbch_k4_fast", gx, nb);
        hipLaunchKernelGGL(fast::frbch_k4_fast, dim3(gx, nb), dim3(256), 0, s, p);
      } else
#endif
      REC_LAUNCH(h, frbch_k4_out, gx, nb, pl.nthreads, pl.k4_lds, s, p);
    }
    CHECK_DEV(h, dev_check_launch(), "launch K2c/K3/K4");
    return FRBCH_OK;
  }
#ifndef FRBCH_NO_FAST
  const int kid = priv_takes(pl, p, h->priv_grid) ? KID_K2P : KID_K2;   // the two K2 families of 2C = 2048 report separately
#else
  const int kid = KID_K2;
#endif
  ProfScope ps(h, s, kid, bytes);
  if (!launch_k2_fast(h, p, nb, s)) REC_LAUNCH(h, frbch_k2_chan, pl.r / tile_t, nb, pl.nthreads, pl.k2_lds, s, p);
  CHECK_DEV(h, dev_check_launch(), "launch K2");
  return FRBCH_OK;
}

// the table of partial rescale sums (separate statistics pass: partial_chunks rows; sums fused into K2: fused_chunks rows)
int ensure_partial(frbch_handle* h) {
  if (h->partial) return FRBCH_OK;
  const Plan& pl = h->pl;
  // rows of partial sums of the separate statistics pass = its workgroups (x threads sharing a column group).  Narrow rows (32 .. 128
  // columns: the online chain's channel counts) need more of them: 2048 rows left 256 single-wave workgroups for the whole chip and the
  // reduction took 11 % of a 32-channel step (0.45 ms for 40 MB); the table stays within 8 MB
  h->partial_chunks = (int)std::min<uint64_t>(32768, std::max<uint64_t>(2048, (8ull << 20) / (pl.ncol * 16)));
  h->fused_chunks = 0;
#ifndef FRBCH_NO_FAST
  h->fused_chunks = fused_stat_chunks(pl, h->cfg.flags, h->cfg.pol_mode, h->priv_grid);   // kFlagSeparateStats forces the separate statistics pass
#endif
  const size_t chunks = (size_t)std::max(h->partial_chunks, h->fused_chunks);
  CHECK_DEV(h, dev_malloc((void**)&h->partial, chunks * pl.ncol * 2 * sizeof(double)), "hipMalloc(partials)");
#ifndef FRBCH_NO_FAST
  // ... and the slices frbch_k2_priv flushes its fp32 sums into, one slot per flush of the longest launch (maxb blocks): at
  // config 3 512 workgroups x 19 slots x 32 KB = 319 MB per handle (beside a 5.1-GB spill)
  h->stat_slots = 0;
  if (pl.fast_k2_priv && h->priv_grid > 0 && !pol_mode_no_sums(h->cfg.pol_mode) && !(h->cfg.flags & kFlagSeparateStats)) {
    h->stat_slots = priv_stat_slots(pl, (uint32_t)pl.maxb, (unsigned)h->priv_grid);
    CHECK_DEV(h, dev_malloc((void**)&h->stat_slices, (size_t)h->priv_grid * h->stat_slots * pl.ncol * 2 * sizeof(float)), "hipMalloc(slices of partials)");
  }
#endif
  return FRBCH_OK;
}
// A rescale interval starts with the K2 launch of `p` (out_mode, tile_major and stat_partial set).  The kernels add into the table, so
// it is cleared first -- except for frbch_k2_priv, whose workgroups own a row each and start their sums from 0.0, not from the row, when told so
// (KParams::stat_first): no memset in front of the pass, and frbch_stats_final reads those rows only (fused_live; the rows behind
// them would be zeros: the sums are the same bit for bit, every column is added up in the same order).
int clear_partial(frbch_handle* h, KParams& p, uint32_t nb, dev_stream_t s) {
  const Plan& pl = h->pl;
  int own = 0;   // rows this launch writes without reading them first
#ifndef FRBCH_NO_FAST
  if (const PrivLaunch pv = priv_launch(h, p, nb); pv.sums) own = priv_stat_chunks(pl, (int)pv.grid);   // (the launch launch_k2_fast makes of p)
#endif
  p.stat_first = own ? 1u : 0u;
  h->fused_live = own;
  return own ? FRBCH_OK : extend_partial(h, s);
}
// ... and goes on with another launch that adds into the table -- more workgroups, or the other K2 family: the rows nobody has
// written yet are cleared now (never, when the interval ends with the launch it started with)
int extend_partial(frbch_handle* h, dev_stream_t s) {
  if (h->fused_live >= h->fused_chunks) return FRBCH_OK;
  const size_t row_bytes = (size_t)h->pl.ncol * 2 * sizeof(double);
  if (dev_memset((char*)h->partial + (size_t)h->fused_live * row_bytes, 0, (size_t)(h->fused_chunks - h->fused_live) * row_bytes, s) != 0)
    return fail(h, FRBCH_E_DEVICE, "clear partial sums");
  h->fused_live = h->fused_chunks;
  return FRBCH_OK;
}
// the float rows of a buffered rescale interval (allocated on first use: a scan whose first interval takes the two-pass form never needs it)
int ensure_powbuf(frbch_handle* h) {
  const int rc = ensure_partial(h);
  if (rc || h->powbuf) return rc;
  const Plan& pl = h->pl;
  h->pow_cap_rows = pl.interval_rows + (uint64_t)pl.maxb * pl.rows_per_block;
  CHECK_DEV(h, dev_malloc((void**)&h->powbuf, h->pow_cap_rows * pl.ncol * sizeof(float)), "hipMalloc(power buffer)");
  return FRBCH_OK;
}

// columns per workgroup of frbch_stats_final: eight (whole lines), two when eight would leave fewer than 128 workgroups
static int stat_final_cpw(const Plan& pl) { return pl.ncol < 1024 ? 2 : 8; }

int run_stats(frbch_handle* h, uint64_t rows, dev_stream_t s) {
  const Plan& pl = h->pl;
  StatParams sp;
  memset(&sp, 0, sizeof sp);
  if (h->fused_valid && h->fused_chunks && h->fused_rows == rows) {   // K2 already summed these rows: reduce only
    sp.partial = h->partial;
    sp.rows = rows;
    sp.ncol = (int)pl.ncol;
    sp.c = pl.c;
    sp.nif = pl.nif;
    sp.flip = pl.flip;
    sp.nchunk = h->fused_live;
    sp.cpw = stat_final_cpw(pl);
    sp.offset = h->offset;
    sp.scale = h->scale;
    ProfScope ps(h, s, KID_STATS, (double)h->fused_live * pl.ncol * 16.0);
    REC_LAUNCH(h, frbch_stats_final, (int)((pl.ncol + sp.cpw - 1) / sp.cpw), 1, 256, 256 * 2 * sizeof(double), s, sp);
    CHECK_DEV(h, dev_check_launch(), "launch stats (final)");
    return FRBCH_OK;
  }
  if (!h->powbuf) return fail(h, FRBCH_E_STATE, "rescale statistics: neither fused sums nor buffered rows");
  sp.power = h->powbuf;
  sp.partial = h->partial;
  sp.rows = rows;
  sp.ncol = (int)pl.ncol;
  sp.c = pl.c;
  sp.nif = pl.nif;
  sp.flip = pl.flip;
  // narrow rows (fewer than 64 column groups): the threads of a 64-thread workgroup share the column groups and split the rows
  const int cg = (int)(pl.ncol / 4);
  sp.rsplit = (cg < 64 && 64 % cg == 0) ? 64 / cg : 1;
  sp.nchunk = (int)std::min<uint64_t>((uint64_t)h->partial_chunks / sp.rsplit, std::max<uint64_t>(1, rows / (32 * sp.rsplit)));
  if (sp.nchunk < 1) sp.nchunk = 1;
  sp.rows_per_chunk = (rows + sp.nchunk - 1) / sp.nchunk;
  sp.nchunk = (int)((rows + sp.rows_per_chunk - 1) / sp.rows_per_chunk);
  sp.cpw = stat_final_cpw(pl);
  sp.offset = h->offset;
  sp.scale = h->scale;
  const int gx4 = (int)((pl.ncol / 4 * sp.rsplit + 63) / 64);
  ProfScope ps(h, s, KID_STATS, (double)rows * pl.ncol * 4.0);
  REC_LAUNCH(h, frbch_stats_partial, gx4, sp.nchunk, 64, 0, s, sp);
  sp.nchunk *= sp.rsplit;          // rows of partial sums the final reduction adds up (fixed order: deterministic)
  REC_LAUNCH(h, frbch_stats_final, (int)((pl.ncol + sp.cpw - 1) / sp.cpw), 1, 256, 256 * 2 * sizeof(double), s, sp);
  CHECK_DEV(h, dev_check_launch(), "launch stats");
  return FRBCH_OK;
}

// Geometry of the lean 8-bit digitiser (frbch_quantise_fast) on `ncu` CUs (0 = the whole chip; negative: |ncu| CUs held by one
// 512-thread workgroup each, see run_quantise): workgroups, threads per workgroup and row phases; false = the generic kernel runs
bool quant_fast_geometry(const frbch_handle* h, int ncu, uint64_t* wgs_out, uint64_t* nthr_out, uint64_t* rp_out) {
  const Plan& pl = h->pl;
  if (h->cfg.nbit_out != 8 || pl.digi_max != 255.0f) return false;
  const uint64_t cg = pl.ncol / 4;
  const bool pow2 = (pl.ncol & (pl.ncol - 1)) == 0 && (pl.c & (pl.c - 1)) == 0;
  if (!pow2 || pl.c < 4 || cg < 8) return false;   // (narrow rows, 32 .. 128 columns: a wave covers several rows -- one contiguous run all the same)
  const bool excl = ncu < 0;
  const uint64_t nthr = excl ? 512 : 256;
  const uint64_t rp = excl ? (uint64_t)(-ncu) * nthr / cg : (uint64_t)(ncu > 0 ? ncu : 256) * 3 * 256 / cg;
  const uint64_t wgs = rp * cg / nthr;
  const uint64_t pitch = h->out_pitch ? h->out_pitch : (uint64_t)pl.c;
  if (!wgs || wgs * nthr != rp * cg || pitch % 4 || rp * (uint64_t)pl.nif * pitch >= (1ull << 31) || rp * pl.ncol * 4 >= (1ull << 31)) return false;
  *wgs_out = wgs;
  *nthr_out = nthr;
  *rp_out = rp;
  return true;
}

int run_quantise(frbch_handle* h, uint64_t rows, uint8_t* dst, dev_stream_t s, int ncu) {
  const Plan& pl = h->pl;
  QuantParams qp;
  memset(&qp, 0, sizeof qp);
  qp.power = h->powbuf;
  qp.out = dst;
  qp.rows = rows;
  qp.ncol = (int)pl.ncol;
  qp.c = pl.c;
  qp.nif = pl.nif;
  qp.flip = pl.flip;
  qp.nbit = h->cfg.nbit_out;
  qp.offset = h->offset;
  qp.scale = h->scale;
  qp.digi_mean = pl.digi_mean;
  qp.digi_scale = pl.digi_scale;
  qp.digi_max = pl.digi_max;
  const uint64_t total = rows * pl.ncol / 4;
  // grid-stride, 4 groups per thread per trip, up to 32 workgroups per CU of the stream it runs on.  (A bare 16-B-in / 4-B-out
  // stream reads fastest with 8 waves per CU, tools/micro/stream_cus; this kernel carries ~60 VALU instructions per group --
  // index arithmetic, rescale, four digitiser chains -- and needs the waves: 1 / 2 / 4 / 8 / 32 workgroups per CU measured
  // 2.8 / 1.76 / 1.41 / 1.59 / 1.28 ms per 6.4 GB, profiles/r03_overlap_sweep_quantise_lane.txt)
  const uint64_t gx = std::min<uint64_t>((total + 256 * 4 - 1) / (256 * 4), (uint64_t)(ncu != 0 ? std::abs(ncu) : 256) * 32);
  qp.grid_x = (uint32_t)std::max<uint64_t>(1, gx);
  qp.log2_c = 0;
  while ((1 << qp.log2_c) < pl.c) ++qp.log2_c;
  qp.log2_ncol = 0;
  while ((1ull << qp.log2_ncol) < pl.ncol) ++qp.log2_ncol;
  qp.pitch = h->out_pitch ? h->out_pitch : (uint64_t)pl.c;
  ProfScope ps(h, s, KID_QUANT, (double)rows * (pl.ncol * 4.0 + pl.row_bytes));
#ifndef FRBCH_NO_FAST
  {
    // 8-bit codes of power-of-two rows: the lean stream (frbch_quantise_fast): every thread one column group, threads = row
    // phases x column groups.  The loads a thread has in flight are `rphases` rows apart, and the HBM address hash does not like
    // every distance: 3 workgroups per CU (four products at 1024 channels: 192 phases, the loads 3 MiB apart) measured 9.1 ms per
    // 8 IFs of config 3, 1 / 2 / 4 / 6 / 8 / 16 per CU 9.7 / 10.6 / 11.1 / 9.5 / 11.1 / 10.4, odd phase counts 63 / 95 / 127 / 191 /
    // 193 / 255 / 383 / 511: 10.1 / 9.5 / 10.5 / 9.4 / 10.1 / 11.2 / 10.1 / 11.8 (generic kernel: 9.9)
    // ncu < 0: |ncu| workgroups of 512 threads, each reserving more than half the LDS: one per CU, and no wave K1 workgroup (148 KB)
    // beside it -- the digitiser holds |ncu| CUs to itself on a plain stream while the next IF's K1 runs on the others.  (16 loads
    // in flight per thread or 1024 threads per workgroup: the same time; the two kernels together move 5.2 TB/s.)
    const bool excl = ncu < 0;
    uint64_t wgs = 0, nthr = 0, rp = 0;
    if (quant_fast_geometry(h, ncu, &wgs, &nthr, &rp)) {
      qp.grid_x = (uint32_t)wgs;
      qp.rphases = (uint32_t)rp;
      h->kname[KID_QUANT] = "frbch_quantise_fast<8>";
      if (excl) {
        constexpr size_t kHold = 84 * 1024;
        if (!h->quant_lds_allowed) {   // (per handle: the attribute belongs to the handle's device)
          CHECK_DEV(h, dev_allow_lds(fast::frbch_quantise_fast<8, 512>, kHold), "LDS size digitiser");
          h->quant_lds_allowed = true;
        }
        if (h->profiling) note_launch(h, "frbch_quantise_fast<8, 512>", qp.grid_x, 1);
        hipLaunchKernelGGL((fast::frbch_quantise_fast<8, 512>), dim3(qp.grid_x), dim3(512), kHold, s, qp);
      } else {
        if (h->profiling) note_launch(h, "frbch_quantise_fast<8, 256>", qp.grid_x, 1);
        hipLaunchKernelGGL((fast::frbch_quantise_fast<8, 256>), dim3(qp.grid_x), dim3(256), 0, s, qp);
      }
      CHECK_DEV(h, dev_check_launch(), "launch quantise");
      return FRBCH_OK;
    }
  }
#endif
  REC_LAUNCH(h, frbch_quantise, qp.grid_x, 1, 256, 0, s, qp);
  CHECK_DEV(h, dev_check_launch(), "launch quantise");
  return FRBCH_OK;
}

// bytes between the starts of consecutive output rows at d_out, and bytes `rows` rows span from d_out
// (packed rows, or this IF's columns of a wider row buffer: out_pitch values per (row, product) line)
uint64_t out_row_span(const frbch_handle* h) {
  const Plan& pl = h->pl;
  if (!h->out_pitch) return pl.row_bytes;
  const uint64_t bits = pl.row_bytes * 8 / pl.ncol;                 // bits per value
  return h->out_pitch * (uint64_t)pl.nif * bits / 8;
}
uint64_t out_extent(const frbch_handle* h, uint64_t rows) {
  const Plan& pl = h->pl;
  if (!rows) return 0;
  if (!h->out_pitch) return rows * pl.row_bytes;
  const uint64_t bits = pl.row_bytes * 8 / pl.ncol;                 // bits per value
  const uint64_t line = h->out_pitch * bits / 8, seg = (uint64_t)pl.c * bits / 8;
  return (rows * pl.nif - 1) * line + seg;
}


int allow_generic_lds(frbch_handle* h) {
  const Plan& pl = h->pl;
  CHECK_DEV(h, dev_allow_lds(frbch_k1_branch, pl.k1_lds), "LDS size K1");
  CHECK_DEV(h, dev_allow_lds(frbch_k2_chan, pl.k2_lds), "LDS size K2");
  CHECK_DEV(h, dev_allow_lds(frbch_kc_dcfix, pl.kc_lds), "LDS size Kc");
  if (pl.coherent) {
    CHECK_DEV(h, dev_allow_lds(frbch_k2c_chirp, pl.k2_lds), "LDS size K2c");
    CHECK_DEV(h, dev_allow_lds(frbch_k3_dedisp, pl.k3_lds), "LDS size K3");
  }
  return FRBCH_OK;
}

// Everything a handle derives from its plan: LDS limits, tables and timing-slot names of its kernels, the grid of frbch_k2_priv and
// the buffers whose size follows the layout group or the kernel choice.  frbch_open calls it, and the host streaming path again
// when the first frame of a stream makes it plan anew (1-bit samples): what an earlier call allocated is released first.
int apply_plan(frbch_handle* h) {
  const Plan& pl = h->pl;
  cf** const tables[] = {&h->ftw1_r, &h->ftw2_r, &h->ftw1_c, &h->ftw2_c, &h->td1, &h->td2, &h->spill, &h->spill2, &h->chirp};
  for (cf** t : tables) { dev_free(*t); *t = nullptr; }
  dev_free(h->stg); h->stg = nullptr; h->stg_ready = false;
  dev_free(h->scr2); h->scr2 = nullptr;
  dev_free(h->ptmp); h->ptmp = nullptr;
  dev_free(h->partial); h->partial = nullptr;   // (its rows follow the K2 of the plan: ensure_partial sizes it again)
  dev_free(h->stat_slices); h->stat_slices = nullptr;
  h->stat_slots = 0;
  h->partial_chunks = h->fused_chunks = 0;
  h->fused_rows = 0;
  h->fused_valid = false;
  for (std::string& n : h->kname) n.clear();
  h->launch_rec.clear();
  int rc;
  if ((rc = allow_generic_lds(h))) return rc;
  h->priv_grid = pl.fast_k2_priv ? 2 * std::max(1, h->lane_ncu) : 0;   // two 80-KiB workgroups per CU
  if ((rc = setup_fast(h))) return rc;
  CHECK_DEV(h, dev_malloc((void**)&h->spill, (size_t)pl.maxb * (pl.c2 / pl.g) * pl.gs * sizeof(cf)), "hipMalloc(spill)");
#ifndef FRBCH_NO_FAST
  if (pl.k2_two_stage)
    CHECK_DEV(h, dev_malloc((void**)&h->scr2, (size_t)pl.maxb * (pl.r / pl.k2_stage1_tscr) * pl.ncol * sizeof(float)), "hipMalloc(tscrunch scratch)");
#endif
  if (pl.coherent) {
    CHECK_DEV(h, dev_malloc((void**)&h->spill2, (size_t)pl.maxb * pl.n * sizeof(cf)), "hipMalloc(spill2)");
    CHECK_DEV(h, dev_malloc((void**)&h->chirp, (size_t)pl.n * sizeof(cf)), "hipMalloc(chirp)");
    CHECK_DEV(h, dev_malloc((void**)&h->ptmp, (size_t)pl.maxb * pl.rows_per_block * pl.ncol * sizeof(float)), "hipMalloc(ptmp)");
    if ((rc = build_chirp(h, pl.coh_fast_r ? (1 << pl.coh_fast_r) : 0))) return rc;
    if (h->kname[KID_K2].empty()) h->kname[KID_K2] = "frbch_k2c_chirp";   // (the slot's own name is that of the incoherent K2)
  }
  return FRBCH_OK;
}

int fused_chunks_of(const frbch_handle* h) {
#ifndef FRBCH_NO_FAST
  return fused_stat_chunks(h->pl, h->cfg.flags, h->cfg.pol_mode, h->priv_grid);
#else
  (void)h;
  return 0;
#endif
}

// the unpack tap: voltages as the filterbank sees them (A4 in isolation)
int launch_unpack_tap(frbch_handle* h, KParams& p, uint64_t nsamples, int decoder, dev_stream_t s) {
  if (h->pl.dls_lg_ns) {
    if (decoder != 0) return fail(h, FRBCH_E_ARG, "dynamic level setting is decoded by the generic unpack only");
    const int rc = launch_dls_count(h, p, nsamples, s);
    if (rc) return rc;
  }
  if (decoder == 0) {
    REC_LAUNCH(h, frbch_unpack_tap, (nsamples + 255) / 256, 1, 256, 0, s, p);
  } else {
#ifndef FRBCH_NO_FAST
    if (h->profiling) note_launch(h, "frbch_unpack_tap_fast", (nsamples / 2 + 255) / 256, 1);
    hipLaunchKernelGGL(fast::frbch_unpack_tap_fast, dim3((unsigned)((nsamples / 2 + 255) / 256)), dim3(256), 0, s, p);
#else
    return fail(h, FRBCH_E_ARG, "the register kernels are not part of this build");
#endif
  }
  CHECK_DEV(h, dev_check_launch(), "launch unpack tap");
  return FRBCH_OK;
}

}  // namespace frbchi
