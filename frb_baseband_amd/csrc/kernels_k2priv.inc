// frbch_k2_priv -- the across-branch kernel (K2) for 2C = 2048 (1024 channels: BASELINE configs[1] and configs[2]) with ONE
// WAVEFRONT PER TIME SAMPLE and no barrier inside the transform.
//
// What it replaces and why (round 4): frbch_k2_wave<3,4,PM,2> ran 2.1 times the time per transform of the along-branch kernel
// K1 -- seven workgroup barriers per two-sample tile (tile into the LDS, two between the passes of the two waves that share a
// sequence, mirror exchange, image -> power rows, rows consumed), the tile staged through the LDS before the first pass, and a
// register prefetch of the next tile that lives beside the current one.  Here:
//   * a wave owns a whole 2048-point sequence (32 points per lane, two virtual threads) exactly like frbch_k1_wave<3,8,1>:
//     the three register passes exchange through the wave's OWN LDS image, LDS operations of one wave execute in program
//     order, so the transform, the DC repair, the mirror exchange of the two-for-one separation and the detection contain
//     no barrier at all and the eight waves of a workgroup drift apart;
//   * the tile is loaded from the tile-major spill of the paired-branch K1 ([blk][t/2][n1/8][t%2][n1%8]) DIRECTLY in the
//     register layout of the first pass, v[vt][a] = w[a*128 + lane + 64 vt][t]: no staging through the LDS (16 ds_write_b128
//     + 32 ds_read_b64 per sequence less), every load instruction covers eight 64-byte runs; the two waves that read the two
//     halves of the same 128-byte lines (t even / odd) sit in the same workgroup and run the same trip;
//   * the next tile is requested right behind the detection, INTO THE SAME REGISTERS (the current points are dead by then):
//     no second tile's worth of registers, the request is in front of the trip's row stores in the in-order vector-memory
//     queue and has the whole emit phase plus the partner waves' work to land;
//   * a workgroup owns a CONTIGUOUS run of tiles, so the block (and with it the DC-repair row dP, kept in the LDS) changes
//     once or twice per workgroup, not every trip;
//   * two barriers per trip, both outside the transform: power rows complete -> the workgroup-wide emit (a thread owns fixed
//     column groups: frozen offset / scale, or the running rescale sums, stay in its registers) -> rows consumed;
//   * FOUR waves per workgroup (a tile = four time samples) and TWO workgroups per CU, each with exactly half of the 160 KiB of
//     LDS (four images of 2304 cf + dP): the waves of one workgroup are phase-locked by its two barriers -- with one 8-wave
//     workgroup per CU every CU alternated between "all waves wait for their tile" (33 MB requested chip-wide at once: 6.7 us at
//     5 TB/s) and "all waves compute" (4.7 us), nothing overlapped: 10.4 us per trip, K2 1.58 ms per IF, no faster than the
//     kernel it replaces (first version, round 4).  Two independent workgroups per CU, started half a trip apart, compute on one
//     tile while the other's tile streams in.
// Three output modes (template MODE): codes (A9 + A10 with the frozen scale), float power rows with the rescale sums of the
// interval (the buffered path), and STATISTICS ONLY -- the first pass of the two-pass rescale (frbch_stream.cpp: the float rows of
// a first rescale interval are never written; K2 runs twice over the resident spill instead, 18 B per sample behind K1 instead of 26).
// Rescale sums: fp32 in registers over at most 8 trips (32 rows), then STORED, as fp32, into the next slot of the workgroup's own
// slice (KParams::stat_slices: write-only inside the loop, no load, no wait); when the workgroup has run its last trip every
// thread adds the slots of its columns, in ascending order and in fp64, into the workgroup's own row of the fp64 partial table
// (exclusive, bit-reproducible: the chain of adds the in-place flush of rounds 4 and 5 evaluated); frbch_stats_final reduces the
// rows in a fixed order.
//
// grid (<= 2 x CUs), 256 threads, LDS 4 images + dP = 81,920 bytes (two workgroups per CU).  HIP only.

namespace fast {

enum { K2P_CODES = 0, K2P_POWER = 1, K2P_STATS = 2 };
// tunables (the measured best, profiles/NOTES.md round 4)
constexpr uint32_t kK2PFlushMask = 7u;   // rescale sums leave the fp32 registers every 8 trips (32 rows)
constexpr int kK2PQReads = 8;            // 16-byte LDS reads of the emit in flight per thread
#ifndef FI
#define FI __device__ __forceinline__
#endif

constexpr int kK2PrivSeq = 2048 + 2048 / 8;      // cf per image: no skew between the images (nothing reads across them at one address)
constexpr size_t k2_priv_lds_bytes() { return (size_t)4 * kK2PrivSeq * sizeof(cf) + (size_t)1024 * sizeof(cf); }   // = 81,920

template <int PM, int MODE>
__global__ void __launch_bounds__(256, 2) frbch_k2_priv(KParams p) {
  constexpr int LOG2M = 3;
  using GE = GeoW<LOG2M, 1>;
  constexpr int M = GE::M, C2 = GE::L, C = C2 / 2, TPS = GE::TPS, SEQ = kK2PrivSeq, LPS = GE::LPS, VT = GE::VT;
  static_assert(M == 8 && C2 == 2048 && TPS == 128 && LPS == 64 && VT == 2, "written for 2C = 2048");
  constexpr int NW = 4, NT = 64 * NW, TT = NW, ROT = 32 / M;
  constexpr int LG_TT = 2;
  constexpr int NIF = PM >= 4 ? 4 : 1, NCOL = NIF * C, NG = NCOL / 4;   // PM 4: -d4 products, 5: I, Q, U, V formed from them
  constexpr int CGT = NG >= NT ? NG / NT : 1;       // column groups per thread (every row of the tile)
  constexpr int RS = NG >= NT ? 1 : NT / NG;        // ... or row phases: the thread takes rows rph, rph + RS, ...
  constexpr int GL = 8;                             // branches per K1 workgroup = layout group of the tile-major spill
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  cf* dpl = lds + NW * SEQ;                         // [C] dP[C + i] of the current block, swizzled like the power rows

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane;
  cf* const s = lds + wave * SEQ;

  // contiguous run of tiles per workgroup (tile = TT consecutive time samples of one block)
  const int lg_tpb = p.log2_r - LG_TT;
  const uint32_t ntiles = p.nblk << lg_tpb;
  const uint32_t nwg = gridDim.x, wg = blockIdx.x;
  const uint32_t per = ntiles / nwg, extra = ntiles % nwg;
  const uint32_t first = wg * per + (wg < extra ? wg : extra);
  const uint32_t count = per + (wg < extra ? 1u : 0u);
  if (!count) return;

  // The second half of the grid lands in the CUs' second workgroup slots: started ~half a trip late, so that the two workgroups
  // of a CU do not wait for their tiles (and then compute) at the same time.  (Placement affects speed only.)
  if (gridDim.x > 1 && blockIdx.x >= (gridDim.x + 1) / 2) __builtin_amdgcn_s_sleep(127);

  RegTw<LOG2M, VT> rtw;
  rtw.load(p.ftw1_c, p.ftw2_c, ql, LPS, TPS);

  const uint32_t ng = (uint32_t)(C2 / GL);
  const uint32_t loff = (uint32_t)((lane >> 3) * (2 * GL) + (lane & 7));     // cf inside a [t/2] run of 2 * 2C
  cf v[VT][16];
  auto tile_base = [&](uint32_t tile) {   // this wave's time sample of the tile: its [t/2] run + parity offset (wave-uniform)
    const uint32_t b_ = tile >> lg_tpb, t_ = ((tile & ((1u << lg_tpb) - 1u)) << LG_TT) + (uint32_t)wave;
    return p.spill + (uint64_t)b_ * (uint64_t)ng * p.gs + (uint64_t)(t_ >> 1) * (uint64_t)(2 * C2) + (uint64_t)((t_ & 1u) * GL);
  };
  auto load_reg = [&](const cf* base, const int vt, const int a) {
    // branch n1 = a*128 + 64 vt + lane  ->  group n1 / 8 = a*16 + 8 vt + lane / 8, 16 cf apart
    // (plain loads: the sibling wave takes the other half of every line a moment later; non-temporal loads measured 1.38 against 1.30 ms)
    const nf2 t2 = *reinterpret_cast<const nf2*>(base + (size_t)(a * 16 * 2 * GL + vt * 8 * 2 * GL) + loff);
    v[vt][a] = cf{t2.x, t2.y};
  };
  auto load_tile = [&](uint32_t tile) {
    const cf* base = tile_base(tile);
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int a = 0; a < 16; ++a) load_reg(base, vt, a);
  };
  load_tile(first);

  // per-thread column registers: frozen offset / scale (codes), or the rescale sums in double (power / statistics)
  const int rph = RS > 1 ? tid / NG : 0;
  float4 of4[CGT], sc4[CGT];       // codes: frozen offset / scale; else: running sums and sums of squares (fp32, flushed every 8 trips)
#pragma unroll
  for (int g = 0; g < CGT; ++g) of4[g] = sc4[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int flip = p.flip;
  if constexpr (MODE == K2P_CODES) {
#pragma unroll
    for (int g = 0; g < CGT; ++g) {
      const int col0 = ((RS > 1 ? tid % NG : tid) + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
      const int kbase = flip ? (C - 4 - cout0) : cout0;
      of4[g] = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
      sc4[g] = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
    }
  }
  const bool stat_on = MODE != K2P_CODES && p.stat_partial != nullptr;
  const int lg_t = 31 - __builtin_clz(p.tscr);
  const int R = p.r;
  // The fp32 sums of flush k (trips 8 k .. 8 k + 7) leave the registers as they are: 16-byte stores into slot k of the workgroup's
  // own slice of p.stat_slices, [workgroup][slot][sums | sums of squares][NCOL], nothing loaded, nothing waited for.  The workgroup's
  // row of the fp64 table is formed once, behind the loop (fold_sums).  (Before round 6 every flush added into the row in place:
  // load, wait, add in fp64, store at the end of every 8th trip -- 64 KB read and 64 KB written per flush through a table that
  // 5 GB of spill had long pushed out of the caches, and a wait that covered the whole in-order vector-memory queue.  No-return
  // fp64 atomics, tried first of all, took 2.1 ms per IF.)
  // The statistics pass keeps its sums in the order the row lies in the LDS (input channels), slices and table are in output
  // channel order: `flip` reverses the four columns of a group here, once per flush, not once per row.
  static_assert(MODE == K2P_CODES || RS == 1, "the slices hold one row of sums per workgroup");
  auto flush_sums = [&](const uint32_t k) {
    int tl = tid;
    asm volatile("" : "+v"(tl));   // (the CGT target addresses are recomputed here: hoisted out of the loop they were spilled)
    const bool fl = MODE == K2P_STATS && flip;      // (the float-row form sums in output order already)
    float* const sl = p.stat_slices + ((uint64_t)blockIdx.x * (uint64_t)p.stat_slots + (uint64_t)k) * (uint64_t)(2 * NCOL);
#pragma unroll
    for (int g = 0; g < CGT; ++g) {
      const uint64_t col = (uint64_t)(tl + NT * g) * 4u;
      const nf4 a1 = {fl ? of4[g].w : of4[g].x, fl ? of4[g].z : of4[g].y, fl ? of4[g].y : of4[g].z, fl ? of4[g].x : of4[g].w};
      const nf4 a2 = {fl ? sc4[g].w : sc4[g].x, fl ? sc4[g].z : sc4[g].y, fl ? sc4[g].y : sc4[g].z, fl ? sc4[g].x : sc4[g].w};
      *reinterpret_cast<nf4*>(sl + col) = a1;
      *reinterpret_cast<nf4*>(sl + (uint64_t)NCOL + col) = a2;
      of4[g] = sc4[g] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  // The end of the workgroup's life: every thread adds up the slots of its own columns -- what it wrote itself, nobody else's -- one
  // at a time in ascending k, in fp64, starting from 0.0 when the launch starts a rescale interval (p.stat_first: nobody cleared the
  // row, it is not read) and from the row of the table otherwise: ((row + a0) + a1) + ..., the chain the in-place add evaluated, on
  // the same values in the same order, hence the same bits.  The loads of kFoldSlots slots are requested before their adds.
  auto fold_sums = [&](const uint32_t nflush) {
    typedef double nd2 __attribute__((ext_vector_type(2)));
    constexpr uint32_t kFoldSlots = 4;
    const float* const sl0 = p.stat_slices + (uint64_t)blockIdx.x * (uint64_t)p.stat_slots * (uint64_t)(2 * NCOL);
    const bool fresh = p.stat_first != 0;
    for (int g = 0; g < CGT; ++g) {
      const uint64_t col = (uint64_t)(tid + NT * g) * 4u;
      nd2* const row = reinterpret_cast<nd2*>(p.stat_partial + ((uint64_t)blockIdx.x * (uint64_t)NCOL + col) * 2u);
      nd2 acc[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fresh ? nd2{0.0, 0.0} : row[e];
      for (uint32_t k0 = 0; k0 < nflush; k0 += kFoldSlots) {
        nf4 a1[kFoldSlots], a2[kFoldSlots];
#pragma unroll
        for (uint32_t j = 0; j < kFoldSlots; ++j) {
          const uint32_t k = k0 + j < nflush ? k0 + j : nflush - 1u;   // (past the end: the last slot again, not added)
          const float* const sl = sl0 + (uint64_t)k * (uint64_t)(2 * NCOL) + col;
          a1[j] = *reinterpret_cast<const nf4*>(sl);
          a2[j] = *reinterpret_cast<const nf4*>(sl + NCOL);
        }
#pragma unroll
        for (uint32_t j = 0; j < kFoldSlots; ++j) {
          if (k0 + j < nflush) {
            acc[0].x += (double)a1[j].x; acc[0].y += (double)a2[j].x;
            acc[1].x += (double)a1[j].y; acc[1].y += (double)a2[j].y;
            acc[2].x += (double)a1[j].z; acc[2].y += (double)a2[j].z;
            acc[3].x += (double)a1[j].w; acc[3].y += (double)a2[j].w;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) row[e] = acc[e];
    }
  };
  int cur_blk = -1;
  // Everything requested so far (first tile, offset / scale) is waited for here: the loop starts with an empty vector-memory queue.
  // (Inside the loop the compiler waits for the tile's k-th load with vmcnt(31 - k), as if nothing younger were in flight -- its model
  // lets stores retire out of order with respect to loads.  The counter itself runs in issue order, so those waits also cover the
  // emit's 16 row stores of the previous trip; they were issued a barrier and ~1 k cycles earlier than the loads are needed.)
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0); the builtin, not inline asm: the wait-count pass must see it

  for (uint32_t it = 0; it < count; ++it) {
    const uint32_t tile = first + it;
    const int blk = (int)(tile >> lg_tpb);
    const int t0 = (int)(tile & ((1u << lg_tpb) - 1u)) << LG_TT;
    if (blk != cur_blk) {   // (workgroup-uniform) the DC repair of this block: dP[C ..] into the LDS; nobody reads the old one any more
      cur_blk = blk;
      const cf* dP = p.p0 + (size_t)blk * C2 + C;
      int tl = tid;
      asm volatile("" : "+v"(tl));   // (once or twice per workgroup: its addresses are formed here, not kept -- spilled -- across the loop)
#pragma unroll
      for (int i = 0; i < C / NT; ++i) dpl[pw_swz(tl + NT * i, ROT)] = dP[tl + NT * i];
      __syncthreads();
    }

    // ---- FFT_2C across the branches, wave-private (three register passes, two exchanges through the wave's own image) ----
    // the transform and the detection at raised priority: the partner workgroup of the CU is in its emit or waits for its tile, and
    // the wave that computes should win the issue arbitration (digitising pass 1.27 -> 1.25 ms; the statistics pass does not react)
    __builtin_amdgcn_s_setprio(1);
    fwd_passes_w<LOG2M, 1, VT, true>(v, s, ql, p.ftw1_c, p.ftw2_c, &rtw);

    // ---- DC repair + mirror exchange inside the wave: D[k] = conj(W[2C-1-k] + dP[2C-1-k]) ---------------------------------
    // The NEXT tile is requested register by register, each load right behind the last use of its register (unconditional: a load
    // behind a branch makes the compiler's wait-count bookkeeping pessimise every later wait; the last trip re-requests its own
    // tile): the upper halves are free once they have gone to the LDS, the lower ones as the detection walks through them.  A wave
    // that issues its 32 loads in one go sits in the issue stage until the CU's memory pipe has taken them all; spread like this the
    // first ones are also a detection earlier on their way.  (round 4: K2 passes 1.45 / 1.50 -> 1.33 / 1.39 ms with the halves, ...)
    const cf* const nbase = tile_base(it + 1 < count ? tile + 1 : tile);
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const int q = ql + LPS * vt;
      const int k0 = (q / M) + 16 * (q % M);
      // the swizzle of k0 + TPS j repeats with period two in j (static_assert below): two addresses per virtual thread and constant
      // offsets instead of sixteen addresses held -- or spilled -- across the loop
      static_assert((2 * ROT * (TPS / 32)) % 32 == 0 && TPS % 32 == 0, "pw_swz(k + 2 TPS) == pw_swz(k) + 2 TPS");
      const int ks0 = pw_swz(k0, ROT), ks1 = pw_swz(k0 + TPS, ROT);
      cf2* dst = reinterpret_cast<cf2*>(s + q * 18 + 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const cf a = add(v[vt][8 + 2 * i], dpl[ks0 + 2 * TPS * i]);      // = pw_swz(k0 + TPS * (2 i), ROT)
        const cf b = add(v[vt][9 + 2 * i], dpl[ks1 + 2 * TPS * i]);      // = pw_swz(k0 + TPS * (2 i + 1), ROT)
        dst[i] = cf2{a, b};
        __builtin_amdgcn_sched_barrier(0);
        load_reg(nbase, vt, 8 + 2 * i);
        load_reg(nbase, vt, 9 + 2 * i);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    cf wm[VT][8];
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const int q = ql + LPS * vt;
      const cf2* src = reinterpret_cast<const cf2*>(s + (TPS - 1 - q) * 18 + 8);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const cf2 t = src[i];
        wm[vt][7 - 2 * i] = t.a;
        wm[vt][6 - 2 * i] = t.b;
      }
    }
    // ---- A7: detection; the wave's power row goes over its own image (in-order LDS: the reads above are through) ----------
    {
      float* row = reinterpret_cast<float*>(s);
      const int pm = p.pol_mode;
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) {
        const int q = ql + LPS * vt;
        const int k0 = (q / M) + 16 * (q % M);
        const int ks0 = pw_swz(k0, ROT), ks1 = pw_swz(k0 + TPS, ROT);
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
          const cf wk = v[vt][kc];
          const cf d = cf{wm[vt][kc].x, -wm[vt][kc].y};
          const int ks = ((kc & 1) ? ks1 : ks0) + TPS * (kc & ~1);   // = pw_swz(k0 + TPS * kc, ROT), see the DC repair
          if constexpr (PM == 2) {
            row[ks] = 0.5f * ((wk.x * wk.x + wk.y * wk.y) + (d.x * d.x + d.y * d.y));
          } else if constexpr (PM >= 4) {
            // pol0 = (wk + d) / 2, pol1 = -i (wk - d) / 2.  With s1 = |wk|^2, s2 = |d|^2, c = wk d* the four products need neither
            // polarisation spelled out (12 operations per channel instead of 20):
            //   PP = (s1 + s2) / 4 + Re c / 2,  QQ = (s1 + s2) / 4 - Re c / 2,  PQ* = Im c / 2 + i (s1 - s2) / 4
            //   I = PP + QQ = (s1 + s2) / 2,  Q = 2 Re PQ* = Im c,  U = 2 Im PQ* = (s1 - s2) / 2,  V = PP - QQ = Re c
            const float s1 = wk.x * wk.x + wk.y * wk.y, s2 = d.x * d.x + d.y * d.y;
            const float cr = wk.x * d.x + wk.y * d.y, ci = wk.y * d.x - wk.x * d.y;
            if constexpr (PM == 5) {   // Stokes I, Q, U, V of circular feeds
              row[ks] = 0.5f * (s1 + s2);
              row[C + ks] = ci;
              row[2 * C + ks] = 0.5f * (s1 - s2);
              row[3 * C + ks] = cr;
            } else {
              const float q4 = 0.25f * (s1 + s2), hr = 0.5f * cr;
              row[ks] = q4 + hr;
              row[C + ks] = q4 - hr;
              row[2 * C + ks] = 0.5f * ci;
              row[3 * C + ks] = 0.25f * (s1 - s2);
            }
          } else {
            const cf y0 = cf{0.5f * (wk.x + d.x), 0.5f * (wk.y + d.y)};
            const cf y1 = cf{0.5f * (wk.y - d.y), -0.5f * (wk.x - d.x)};
            const float pp = y0.x * y0.x + y0.y * y0.y;
            const float qq = y1.x * y1.x + y1.y * y1.y;
            const float i1 = pp + qq;
            row[ks] = pm == 0 ? pp : (pm == 1 ? qq : i1 * i1);
          }
          // register (vt, kc) has had its last use
          __builtin_amdgcn_sched_barrier(0);
          load_reg(nbase, vt, kc);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();   // every wave's power row is complete (the next tile is on its way: in front of this trip's row stores in
                       // the in-order vector-memory queue)

    // ---- A8 + (A9 + A10 | float rows | rescale sums): workgroup-wide, a thread owns fixed column groups --------------------
    {
      const int T = 1 << lg_t;
      const int rows_out = TT >> lg_t;
      const uint64_t row_base = p.row0 + (uint64_t)blk * (uint64_t)(R >> lg_t) + (uint64_t)(t0 >> lg_t);
      const int nbit = p.nbit;
      const int cg0 = RS > 1 ? tid % NG : tid;          // this thread's first column group
      // one group of four columns of one output row: `a` = its sums in the order the row lies in the LDS (input channels)
      // (`chk`: std::true_type = the row enters the sums only below p.stat_limit; false_type = the caller knows that it does)
      auto emit_group = [&](const float4 a, const int g, const uint64_t orow, auto chk) {
        const int col0 = (cg0 + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
        if constexpr (MODE == K2P_CODES) {
          // rescale in the order the row lies in the LDS (= the order of offset / scale: input channels)
          const float x[4] = {FMUL_RN(FADD_RN(a.x, of4[g].x), sc4[g].x), FMUL_RN(FADD_RN(a.y, of4[g].y), sc4[g].y),
                              FMUL_RN(FADD_RN(a.z, of4[g].z), sc4[g].z), FMUL_RN(FADD_RN(a.w, of4[g].w), sc4[g].w)};
          const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, orow, NIF, prod, cout0);
          if (nbit == 8) {
            *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale, flip != 0);
          } else if (nbit == -32) {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.code_out) + oc) =
                flip ? make_float4(x[3], x[2], x[1], x[0]) : make_float4(x[0], x[1], x[2], x[3]);
          } else {
            uint32_t code[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) code[e] = digitise(x[flip ? 3 - e : e], p.digi_mean, p.digi_scale, p.digi_max);
            if (nbit == 16)
              *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.code_out) + oc) = make_uint2(code[0] | (code[1] << 16), code[2] | (code[3] << 16));
            else
              p.code_out[oc >> 2] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
          }
        } else {
          // float rows: output channel order, and the sums with them.  Statistics only: the sums stay in the order of the LDS row
          // -- a sum does not care, flush_sums puts them into output order once per flush.  (Either way every column sees the same
          // rows in the same order with the same operations.)
          float4 t = a;
          if constexpr (MODE == K2P_POWER) {
            t = make_float4(flip ? a.w : a.x, flip ? a.z : a.y, flip ? a.y : a.z, flip ? a.x : a.w);
            const nf4 o4 = {t.x, t.y, t.z, t.w};
            __builtin_nontemporal_store(o4, reinterpret_cast<nf4*>(p.power_out + orow * (uint64_t)NCOL + col0));
          }
          if (!decltype(chk)::value || (stat_on && orow < p.stat_limit)) {
            of4[g].x += t.x; of4[g].y += t.y; of4[g].z += t.z; of4[g].w += t.w;
            sc4[g].x = fmaf(t.x, t.x, sc4[g].x); sc4[g].y = fmaf(t.y, t.y, sc4[g].y);
            sc4[g].z = fmaf(t.z, t.z, sc4[g].z); sc4[g].w = fmaf(t.w, t.w, sc4[g].w);
          }
        }
      };
      auto row_ptr = [&](const int t, const int g) {
        const int col0 = (cg0 + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
        const int kb = flip ? (C - 4 - cout0) : cout0;
        return reinterpret_cast<const float4*>(reinterpret_cast<const float*>(lds + (size_t)t * SEQ) + prod * C + pw_swz(kb, ROT));
      };
      // the statistics pass tests the end of the rescale interval once per tile (workgroup-uniform): a tile below it sums every
      // row unasked, a tile behind it is not read at all, the one tile that straddles it takes the rolled path and asks per row
      bool all_in = true, none_in = false;
      if constexpr (MODE == K2P_STATS) {
        const uint64_t lim = stat_on ? p.stat_limit : 0;
        all_in = row_base + (uint64_t)rows_out <= lim;
        none_in = row_base >= lim;
      }
      using Chk = std::integral_constant<bool, MODE != K2P_STATS>;
      if (lg_t == 0 && (MODE != K2P_CODES || nbit == 8) && all_in) {
        // the common case, straight-line (in front of a rolled loop the compiler drains vmcnt: the next tile's loads, just
        // requested, would be waited for here): no tscrunch, 8-bit codes or float rows / sums; four rows at a time -- every LDS
        // read of the quartet requested first, then the arithmetic and the stores
        constexpr int NR = TT / RS;              // rows of this thread
        constexpr int QR = (NR * CGT > kK2PQReads) ? (kK2PQReads / CGT > 0 ? kK2PQReads / CGT : 1) : NR;   // at most eight 16-byte reads in flight per thread
#pragma unroll
        for (int j0 = 0; j0 < NR; j0 += QR) {
          float4 acc[QR][CGT];
#pragma unroll
          for (int jj = 0; jj < QR; ++jj)
#pragma unroll
            for (int g = 0; g < CGT; ++g) acc[jj][g] = *row_ptr(rph + RS * (j0 + jj), g);
#pragma unroll
          for (int jj = 0; jj < QR; ++jj)
#pragma unroll
            for (int g = 0; g < CGT; ++g) emit_group(acc[jj][g], g, row_base + (uint64_t)(rph + RS * (j0 + jj)), Chk());
        }
      } else if (!none_in) {
        for (int j = rph; j < rows_out; j += RS) {
#pragma unroll
          for (int g = 0; g < CGT; ++g) {
            float4 acc = *row_ptr(j << lg_t, g);
            for (int tt = 1; tt < T; ++tt) {   // ascending time, as the generic kernels and the oracle sum
              const float4 x = *row_ptr((j << lg_t) + tt, g);
              acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
            }
            emit_group(acc, g, row_base + (uint64_t)j, std::true_type());
          }
        }
      }
    }
    __syncthreads();   // the power rows are consumed: the next trip's first pass may overwrite the images
    if constexpr (MODE != K2P_CODES) {   // at most 8 trips = 32 rows in fp32
      if (stat_on && ((it & kK2PFlushMask) == kK2PFlushMask || it + 1 == count)) flush_sums(it >> 3);   // slot it / 8 (kK2PFlushMask + 1 = 8)
    }
  }
  if constexpr (MODE != K2P_CODES) {
    static_assert(kK2PFlushMask == 7u, "slot = trip / 8");
    if (stat_on) fold_sums((count + kK2PFlushMask) >> 3);
  }
}

}  // namespace fast
