// Fast gfx950 kernels for sequence lengths L = 256*M, M in {2,4,8,16,32} (L = 512 ... 8192; M = 32 only in the
// workgroup-barrier variants, where the radix-32 middle pass occupies half the threads of a sequence):
// every thread keeps 16 complex points in registers; a sequence is owned by TPS = 16*M threads;
// LDS is only the exchange buffer between the three register passes
//     radix-16 over a | radix-M over b | radix-16 over c        index n = a*16M + b*16 + c
// (DIF forward: natural order in, digit-reversed out: thread (ka,kb) register kc holds bin
//  k = ka + 16*kb + 16M*kc;  DIT backward is the exact mirror and returns natural order.)
//
// LDS image of one sequence: element idx at cf-index  idx + 2*(idx >> 4)  (16 B of padding after
// every 128 B): lane-contiguous b64 accesses (passes over a and b) and 128-B-per-lane b128
// accesses (pass over c) are then both bank-conflict free (lane stride 144 B).  Sequences are
// SEQ = L*9/8 + 8 cf apart (the +64 B skews consecutive sequences by half a bank row).
//
// HIP only (not part of the host emulator build): wave64, 1024- or 512-thread workgroups,
// <= 128 VGPRs so that 16 waves stay resident per CU.

#include <type_traits>

namespace fast {

#define FI __device__ __forceinline__

constexpr float kC1 = 0.92387953251128674f;  // cos(pi/8)
constexpr float kS1 = 0.38268343236508977f;  // sin(pi/8)
constexpr float kC2 = 0.70710678118654752f;  // cos(pi/4)

// ---- 8-bit digitiser of the fast kernels (A10): digitise() of kernels_generic.inc, four / eight values at a time ----------
// code = clip(floor(t + 0.5), 0, 255), t = fl(fl(x * digi_scale) + digi_mean), the sum t + 0.5 EXACT.  Rounding that sum toward
// -infinity cannot cross an integer (integers below 2^24 are representable), so floor(t + 0.5) = floor(RTN(t + 0.5)): one
// v_add_f32 issued while MODE.FP_ROUND says "toward -infinity" replaces fract / compare / select of the generic form.  The two
// mode writes and the sums are ONE asm statement: nothing the compiler schedules can land between them.  v_cvt_pk_u8_f32 then
// clips, converts and packs a value per instruction: it saturates (below 0 -> 0, above 255 and +inf -> 255, NaN -> 0) and
// rounds to nearest EVEN (tools/micro/cvt_probe, measured on the MI355X), so it is given the integer v_floor leaves.
// 5 VALU instructions per value behind the rescale (digitise() + packing: ~11).  Held to zero differing codes against the
// oracle's digitiser on identical floats (tests/test_gpu_pins.py).
// rev (wave-uniform): value e goes to byte 3 - e -- a flipped band's four channels in the order the kernel holds them
FI uint32_t digitise4_u8(const float (&x)[4], float dmean, float dscale, bool rev = false) {
  float t[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) t[e] = FADD_RN(FMUL_RN(x[e], dscale), dmean);
  asm volatile(
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2\n\t"
      "s_nop 1\n\t"
      "v_add_f32 %0, 0.5, %0\n\t"
      "v_add_f32 %1, 0.5, %1\n\t"
      "v_add_f32 %2, 0.5, %2\n\t"
      "v_add_f32 %3, 0.5, %3\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\t"
      "s_nop 1"
      : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
  uint32_t c = 0u;
  const uint32_t r3 = rev ? 3u : 0u;     // byte select = e ^ 3 when reversed (a scalar operand of the pack instruction)
#pragma unroll
  for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(t[e]), (uint32_t)e ^ r3, c);
  return c;
}
FI void digitise8_u8(const float (&x)[8], float dmean, float dscale, uint32_t& c0, uint32_t& c1) {
  float t[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = FADD_RN(FMUL_RN(x[e], dscale), dmean);
  asm volatile(
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 2\n\t"
      "s_nop 1\n\t"
      "v_add_f32 %0, 0.5, %0\n\t"
      "v_add_f32 %1, 0.5, %1\n\t"
      "v_add_f32 %2, 0.5, %2\n\t"
      "v_add_f32 %3, 0.5, %3\n\t"
      "v_add_f32 %4, 0.5, %4\n\t"
      "v_add_f32 %5, 0.5, %5\n\t"
      "v_add_f32 %6, 0.5, %6\n\t"
      "v_add_f32 %7, 0.5, %7\n\t"
      "s_setreg_imm32_b32 hwreg(HW_REG_MODE, 0, 2), 0\n\t"
      "s_nop 1"
      : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]));
  c0 = 0u;
  c1 = 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c0 = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(t[e]), (uint32_t)e, c0);
    c1 = __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(t[4 + e]), (uint32_t)e, c1);
  }
}

FI cf mk(float x, float y) { return cf{x, y}; }
FI cf add(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
FI cf sub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }
FI cf mul(cf a, cf b) { return cf{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
FI cf mulc(cf a, cf b) { return cf{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y}; }  // a * conj(b)
// a * exp(DIR * i * 2 pi * m / 16), DIR = -1 forward, +1 backward; m compile-time
template <int M16, int DIR>
FI cf rot16(cf a) {
  constexpr int m = ((M16 % 16) + 16) % 16;
  if constexpr (m == 0) return a;
  else if constexpr (m == 8) return cf{-a.x, -a.y};
  else if constexpr (m == 4) return DIR < 0 ? cf{a.y, -a.x} : cf{-a.y, a.x};
  else if constexpr (m == 12) return DIR < 0 ? cf{-a.y, a.x} : cf{a.y, -a.x};
  else {
    constexpr float cs[16] = {1.f, kC1, kC2, kS1, 0.f, -kS1, -kC2, -kC1, -1.f, -kC1, -kC2, -kS1, 0.f, kS1, kC2, kC1};
    constexpr float sn[16] = {0.f, kS1, kC2, kC1, 1.f, kC1, kC2, kS1, 0.f, -kS1, -kC2, -kC1, -1.f, -kC1, -kC2, -kS1};
    constexpr float c = cs[m];
    constexpr float s = DIR < 0 ? -sn[m] : sn[m];
    return cf{a.x * c - a.y * s, a.x * s + a.y * c};
  }
}

// 4-point DFT in place, natural order out
template <int DIR>
FI void bf4(cf& a, cf& b, cf& c, cf& d) {
  const cf t0 = add(a, c), t1 = sub(a, c), t2 = add(b, d), t3 = sub(b, d);
  a = add(t0, t2);
  c = sub(t0, t2);
  if constexpr (DIR < 0) {
    b = cf{t1.x + t3.y, t1.y - t3.x};
    d = cf{t1.x - t3.y, t1.y + t3.x};
  } else {
    b = cf{t1.x - t3.y, t1.y + t3.x};
    d = cf{t1.x + t3.y, t1.y - t3.x};
  }
}

template <int N, int DIR>
struct Dft;

template <int DIR>
struct Dft<1, DIR> {   // 256-point sequences: radix 16 x 16, no middle pass
  static FI void run(cf (&)[1]) {}
};
template <int DIR>
struct Dft<2, DIR> {
  static FI void run(cf (&v)[2]) {
    const cf a = v[0], b = v[1];
    v[0] = add(a, b);
    v[1] = sub(a, b);
  }
};
template <int DIR>
struct Dft<4, DIR> {
  static FI void run(cf (&v)[4]) { bf4<DIR>(v[0], v[1], v[2], v[3]); }
};
template <int DIR>
struct Dft<8, DIR> {
  // n = 4*n1 + n0, k = k1 + 2*k0: DFT-2 over n1, twiddle W8^(n0*k1), DFT-4 over n0
  static FI void run(cf (&v)[8]) {
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) {
      const cf a = v[n0], b = v[n0 + 4];
      v[n0] = add(a, b);
      v[n0 + 4] = sub(a, b);
    }
    v[5] = rot16<2, DIR>(v[5]);
    v[6] = rot16<4, DIR>(v[6]);
    v[7] = rot16<6, DIR>(v[7]);
    bf4<DIR>(v[0], v[1], v[2], v[3]);
    bf4<DIR>(v[4], v[5], v[6], v[7]);
    // v[4*k1 + k0] = X[k1 + 2*k0]
    const cf t[8] = {v[0], v[4], v[1], v[5], v[2], v[6], v[3], v[7]};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = t[k];
  }
};
template <int DIR>
struct Dft<16, DIR> {
  // n = 4*n1 + n0, k = k1 + 4*k0: DFT-4 over n1, twiddle W16^(n0*k1), DFT-4 over n0
  static FI void run(cf (&v)[16]) {
    bf4<DIR>(v[0], v[4], v[8], v[12]);
    bf4<DIR>(v[1], v[5], v[9], v[13]);
    bf4<DIR>(v[2], v[6], v[10], v[14]);
    bf4<DIR>(v[3], v[7], v[11], v[15]);
    // v[n0 + 4*k1] = Y[n0][k1]
    v[5] = rot16<1, DIR>(v[5]);
    v[6] = rot16<2, DIR>(v[6]);
    v[7] = rot16<3, DIR>(v[7]);
    v[9] = rot16<2, DIR>(v[9]);
    v[10] = rot16<4, DIR>(v[10]);
    v[11] = rot16<6, DIR>(v[11]);
    v[13] = rot16<3, DIR>(v[13]);
    v[14] = rot16<6, DIR>(v[14]);
    v[15] = rot16<9, DIR>(v[15]);
    bf4<DIR>(v[0], v[1], v[2], v[3]);
    bf4<DIR>(v[4], v[5], v[6], v[7]);
    bf4<DIR>(v[8], v[9], v[10], v[11]);
    bf4<DIR>(v[12], v[13], v[14], v[15]);
    // v[4*k1 + k0] = X[k1 + 4*k0]
    const cf t[16] = {v[0], v[4], v[8], v[12], v[1], v[5], v[9], v[13],
                      v[2], v[6], v[10], v[14], v[3], v[7], v[11], v[15]};
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = t[k];
  }
};


// a * exp(DIR * i * 2 pi * m / 32), m compile-time in [0, 16)
template <int M32, int DIR>
FI cf rot32(cf a) {
  if constexpr ((M32 & 1) == 0) return rot16<M32 / 2, DIR>(a);
  else {
    // cos / sin of (2 pi / 32) * {1, 3, 5, 7}
    constexpr float c1 = 0.98078528040323044f, s1 = 0.19509032201612825f;
    constexpr float c3 = 0.83146961230254524f, s3 = 0.55557023301960218f;
    constexpr int m = M32 & 31;
    static_assert(m < 16, "rot32 is used for the first half turn only");
    constexpr float c = (m == 1) ? c1 : (m == 3) ? c3 : (m == 5) ? s3 : (m == 7) ? s1
                      : (m == 9) ? -s1 : (m == 11) ? -s3 : (m == 13) ? -c3 : -c1;
    constexpr float sa = (m == 1) ? s1 : (m == 3) ? s3 : (m == 5) ? c3 : (m == 7) ? c1
                       : (m == 9) ? c1 : (m == 11) ? c3 : (m == 13) ? s3 : s1;
    constexpr float sn = DIR < 0 ? -sa : sa;
    return cf{a.x * c - a.y * sn, a.x * sn + a.y * c};
  }
}
template <int DIR, int N0>
struct Rot32Loop {
  static FI void run(cf (&o)[16]) {
    o[N0] = rot32<N0, DIR>(o[N0]);
    if constexpr (N0 + 1 < 16) Rot32Loop<DIR, N0 + 1>::run(o);
  }
};
template <int DIR>
struct Dft<32, DIR> {
  // n = 16*n1 + n0, k = k1 + 2*k0: DFT-2 over n1, twiddle W32^(n0*k1), DFT-16 over n0
  static FI void run(cf (&v)[32]) {
    cf e[16], o[16];
#pragma unroll
    for (int n0 = 0; n0 < 16; ++n0) {
      const cf a = v[n0], b = v[n0 + 16];
      e[n0] = add(a, b);
      o[n0] = sub(a, b);
    }
    Rot32Loop<DIR, 1>::run(o);
    Dft<16, DIR>::run(e);
    Dft<16, DIR>::run(o);
#pragma unroll
    for (int k0 = 0; k0 < 16; ++k0) {
      v[2 * k0] = e[k0];
      v[2 * k0 + 1] = o[k0];
    }
  }
};

FI int pidx(int idx) { return idx + ((idx >> 4) << 1); }   // pidx(x + 16 m) = pidx(x) + 18 m: strides are spelled out below

typedef float nf4 __attribute__((ext_vector_type(4)));   // native 16-byte vector (non-temporal builtins)


struct __attribute__((aligned(16))) cf2 {
  cf a, b;
};
typedef float nf2 __attribute__((ext_vector_type(2)));
// The spill is written once and read once, 5 GB later: non-temporal stores (measured on the paired-branch K1:
// K1 1.66 -> 1.61 ms, K2 behind it 1.28 -> 1.25 ms)
FI void store_spill(cf2* dst, const cf& a, const cf& b) {
  const nf4 t = {a.x, a.y, b.x, b.y};
  __builtin_nontemporal_store(t, reinterpret_cast<nf4*>(dst));
}
FI void store_spill(cf* dst, const cf& a) {
  const nf2 t = {a.x, a.y};
  __builtin_nontemporal_store(t, reinterpret_cast<nf2*>(dst));
}

template <int LOG2M>
struct Geo {
  static constexpr int M = 1 << LOG2M;
  static constexpr int L = 256 * M;
  static constexpr int TPS = 16 * M;              // threads per sequence
  static constexpr int SEQ = L + L / 8 + 8;       // cf per sequence image
  static constexpr int NB2 = M <= 16 ? 16 / M : 1;  // radix-M butterflies per thread in the b pass (M = 32: threads r >= 16 sit it out)
};

// ---- the two LDS exchanges of a forward transform (registers -> registers) ----------------------
// in : v[a]  = x[a*TPS + q]                 (thread q of the sequence at `s`)
// out: v[kc] = X[ka + 16*kb + 16M*kc],  ka = q / M, kb = q % M
// first- / last-pass twiddles W^(ka q), ka = 1..15: from the table, or from registers the caller filled at the top of the
// kernel -- together with its gather, so that their L2 round trip is not exposed behind the first barrier
struct Tw1Mem {
  const cf* __restrict__ t;
  int tps, q;
  FI cf operator()(int ka) const { return t[ka * tps + q]; }
};
struct Tw1Reg {
  const cf (&t)[16];
  FI cf operator()(int ka) const { return t[ka]; }
};
template <int LOG2M>
FI void load_tw1(cf (&t)[16], const cf* __restrict__ tw1, int q) {
  t[0] = cf{1.f, 0.f};
#pragma unroll
  for (int ka = 1; ka < 16; ++ka) t[ka] = tw1[ka * Geo<LOG2M>::TPS + q];
}
template <int LOG2M, class T1>
FI void fwd_passes_t(cf (&v)[16], cf* s, int q, const T1& tw1, const cf* __restrict__ tw2) {
  using G = Geo<LOG2M>;
  constexpr int M = G::M, TPS = G::TPS;
  Dft<16, -1>::run(v);
#pragma unroll
  for (int ka = 1; ka < 16; ++ka) v[ka] = mul(v[ka], tw1(ka));
#pragma unroll
  for (int ka = 0; ka < 16; ++ka) s[pidx(ka * TPS + q)] = v[ka];
  __syncthreads();
  if constexpr (M > 16) {   // radix-32 middle pass: 16*16 butterflies for 512 threads, ka = r < 16 (whole waves idle)
    const int c = q & 15, r = q >> 4;
    if (r < 16) {
      cf u[M];
#pragma unroll
      for (int b = 0; b < M; ++b) u[b] = s[pidx(r * TPS + b * 16 + c)];
      Dft<M, -1>::run(u);
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mul(u[kb], tw2[kb * 16 + c]);
#pragma unroll
      for (int kb = 0; kb < M; ++kb) s[pidx(r * TPS + kb * 16 + c)] = u[kb];
    }
  } else {
    const int c = q & 15, r = q >> 4;
    cf twb[M];
#pragma unroll
    for (int kb = 1; kb < M; ++kb) twb[kb] = tw2[kb * 16 + c];
#pragma unroll
    for (int i = 0; i < G::NB2; ++i) {
      const int ka = r + M * i;
      cf u[M];
#pragma unroll
      for (int b = 0; b < M; ++b) u[b] = s[pidx(ka * TPS + b * 16 + c)];
      Dft<M, -1>::run(u);
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mul(u[kb], twb[kb]);
#pragma unroll
      for (int kb = 0; kb < M; ++kb) s[pidx(ka * TPS + kb * 16 + c)] = u[kb];
    }
  }
  __syncthreads();
  {
    const cf2* src = reinterpret_cast<const cf2*>(s + q * 18);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const cf2 t = src[i];
      v[2 * i] = t.a;
      v[2 * i + 1] = t.b;
    }
  }
  Dft<16, -1>::run(v);
}
template <int LOG2M>
FI void fwd_passes(cf (&v)[16], cf* s, int q, const cf* __restrict__ tw1, const cf* __restrict__ tw2) {
  fwd_passes_t<LOG2M>(v, s, q, Tw1Mem{tw1, Geo<LOG2M>::TPS, q}, tw2);
}

// mirror image: in v[kc] = A[ka + 16*kb + 16M*kc] (thread q = ka*M + kb), out v[a] = x[a*TPS + q]
// (unnormalised backward transform).  No barrier is needed in front (each thread overwrites the
// 128 B it read last); the caller must place one after it before the LDS is reused.
template <int LOG2M, class T1>
FI void bwd_passes_t(cf (&v)[16], cf* s, int q, const T1& tw1, const cf* __restrict__ tw2) {
  using G = Geo<LOG2M>;
  constexpr int M = G::M, TPS = G::TPS;
  Dft<16, +1>::run(v);
  {
    cf2* dst = reinterpret_cast<cf2*>(s + q * 18);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = cf2{v[2 * i], v[2 * i + 1]};
  }
  __syncthreads();
  if constexpr (M > 16) {
    const int c = q & 15, r = q >> 4;
    if (r < 16) {
      cf u[M];
#pragma unroll
      for (int kb = 0; kb < M; ++kb) u[kb] = s[pidx(r * TPS + kb * 16 + c)];
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mulc(u[kb], tw2[kb * 16 + c]);
      Dft<M, +1>::run(u);
#pragma unroll
      for (int b = 0; b < M; ++b) s[pidx(r * TPS + b * 16 + c)] = u[b];
    }
  } else {
    const int c = q & 15, r = q >> 4;
    cf twb[M];
#pragma unroll
    for (int kb = 1; kb < M; ++kb) twb[kb] = tw2[kb * 16 + c];
#pragma unroll
    for (int i = 0; i < G::NB2; ++i) {
      const int ka = r + M * i;
      cf u[M];
#pragma unroll
      for (int kb = 0; kb < M; ++kb) u[kb] = s[pidx(ka * TPS + kb * 16 + c)];
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mulc(u[kb], twb[kb]);
      Dft<M, +1>::run(u);
#pragma unroll
      for (int b = 0; b < M; ++b) s[pidx(ka * TPS + b * 16 + c)] = u[b];
    }
  }
  __syncthreads();
#pragma unroll
  for (int ka = 0; ka < 16; ++ka) v[ka] = s[pidx(ka * TPS + q)];
#pragma unroll
  for (int ka = 1; ka < 16; ++ka) v[ka] = mulc(v[ka], tw1(ka));
  Dft<16, +1>::run(v);
}
template <int LOG2M>
FI void bwd_passes(cf (&v)[16], cf* s, int q, const cf* __restrict__ tw1, const cf* __restrict__ tw2) {
  bwd_passes_t<LOG2M>(v, s, q, Tw1Mem{tw1, Geo<LOG2M>::TPS, q}, tw2);
}

// 2-bit offset-binary state -> level: the four entries of the run-time table KParams::lut (default -3.3359, -1, +1,
// +3.3359; frbch_config::levels replaces it, so another level scheme is a data change)
struct Levels {
  float l0, l1, l2, l3;
};
FI float level(uint32_t s, const Levels& lv) {   // (four scalars, not an array: an indexable array would go to scratch)
  const float lo = (s & 1u) ? lv.l1 : lv.l0, hi = (s & 1u) ? lv.l3 : lv.l2;
  return (s & 2u) ? hi : lo;
}

// the wave kernels' unpack table in the LDS: nibble (one dual-pol 2-bit sample) -> both polarisations' levels
FI void fill_lut16(cf* lut16, const KParams& p, int tid) {
  if (tid < 16) {
    const Levels lv = {p.lut[0], p.lut[1], p.lut[2], p.lut[3]};
    lut16[tid] = cf{level(tid & 3u, lv), level((tid >> 2) & 3u, lv)};
  }
}

// Unpack tap of the register kernels (frbch_unpack_device, mode 1): the decode of frbch_k1_wave (nibble table in the
// LDS) and of frbch_k1_fast (select chain) on a contiguous payload -- thread t handles payload byte t: samples 2t, 2t+1.
// out [2 decoders][2 pols][nsamp].  grid (ceil(nbytes/256)), 256 threads.
__global__ void __launch_bounds__(256) frbch_unpack_tap_fast(KParams p) {
  __shared__ cf lut16[16];
  fill_lut16(lut16, p, threadIdx.x);
  __syncthreads();
  const uint64_t nsamp = p.row0, nbytes = nsamp >> 1;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= nbytes) return;
  const uint64_t byte = p.payload_off + t;
  const uint64_t fr = byte / p.payload_bytes;
  const uint32_t b = p.frames[fr * p.frame_bytes + p.header_bytes + (uint32_t)(byte - fr * p.payload_bytes)];
  const Levels lv = {p.lut[0], p.lut[1], p.lut[2], p.lut[3]};
#pragma unroll
  for (uint32_t sh = 0; sh < 8; sh += 4) {
    const uint64_t n = 2 * t + (sh >> 2);
    const cf a = lut16[(b >> sh) & 15u];                                                   // frbch_k1_wave
    const cf c = cf{level((b >> sh) & 3u, lv), level((b >> (sh + 2)) & 3u, lv)};           // frbch_k1_fast
    p.power_out[n] = a.x;
    p.power_out[nsamp + n] = a.y;
    p.power_out[2 * nsamp + n] = c.x;
    p.power_out[3 * nsamp + n] = c.y;
  }
}

// x / d for 32-bit x with the host-computed round-up magic (Granlund-Montgomery)
FI uint32_t fastdiv(uint32_t x, uint32_t magic, uint32_t sh) {
  const uint32_t t = __umulhi(magic, x);
  return (t + ((x - t) >> 1)) >> sh;
}


// =================================================================================================
// K1 fast: one workgroup = G = 64/M adjacent polyphase branches of one block, 1024 threads.
// grid (2C/G, nblk).  LDS: G*SEQ cf + R*(G/2) staging bytes.
// =================================================================================================
template <int LOG2M>
__global__ void __launch_bounds__(1024) frbch_k1_fast(KParams p) {
  using GE = Geo<LOG2M>;
  constexpr int M = GE::M, R = GE::L, TPS = GE::TPS, SEQ = GE::SEQ;
  constexpr int G = 1024 / TPS;          // branches per workgroup
  constexpr int RB = G / 2;              // input bytes per n2 row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  unsigned char* stage = smem + (size_t)G * SEQ * sizeof(cf);

  const int tid = threadIdx.x;
  const int seq = tid / TPS, q = tid % TPS;
  // XCD-aware mapping as in the wave kernel: consecutive branch groups (which share input lines) on one XCD
  const int ngrp_ = gridDim.x;
  const int grp = (ngrp_ % 8 == 0) ? (int)(blockIdx.x % 8) * (ngrp_ / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int blk = blockIdx.y;
  const int n1 = grp * G + seq;
  const uint64_t samp0 = (uint64_t)blk * p.hop + (uint64_t)grp * G;   // hop = N, or less with overlap-save (coherent)

  // ---- A3: frame arithmetic + header strip; one RB-byte piece per n2 row ------------------------
  // launch-relative 32-bit byte offsets and a multiply-shift division when the host could set them up (div_magic != 0:
  // `frames` then points at the frame that holds block 0 and rel0 is the payload byte inside it); else 64-bit arithmetic
  const bool rel32 = p.div_magic != 0u;
  const uint32_t x0 = p.rel0 + (uint32_t)(samp0 >> 1);
  if (p.stg) {   // corner-turned by frbch_k0_stage: the workgroup's R*RB = 8192 bytes are contiguous and in stage order
    *reinterpret_cast<uint2*>(stage + tid * 8) =
        *reinterpret_cast<const uint2*>(p.stg + ((size_t)blk * gridDim.x + grp) * (size_t)(R * RB) + (size_t)tid * 8);
  } else
  for (int row = tid; row < R; row += 1024) {
    uint64_t fr;
    uint32_t off;
    if (rel32) {
      const uint32_t x = x0 + (uint32_t)p.c * (uint32_t)row;
      const uint32_t f = fastdiv(x, p.div_magic, p.div_shift);
      fr = f;
      off = x - f * p.payload_bytes;
    } else {
      const uint64_t byte = p.payload_off + ((samp0 + (uint64_t)p.c2 * (uint64_t)row) >> 1);
      fr = byte / p.payload_bytes;
      off = (uint32_t)(byte - fr * p.payload_bytes);
    }
    const unsigned char* src = p.frames + fr * p.frame_bytes + p.header_bytes + off;
    if constexpr (RB == 1) stage[row] = *src;
    else if constexpr (RB == 2) *reinterpret_cast<uint16_t*>(stage + row * RB) = *reinterpret_cast<const uint16_t*>(src);
    else if constexpr (RB == 4) *reinterpret_cast<uint32_t*>(stage + row * RB) = *reinterpret_cast<const uint32_t*>(src);
    else if constexpr (RB == 8) *reinterpret_cast<uint2*>(stage + row * RB) = *reinterpret_cast<const uint2*>(src);
    else *reinterpret_cast<uint4*>(stage + row * RB) = *reinterpret_cast<const uint4*>(src);
  }
  __syncthreads();

  // the fine delay factor of this thread's bins is requested here, in front of the transform, so that its L2 round
  // trip is not exposed behind the forward passes (one workgroup per CU at M >= 16)
  // (not at M = 32: the 128-register budget of that kernel is spent, the early value would be spilled)
  cf rho_early = cf{0.f, 0.f};
  if constexpr (LOG2M <= 4) rho_early = p.td2[(uint64_t)n1 * TPS + ((q / M) + 16 * (q % M))];
  // (the first pass's twiddles requested here as well: measured WORSE, 1.69 -> 1.78 ms at M = 16 -- 15 more loads per thread
  // in front of the unpack)
  constexpr bool PRE_TW = false;
  cf t1r[16];
  if constexpr (PRE_TW) load_tw1<LOG2M>(t1r, p.ftw1_r, q);
  // ---- A4: 2-bit unpack straight into the registers of the first pass ---------------------------
  cf v[16];
  {
    const Levels lv = {p.lut[0], p.lut[1], p.lut[2], p.lut[3]};
    const uint32_t sh = (uint32_t)(seq & 1) << 2;
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const uint32_t b = stage[(a * TPS + q) * RB + (seq >> 1)];
      v[a] = cf{level((b >> sh) & 3u, lv), level((b >> (sh + 2)) & 3u, lv)};
    }
  }
  cf* s = lds + seq * SEQ;
  // M >= 16: the twiddles of the radix-M pass come from the LDS (one workgroup per CU: nothing hides the L2 round
  // trips of 2 x (M-1) loads per thread)
  const cf* tw2 = p.ftw2_r;
  if constexpr (LOG2M >= 4) {   // (M = 16: the coherent pipeline's K1, one workgroup per CU as well)
    cf* tl = reinterpret_cast<cf*>(stage + (size_t)R * RB);
    if (tid < M * 16) tl[tid] = p.ftw2_r[tid];
    tw2 = tl;     // (visible after the first barrier inside fwd_passes)
  }
  if constexpr (PRE_TW) fwd_passes_t<LOG2M>(v, s, q, Tw1Reg{t1r}, tw2);
  else fwd_passes<LOG2M>(v, s, q, p.ftw1_r, tw2);

  // ---- side product S[n1] = A[0]; fractional delay A[k] *= exp(-2 pi i n1 k / N) ----------------
  if (q == 0) p.s_dc[(uint64_t)blk * p.c2 + n1] = v[0];
  {
    const cf rho = (LOG2M <= 4) ? rho_early : p.td2[(uint64_t)n1 * TPS + ((q / M) + 16 * (q % M))];
    const cf* sig = p.td1 + (size_t)n1 * 16;
#pragma unroll
    for (int kc = 0; kc < 16; ++kc) v[kc] = mul(mul(v[kc], sig[kc]), rho);
  }
  // coherent (-F C:D): the dedispersion kernel depends on (channel, fine bin), so the inverse transform waits for K3;
  // the delayed spectrum is spilled as it lies: register kc of thread q = position kc*TPS + q (bin ka + 16 kb + 16M kc)
  if (!p.coherent) bwd_passes<LOG2M>(v, s, q, p.ftw1_r, tw2);
  __syncthreads();  // every thread holds its outputs; LDS may be re-used

  // ---- transpose through LDS into [t][gi] rows (slot swizzled), then one contiguous burst -------
  {
    cf* T = lds;  // R rows of G cf
    constexpr int FSH = (G >= 16) ? 0 : (G == 8 ? 1 : (G == 4 ? 2 : 3));
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int t = a * TPS + q;
      const int f = (t >> FSH) & (G - 1);
      T[t * G + (seq ^ f)] = v[a];
    }
    __syncthreads();
    // slab layout [blk][grp][t][G], or (tile_major == 8) chunks of eight time samples [blk][t/8][grp][t%8][G]: the K2
    // tile then gathers from adjacent cache lines instead of one 16..32-byte piece per 128-KB slab
    const bool chunk8 = p.tile_major == 8;
    const uint32_t ngrp = (uint32_t)(p.c2 / G);
    cf2* dst = reinterpret_cast<cf2*>(p.spill + ((uint64_t)blk * (uint64_t)ngrp + (chunk8 ? 0u : (uint32_t)grp)) * p.gs);
    const cf2* T2 = reinterpret_cast<const cf2*>(T);
    constexpr int CELLS = G / 2;                 // 16-B cells per row
    constexpr int NIT = R * CELLS / 1024;
#pragma unroll 4
    for (int i = 0; i < NIT; ++i) {
      const int id = tid + 1024 * i;
      const int t = id / CELLS, cell = id % CELLS;
      const int f = (t >> FSH) & (G - 1);
      cf2 x = T2[id];
      if (f & 1) {
        const cf tmp = x.a;
        x.a = x.b;
        x.b = tmp;
      }
      const uint32_t trow = chunk8 ? ((((uint32_t)t >> 3) * ngrp + (uint32_t)grp) * 8u + ((uint32_t)t & 7u)) : (uint32_t)t;
      store_spill(dst + (size_t)trow * CELLS + (cell ^ (f >> 1)), x.a, x.b);
    }
  }
}

// =================================================================================================
// K2 fast: one workgroup = TT = NT/TPS consecutive time samples of one block, all 2C branches.
// grid (R/TT, nblk).  Requires tscrunch <= TT.  LDS: TT*SEQ cf (re-used for the power rows).
// =================================================================================================
FI int pw_swz(int k, int rotmul) {  // rotate inside each 32-channel group: conflict-free b32 stores
  return (k & ~31) | ((k + rotmul * ((k >> 5))) & 31);
}

template <int LOG2M, int NT>
__global__ void __launch_bounds__(NT, (LOG2M >= 5 && NT == 512) ? 2 : 1) frbch_k2_fast(KParams p) {   // (M = 32, 512 threads: two workgroups per CU)
  using GE = Geo<LOG2M>;
  constexpr int M = GE::M, C2 = GE::L, C = C2 / 2, TPS = GE::TPS;
  // M = 32: two images of 9/8 * 64 KiB leave exactly C floats of the 160 KiB for the sub-tile sums (no skew between images)
  constexpr int SEQ = LOG2M >= 5 ? GE::L + GE::L / 8 : GE::SEQ;
  constexpr int TT = NT / TPS;
  constexpr int ROT = 32 / M;
  // M = 32, one product: tscrunch > TT allowed -- the workgroup walks tscr/TT sub-tiles and sums them in an LDS row
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);

  const int tid0 = threadIdx.x;
  const int blk = blockIdx.y;
  const int G1 = p.g, R = p.r;
  const int ngrp = C2 / G1;
  const int T = p.tscr;
  constexpr bool ACC = LOG2M >= 5;
  const int nsub = (ACC && T > TT) ? T / TT : 1;
  float* accL = reinterpret_cast<float*>(lds + TT * SEQ);   // [C], swizzled like the power rows
  // XCD-aware tile order (speed only): tiles b and b+8 of the grid share an XCD, so give each XCD a contiguous run
  // of tiles -- neighbouring tiles read neighbouring 16..64-byte pieces of the same lines
  const int ntile_ = gridDim.x;
  const int tile = (ntile_ % 8 == 0) ? (int)(blockIdx.x % 8) * (ntile_ / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int tile0 = tile * TT * nsub;
  const int NIF = p.nif;
  float* pw = reinterpret_cast<float*>(lds);

#pragma unroll 1
  for (int sub = 0; sub < nsub; ++sub) {
  // the thread index is laundered per trip: with a run-time trip count the compiler would otherwise hoist every
  // address of the body out of the loop and spill ~70 registers under the 128-VGPR cap of a 1024-thread workgroup
  int tid = tid0;
  if constexpr (ACC) asm volatile("" : "+v"(tid));
  const int seq = tid / TPS, q = tid % TPS;
  const int k0 = (q / M) + 16 * (q % M);
  const int t0 = tile0 + sub * TT;
  // ---- gather the tile: per K1 group a contiguous run of TT*G1 cf -------------------------------
  {
    const int pairs_per_grp = TT * G1 / 2;
    constexpr int NLD = TT * C2 / 2 / NT;
    cf2 buf[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NT * i;
      const int grp = id / pairs_per_grp, rem = id - grp * pairs_per_grp;
      const cf2* src = (p.tile_major == 8)   // chunks of eight time samples (TT divides 8): [blk][t/8][grp][t%8][G1]
          ? reinterpret_cast<const cf2*>(p.spill + (uint64_t)blk * ngrp * p.gs +
                                         ((((uint64_t)(t0 >> 3) * ngrp + grp) << 3) + (uint64_t)(t0 & 7)) * G1)
          : reinterpret_cast<const cf2*>(p.spill + ((uint64_t)blk * ngrp + grp) * p.gs + (uint64_t)t0 * G1);
      buf[i] = src[rem];   // (plain: the 16..128-byte pieces of neighbouring tiles share cache lines -- non-temporal loads were measured 20 % slower)
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int id = tid + NT * i;
      const int grp = id / pairs_per_grp, rem = id - grp * pairs_per_grp;
      const int tt = rem / (G1 / 2), pr = rem - tt * (G1 / 2);
      const int n1 = grp * G1 + 2 * pr;
      *reinterpret_cast<cf2*>(lds + tt * SEQ + pidx(n1)) = buf[i];
    }
  }
  __syncthreads();

  cf* s = lds + seq * SEQ;
  cf v[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) v[a] = s[pidx(a * TPS + q)];
  const cf* tw2 = p.ftw2_c;
  if constexpr (LOG2M >= 5 && NT == 512) {   // radix-32 twiddles from the LDS (behind the image; see frbch_k1_fast)
    cf* tl = lds + TT * SEQ;
    tl[tid] = p.ftw2_c[tid];
    tw2 = tl;
  }
  fwd_passes<LOG2M>(v, s, q, p.ftw1_c, tw2);

  // ---- mirror exchange: bins k' = 2C-1-k (k' >= C) live in registers kc >= 8 of thread TPS-1-q --
  {
    const cf* dP = p.p0 + (uint64_t)blk * C2;
    cf2* dst = reinterpret_cast<cf2*>(s + q * 18 + 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const cf a = add(v[8 + 2 * i], dP[k0 + TPS * (8 + 2 * i)]);
      const cf b = add(v[9 + 2 * i], dP[k0 + TPS * (9 + 2 * i)]);
      dst[i] = cf2{a, b};
    }
  }
  __syncthreads();
  cf wm[8];  // wm[kc] = W[2C-1-k] + dP, for this thread's k = k0 + TPS*kc, kc < 8
  {
    const cf2* src = reinterpret_cast<const cf2*>(s + (TPS - 1 - q) * 18 + 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const cf2 t = src[i];            // partner registers 8+2i, 9+2i  ->  kc = 7-2i, 6-2i
      wm[7 - 2 * i] = t.a;
      wm[6 - 2 * i] = t.b;
    }
  }
  __syncthreads();  // LDS is free from here on

  // ---- A7 detection into swizzled float rows [tt][prod][k] (through the register sums when sub-tiles add up) ----
  {
    const bool last = sub + 1 == nsub;
    float* row = pw + (size_t)seq * NIF * C;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
      const int k = k0 + TPS * kc;
      const cf wk = v[kc];
      const cf d = cf{wm[kc].x, -wm[kc].y};
      const int ks = pw_swz(k, ROT);
      float o0, o1 = 0.f, o2 = 0.f, o3 = 0.f;
      if (p.pol_mode == 2) {
        o0 = 0.5f * ((wk.x * wk.x + wk.y * wk.y) + (d.x * d.x + d.y * d.y));
      } else {
        const cf y0 = cf{0.5f * (wk.x + d.x), 0.5f * (wk.y + d.y)};
        const cf y1 = cf{0.5f * (wk.y - d.y), -0.5f * (wk.x - d.x)};
        const float pp = y0.x * y0.x + y0.y * y0.y;
        const float qq = y1.x * y1.x + y1.y * y1.y;
        if (p.pol_mode == 0) o0 = pp;
        else if (p.pol_mode == 1) o0 = qq;
        else if (p.pol_mode == 3) o0 = (pp + qq) * (pp + qq);
        else {
          const cf pq = mulc(y0, y1);
          if (p.pol_mode == 5) {   // Stokes I, Q, U, V of circular feeds
            o0 = pp + qq;
            o1 = 2.0f * pq.x;
            o2 = 2.0f * pq.y;
            o3 = pp - qq;
          } else {
            o0 = pp;
            o1 = qq;
            o2 = pq.x;
            o3 = pq.y;
          }
        }
      }
      if constexpr (ACC) {
        if (nsub > 1) {   // fixed order: sample 0 of the tile, then (behind the barrier below) sample 1
          if (seq == 0) accL[ks] = (sub ? accL[ks] : 0.0f) + o0;
          else row[ks] = o0;     // parked in the (free) image area until sample 0 is in
          continue;
        }
      }
      if (last) {
        row[ks] = o0;
        if (p.pol_mode >= 4) {
          row[C + ks] = o1;
          row[2 * C + ks] = o2;
          row[3 * C + ks] = o3;
        }
      }
    }
    if constexpr (ACC) {
      if (nsub > 1) {
        __syncthreads();
        if (seq == 1) {
#pragma unroll
          for (int kc = 0; kc < 8; ++kc) {
            const int ks = pw_swz(k0 + TPS * kc, ROT);
            accL[ks] += row[ks];
          }
        }
        if (!last) __syncthreads();   // the parked values are consumed: the next gather may overwrite them
      }
    }
  }
  }
  __syncthreads();

  // ---- A8 tscrunch + (float power | A9 rescale + A10 digitise), 4 channels per thread-task -------
  {
    const int tid = tid0;
    const int Te = T > TT ? TT : T;             // rows of the tile that add up to one output row
    const int rows_here = TT / Te;
    const int ncol = NIF * C;
    const int flip = p.flip;
    const uint64_t row_base = p.row0 + (uint64_t)blk * (uint64_t)(R / T) + (uint64_t)(tile0 / T);
    for (int id = tid; id < rows_here * ncol / 4; id += NT) {
      const int rr = (id * 4) / ncol;
      const int col0 = id * 4 - rr * ncol;
      const int prod = col0 / C;
      const int cout0 = col0 - prod * C;
      float sv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cout = cout0 + e;
        const int k = p.flip ? (C - 1 - cout) : cout;
        const int ks = pw_swz(k, ROT);
        float a = 0.0f;
        if (ACC && nsub > 1) a = accL[ks];
        else for (int tt = rr * Te; tt < (rr + 1) * Te; ++tt) a += pw[((size_t)tt * NIF + prod) * C + ks];
        sv[e] = a;
      }
      const uint64_t o = (row_base + rr) * (uint64_t)ncol + col0;
      const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, row_base + rr, NIF, prod, cout0);
      if (p.out_mode == FRBCH_OUT_FLOAT_POWER) {
        *reinterpret_cast<float4*>(p.power_out + o) = make_float4(sv[0], sv[1], sv[2], sv[3]);
      } else {
        // four consecutive channels (descending when flipped): one 16-byte load of offset and of scale
        const int kbase = flip ? (C - 4 - cout0) : cout0;
        const float4 of4 = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
        const float4 sc4 = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
        const float ofv[4] = {of4.x, of4.y, of4.z, of4.w}, scv[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = FMUL_RN(FADD_RN(sv[e], ofv[flip ? 3 - e : e]), scv[flip ? 3 - e : e]);
        if (p.nbit == -32) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.code_out) + oc) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
          if (p.nbit == 8) {
            *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale);
          } else {
            uint32_t code[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) code[e] = digitise(x[e], p.digi_mean, p.digi_scale, p.digi_max);
            if (p.nbit == 16)
              *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.code_out) + oc) =
                  make_uint2(code[0] | (code[1] << 16), code[2] | (code[3] << 16));
            else
              p.code_out[oc >> 2] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
          }
        }
      }
    }
  }
}


// =================================================================================================
// "Wave-private" variants: one wavefront owns whole sequences (LPS = min(64, TPS) lanes per
// sequence, VT = TPS/LPS virtual threads per lane), so the FFT passes need no workgroup barrier --
// LDS operations of one wave execute in program order -- and the waves of a workgroup drift apart,
// hiding each other's memory latency.  8 (K1) / 4 (K2) waves per workgroup, <= 256 VGPRs.
// =================================================================================================
// WPS = waves per sequence (1: wave-private; 2: two waves share a sequence and meet at workgroup
// barriers between the passes -- used with small workgroups so that the barrier spans few waves)
template <int LOG2M, int WPS = 1>
struct GeoW : Geo<LOG2M> {
  static constexpr int TPS = Geo<LOG2M>::TPS;
  static constexpr int LPS = TPS < 64 * WPS ? TPS : 64 * WPS;   // lanes (threads) per sequence
  static constexpr int VT = TPS / LPS;                // virtual threads per lane
  static constexpr int SPW = LPS >= 64 ? 1 : 64 / LPS;  // sequences per wave (WPS == 1 only)
};

// Twiddles held in registers for the whole (persistent) kernel: per virtual thread six bases of the radix-16
// pass (W^(j q), W^(4 i q), i, j = 1..3: any W^(ka q) is one product) and three of the radix-M pass
// (W^(c), W^(2c), W^(4c)).  With these the forward passes issue no vector-memory load at all.
template <int LOG2M, int VTN>
struct RegTw {
  cf lo[VTN][4], hi[VTN][4], b2[VTN][4];
  const cf* tl = nullptr;   // M = 32: the radix-32 pass's twiddles lie in the LDS (column c of a [32][16] table); set by the kernel
  FI void load(const cf* __restrict__ tw1, const cf* __restrict__ tw2, int ql, int lps, int tps) {
#pragma unroll
    for (int vt = 0; vt < (LOG2M >= 5 ? 1 : VTN); ++vt) {   // (M = 32: virtual thread 1 derives its factors, see t1s)
      const int q = ql + lps * vt;
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        lo[vt][j] = tw1[j * tps + q];
        hi[vt][j] = tw1[4 * j * tps + q];
      }
      const int c = q & 15;
      if constexpr (LOG2M < 5) {
        if ((1 << LOG2M) > 1) b2[vt][0] = tw2[1 * 16 + c];
        if ((1 << LOG2M) > 2) b2[vt][1] = tw2[2 * 16 + c];
        if ((1 << LOG2M) > 4) b2[vt][2] = tw2[4 * 16 + c];
        if ((1 << LOG2M) > 8) b2[vt][3] = tw2[8 * 16 + c];
      }
    }
  }
  FI cf t1(int vt, int ka) const {
    return (ka < 4) ? lo[vt][ka] : (((ka & 3) == 0) ? hi[vt][ka >> 2] : mul(hi[vt][ka >> 2], lo[vt][ka & 3]));
  }
  // M = 32, two virtual threads 256 apart: W^(ka (q + 256)) = W^(ka q) exp(-2 pi i ka / 32) -- the bases of virtual thread 0
  // and a compile-time rotation serve both (12 registers less)
  FI cf t1s(int vt, int ka) const {   // (ka is a constant after unrolling: the table folds away)
    const cf w = t1(0, ka);
    if (vt == 0) return w;
    constexpr float cs[16] = {1.f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f,
                              0.55557023301960218f, 0.38268343236508977f, 0.19509032201612825f, 0.f, -0.19509032201612825f,
                              -0.38268343236508977f, -0.55557023301960218f, -0.70710678118654752f, -0.83146961230254524f,
                              -0.92387953251128674f, -0.98078528040323043f};
    constexpr float sn[16] = {0.f, 0.19509032201612825f, 0.38268343236508977f, 0.55557023301960218f, 0.70710678118654752f,
                              0.83146961230254524f, 0.92387953251128674f, 0.98078528040323043f, 1.f, 0.98078528040323043f,
                              0.92387953251128674f, 0.83146961230254524f, 0.70710678118654752f, 0.55557023301960218f,
                              0.38268343236508977f, 0.19509032201612825f};
    return mul(w, cf{cs[ka], -sn[ka]});
  }
  FI cf t2(int vt, int kb) const {   // kb in [1, M)
    if constexpr (LOG2M >= 5) return tl[kb * 16];
    cf w = (kb & 1) ? b2[vt][0] : cf{1.f, 0.f};
    if (kb & 2) w = (kb & 1) ? mul(w, b2[vt][1]) : b2[vt][1];
    if (kb & 4) w = (kb & 3) ? mul(w, b2[vt][2]) : b2[vt][2];
    if (kb & 8) w = (kb & 7) ? mul(w, b2[vt][3]) : b2[vt][3];
    return w;
  }
};

// Synchronisation of the WPS waves that share a sequence, between the passes.  WgSync: the workgroup barrier (all
// waves of the workgroup then move in lockstep: everybody computes, then everybody exchanges).  PairSync: a
// monotonic arrival counter per sequence in the LDS -- only the partners wait for each other, the sequences of a
// workgroup drift apart and one pair's LDS exchange overlaps another pair's butterflies.  LDS instructions of a
// wave execute in program order, so the partner's data is in place when its arrival is visible.
struct WgSync {
  FI void operator()() { __syncthreads(); }
};
struct PairSync {
  uint32_t* cnt;        // LDS, zeroed before first use
  uint32_t target;
  uint32_t nwaves;
  bool leader;
  FI void operator()() {
    target += nwaves;
    asm volatile("" ::: "memory");
    if (leader) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (;;) {
      const uint32_t seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
      if ((int32_t)(seen - target) >= 0) break;
      __builtin_amdgcn_s_sleep(1);
    }
    asm volatile("" ::: "memory");
  }
};

// LOADIN: the first pass reads its inputs from the image itself (in place), one virtual thread after the other -- only one
// set of 16 points is live per lane during that pass (2C = 8192: the registers hold the next tile as well)
// (LOADIN also leaves the last pass -- 16 contiguous points per virtual thread, radix 16 -- to the caller, which runs it one
// virtual thread at a time together with its mirror exchange)
// `hook(n)`, n = 0..6 (LOADIN only): fixed points of the two passes where the caller issues its vector-memory requests a
// few at a time -- a wave that issues 16 scattered loads in one go sits in the issue stage until the CU's memory pipe has
// taken them all, i.e. for the whole gather
struct NoHook {
  FI void operator()(int) const {}
};
template <int LOG2M, int WPS = 1, int VTN = 1, bool REGTW = false, class Sync = WgSync, bool LOADIN = false, class Hook = NoHook>
FI void fwd_passes_w(cf (&v)[VTN][16], cf* s, int ql, const cf* __restrict__ tw1,
                     const cf* __restrict__ tw2, const RegTw<LOG2M, VTN>* rt = nullptr, Sync* sync = nullptr, Hook hook = Hook()) {
  constexpr bool HOOKED = !std::is_same<Hook, NoHook>::value;
  auto hk = [&](int n) {
    if constexpr (HOOKED) {
      __builtin_amdgcn_sched_barrier(0);
      hook(n);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  WgSync wg_;
  auto sync_ = [&]() { if (sync) (*sync)(); else wg_(); };
  using G = GeoW<LOG2M, WPS>;
  constexpr int M = G::M, TPS = G::TPS, LPS = G::LPS, VT = G::VT;
  static_assert(VTN == VT, "register array does not match the geometry");
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
    if constexpr (LOADIN) {
      if (vt) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int a = 0; a < 16; ++a) v[vt][a] = s[pidx(q) + a * (TPS + TPS / 8)];
      hk(vt);                    // hooks 0 (and 1): behind the LDS reads of a virtual thread's inputs
    }
    Dft<16, -1>::run(v[vt]);
#pragma unroll
    for (int ka = 1; ka < 16; ++ka) v[vt][ka] = mul(v[vt][ka], REGTW ? (M > 16 ? rt->t1s(vt, ka) : rt->t1(vt, ka)) : tw1[ka * TPS + q]);
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) s[pidx(q) + ka * (TPS + TPS / 8)] = v[vt][ka];
  }
  if constexpr (LOADIN) hk(2);   // hook 2: behind the first pass
  else hk(0);                    // (without LOADIN: hook 0 behind the first pass, 1.. behind each butterfly of the middle pass)
  if constexpr (WPS > 1) sync_();
  if constexpr (M > 1) {   // (M = 1: the image written above is already the one read below)
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
    const int c = q & 15, r = q >> 4;
    if constexpr (M > 16) {   // radix 32: 16 rows of 16 butterflies for 512 virtual threads -- r < 16 only (with two virtual
      if (r >= 16) continue;  // threads per lane, LPS = 256, that is virtual thread 0 of every lane: nobody idles)
      cf u[M];
#pragma unroll
      for (int b = 0; b < M; ++b) u[b] = s[r * (TPS + TPS / 8) + b * 18 + c];
      hk(3);                     // hook 3: behind the LDS reads of the radix-32 pass
      Dft<M, -1>::run(u);
#pragma unroll
      for (int kb = 1; kb < M; ++kb) {   // (twiddles in batches of eight, each stored at once: a batch of 31 costs 62 registers)
        u[kb] = mul(u[kb], REGTW ? rt->t2(vt, kb) : tw2[kb * 16 + c]);
        s[r * (TPS + TPS / 8) + kb * 18 + c] = u[kb];
        if ((kb & 7) == 7) {
          if constexpr (LOADIN) hk(4 + (kb >> 3));   // hooks 4, 5, 6: between the batches
          else __builtin_amdgcn_sched_barrier(0);
        }
      }
      s[r * (TPS + TPS / 8) + c] = u[0];
    } else {
    cf twb[M];
#pragma unroll
    for (int kb = 1; kb < M; ++kb) twb[kb] = REGTW ? rt->t2(vt, kb) : tw2[kb * 16 + c];
#pragma unroll
    for (int i = 0; i < G::NB2; ++i) {
      const int ka = r + M * i;
      cf u[M];
#pragma unroll
      for (int b = 0; b < M; ++b) u[b] = s[ka * (TPS + TPS / 8) + b * 18 + c];
      Dft<M, -1>::run(u);
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mul(u[kb], twb[kb]);
#pragma unroll
      for (int kb = 0; kb < M; ++kb) s[ka * (TPS + TPS / 8) + kb * 18 + c] = u[kb];
      if constexpr (!LOADIN) hk(1 + vt * G::NB2 + i);
    }
    }
  }
  if constexpr (WPS > 1) sync_();
  }
  if constexpr (LOADIN) return;
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
    const cf2* src = reinterpret_cast<const cf2*>(s + q * 18);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const cf2 t = src[i];
      v[vt][2 * i] = t.a;
      v[vt][2 * i + 1] = t.b;
    }
    Dft<16, -1>::run(v[vt]);
  }
}

struct NoMid {
  FI void operator()() const {}
};
// `mid` runs in front of the last virtual thread's radix-M pass: the place of a trip where the vector-memory
// queue of the CU has drained the previous block's stores (K1 issues its input prefetch there)
// `hook(n)` (see fwd_passes_w): 0 behind the first pass, 1.. behind each butterfly of the middle pass, then one behind the LDS
// reads of each virtual thread's last pass
template <int LOG2M, int WPS = 1, int VTN = 1, bool LAST = true, bool REGTW = false, class Mid = NoMid, class Sync = WgSync, class Hook = NoHook>
FI void bwd_passes_w(cf (&v)[VTN][16], cf* s, int ql, const cf* __restrict__ tw1,
                     const cf* __restrict__ tw2, const RegTw<LOG2M, VTN>* rt = nullptr, Mid mid = Mid(), Sync* sync = nullptr,
                     Hook hook = Hook()) {
  constexpr bool HOOKED = !std::is_same<Hook, NoHook>::value;
  auto hk = [&](int n) {
    if constexpr (HOOKED) {
      __builtin_amdgcn_sched_barrier(0);
      hook(n);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  WgSync wg_;
  auto sync_ = [&]() { if (sync) (*sync)(); else wg_(); };
  using G = GeoW<LOG2M, WPS>;
  constexpr int M = G::M, TPS = G::TPS, LPS = G::LPS, VT = G::VT;
  static_assert(VTN == VT, "register array does not match the geometry");
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
    Dft<16, +1>::run(v[vt]);
    cf2* dst = reinterpret_cast<cf2*>(s + q * 18);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = cf2{v[vt][2 * i], v[vt][2 * i + 1]};
  }
  hk(0);
  if constexpr (WPS > 1) sync_();
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    if (vt == (M > 16 ? 0 : VT - 1)) {   // (M = 32: virtual thread 0 is the one that works in this pass)
      __builtin_amdgcn_sched_barrier(0);
      mid();
      __builtin_amdgcn_sched_barrier(0);
    }
    const int q = ql + LPS * vt;
    const int c = q & 15, r = q >> 4;
    if constexpr (M > 16) {   // radix 32: r < 16 only (with LPS = 256 that is virtual thread 0 of every lane), see fwd_passes_w
      if (r >= 16) continue;
      cf u[M];
#pragma unroll
      for (int kb = 0; kb < M; ++kb) u[kb] = s[r * (TPS + TPS / 8) + kb * 18 + c];
#pragma unroll
      for (int kb = 1; kb < M; ++kb) {   // (twiddles in batches of eight: registers)
        u[kb] = mulc(u[kb], REGTW ? rt->t2(vt, kb) : tw2[kb * 16 + c]);
        if ((kb & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
      Dft<M, +1>::run(u);
#pragma unroll
      for (int b = 0; b < M; ++b) s[r * (TPS + TPS / 8) + b * 18 + c] = u[b];
    } else {
    cf twb[M];
#pragma unroll
    for (int kb = 1; kb < M; ++kb) twb[kb] = REGTW ? rt->t2(vt, kb) : tw2[kb * 16 + c];
#pragma unroll
    for (int i = 0; i < G::NB2; ++i) {
      const int ka = r + M * i;
      cf u[M];
#pragma unroll
      for (int kb = 0; kb < M; ++kb) u[kb] = s[ka * (TPS + TPS / 8) + kb * 18 + c];
#pragma unroll
      for (int kb = 1; kb < M; ++kb) u[kb] = mulc(u[kb], twb[kb]);
      Dft<M, +1>::run(u);
#pragma unroll
      for (int b = 0; b < M; ++b) s[ka * (TPS + TPS / 8) + b * 18 + c] = u[b];
      hk(1 + vt * G::NB2 + i);
    }
    }
  }
  if constexpr (!LAST) return;   // the caller runs the last pass itself (K1: remapped for direct stores)
  if constexpr (WPS > 1) sync_();
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
#pragma unroll
    for (int ka = 0; ka < 16; ++ka) v[vt][ka] = s[pidx(q) + ka * (TPS + TPS / 8)];
    hk(1 + VT * G::NB2 + vt);
#pragma unroll
    for (int ka = 1; ka < 16; ++ka) v[vt][ka] = mulc(v[vt][ka], REGTW ? rt->t1(vt, ka) : tw1[ka * TPS + q]);
    Dft<16, +1>::run(v[vt]);
  }
}


// =================================================================================================
// K0: corner-turn of the 2-bit payload for the wave K1.  A K1 workgroup needs RB bytes (its G branches) of every one
// of the R rows of a block, rows C bytes apart: gathered directly, every lane of every load touches its own cache line
// (64 address-unit requests per instruction) and the CU's in-order vector-memory pipe, which also carries the 128 KB of
// row stores per block, becomes the bottleneck (K1 1.98 ms, 1.64 ms with contiguous input).  K0 transposes 64-row x
// 256-byte tiles through the LDS into [blk][group][row][RB]: coalesced both ways, 1 B/sample of extra traffic.
// grid (R/64 * C/256, nblk), 256 threads, LDS 64 * 260 bytes.  Strips the frame headers on the way (A3).
// =================================================================================================
template <int RB, bool WIDE>   // WIDE: 16-byte loads (frame geometry and start offset multiples of 16 bytes)
__global__ void __launch_bounds__(256) frbch_k0_stage(KParams p) {
  constexpr int TG = 256 / RB;                  // branch groups per tile
  constexpr int PITCH = 260;                    // bytes per tile row in the LDS (65 words: conflict-free columns)
  __shared__ __attribute__((aligned(16))) unsigned char tile[64 * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int R = p.r, rowb = p.c;                // bytes per row = 2C samples / 2
  const int gtiles = rowb / 256;
  const int rt = blockIdx.x / gtiles, gt = blockIdx.x - rt * gtiles;
  const int r0 = rt * 64, blk = blockIdx.y;
  const uint32_t xb = p.rel0 + (uint32_t)blk * (uint32_t)(p.hop >> 1) + (uint32_t)gt * 256u;   // hop = N, less with overlap-save
  if constexpr (WIDE) {   // 16 lanes per 256-byte row piece: a wave fetches four rows per instruction
    uint4 t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = (tid >> 4) + 16 * i;
      const uint32_t x = xb + (uint32_t)(tid & 15) * 16u + (uint32_t)rowb * (uint32_t)(r0 + row);
      const uint32_t fr = fastdiv(x, p.div_magic, p.div_shift);
      const uint32_t off = x - fr * p.payload_bytes;
      t[i] = *reinterpret_cast<const uint4*>(p.frames + (size_t)fr * p.frame_bytes + p.header_bytes + off);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t* d = reinterpret_cast<uint32_t*>(tile + ((tid >> 4) + 16 * i) * PITCH + (tid & 15) * 16);
      d[0] = t[i].x; d[1] = t[i].y; d[2] = t[i].z; d[3] = t[i].w;
    }
  } else {
    const uint32_t x0 = xb + (uint32_t)lane * 4u;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int row = w + 4 * i;
      const uint32_t x = x0 + (uint32_t)rowb * (uint32_t)(r0 + row);
      const uint32_t fr = fastdiv(x, p.div_magic, p.div_shift);
      const uint32_t off = x - fr * p.payload_bytes;
      *reinterpret_cast<uint32_t*>(tile + row * PITCH + lane * 4) =
          *reinterpret_cast<const uint32_t*>(p.frames + (size_t)fr * p.frame_bytes + p.header_bytes + off);
    }
  }
  __syncthreads();
  // output: per group 64 rows x RB bytes = 64*RB contiguous bytes; 16-byte pieces, 4 per thread
  const int ngrp = rowb / RB;
  constexpr int PPG = 64 * RB / 16;             // pieces per group
  constexpr int RPP = 16 / RB;                  // rows per piece
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + 256 * i;
    const int g = q / PPG, ch = q - g * PPG;
    union { uint4 v; unsigned char b[16]; } u;
#pragma unroll
    for (int e = 0; e < RPP; ++e) {
      const unsigned char* src = tile + (ch * RPP + e) * PITCH + g * RB;
      if constexpr (RB == 1) u.b[e] = *src;
      else if constexpr (RB == 2) *reinterpret_cast<uint16_t*>(u.b + e * RB) = *reinterpret_cast<const uint16_t*>(src);
      else if constexpr (RB == 4) *reinterpret_cast<uint32_t*>(u.b + e * RB) = *reinterpret_cast<const uint32_t*>(src);
      else if constexpr (RB == 8) { *reinterpret_cast<uint32_t*>(u.b + e * RB) = *reinterpret_cast<const uint32_t*>(src);
                                    *reinterpret_cast<uint32_t*>(u.b + e * RB + 4) = *reinterpret_cast<const uint32_t*>(src + 4); }
      else { for (int k = 0; k < 4; ++k) *reinterpret_cast<uint32_t*>(u.b + 4 * k) = *reinterpret_cast<const uint32_t*>(src + 4 * k); }
    }
    unsigned char* dst = p.stg_out + ((size_t)((size_t)blk * ngrp + (size_t)gt * TG + g) * R + (size_t)r0) * RB + (size_t)ch * 16;
    *reinterpret_cast<uint4*>(dst) = u.v;
  }
}

// NW waves per workgroup, WPS waves per sequence: G = (NW/WPS)*SPW branches per workgroup.  The
// spill layout group is GL = p.g >= G branches; a workgroup fills its G*8-byte share of every row.
// STG: the input comes corner-turned from frbch_k0_stage (compile-time: a run-time choice between the two fetches
// makes the compiler wait for the loaded rows where the paths merge)
// COH: coherent dedispersion (-F C:D): forward transform and delay only -- the delayed branch spectrum is spilled as it lies
// (register kc of virtual thread q = position kc*TPS + q), through the same remapped store sweep without its transform
// MSK (staged input only): blocks that touch frames flagged invalid or inserted for missing frame numbers (KParams::fbad, DESIGN.md
// section 3a).  Every n2 row piece of a workgroup (RB bytes, 4-byte aligned) lies inside ONE frame: the thread that copies a row
// into the stage looks its frame up in the bitmap and leaves a flag per row beside the stage; the unpack reads samples of flagged
// rows as 0 (the level table's mean), as the generic K1 does per sample.  Round 3 sent such blocks to the generic radix-2 K1.
template <int LOG2M, int NW, int WPS, bool STG = false, bool COH = false, bool MSK = false>
__global__ void __launch_bounds__(64 * NW, (LOG2M >= 5 ? 1 : 2)) frbch_k1_wave(KParams p) {
  static_assert(!MSK || STG, "the frame mask rides on the staged input");
  using GE = GeoW<LOG2M, WPS>;
  constexpr int M = GE::M, R = GE::L, TPS = GE::TPS, LPS = GE::LPS, VT = GE::VT, SPW = GE::SPW;
  constexpr int SEQ = GE::L + GE::L / 8 + 4;   // images 32 B askew: branch-fastest lanes of the remapped pass hit distinct banks
  constexpr int NT = 64 * NW;
  constexpr int G = (NW / WPS) * SPW;    // branches per workgroup
  constexpr int RB = G / 2;              // input bytes per n2 row
  constexpr int NROW = R / NT;           // input rows fetched per thread and block
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  unsigned char* stage = smem + (size_t)G * SEQ * sizeof(cf);
  cf* lut16 = reinterpret_cast<cf*>(stage + (size_t)R * RB);
  cf* sigl = lut16 + 16;                 // [G][16] coarse delay factors of this workgroup's branches
  uint32_t* paircnt = reinterpret_cast<uint32_t*>(sigl + G * 16);   // [G] arrival counters (WPS > 1)
  // MSK: one flag byte per n2 row, behind everything else (M = 32: behind the radix-32 twiddles, and one BIT per row -- a thread
  // copies 16 rows there, exactly one 16-bit word of flags; the LDS has 3.7 KB to spare, not 8)
  unsigned char* rowbad = reinterpret_cast<unsigned char*>(paircnt + ((G + 1) & ~1)) + (LOG2M >= 5 ? M * 16 * sizeof(cf) : 0);
  static_assert(!MSK || LOG2M < 5 || R / (64 * NW) == 16, "flag bits: one 16-bit word per thread");

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int seq = WPS > 1 ? wave / WPS : wave * SPW + lane / LPS;
  const int ql = WPS > 1 ? (wave % WPS) * 64 + lane : lane % LPS;
  __builtin_assume(ql >= 0 && ql < LPS);
  // XCD-aware mapping: workgroups b, b+8, b+16, ... share an XCD (round-robin dispatch).  The groups
  // that read the same 128-B input lines are consecutive, so give every XCD a contiguous run of
  // groups: each input line is then fetched into one L2 only (placement affects speed, not results).
  const int ngrp_ = gridDim.x;
  const int grp = (ngrp_ % 8 == 0) ? (int)(blockIdx.x % 8) * (ngrp_ / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int n1 = grp * G + seq;
  const int nblk = (int)p.nblk;

  fill_lut16(lut16, p, tid);
  // per-branch fractional-delay factors: constant over the blocks of this launch
  // the 16 coarse delay factors of every branch go to the LDS once: the loop body must not issue vector-memory
  // loads (they would queue behind the stores of the previous block)
  if (tid < G * 16) sigl[tid] = p.td1[(size_t)(grp * G + (tid >> 4)) * 16 + (tid & 15)];
  if (WPS > 1 && tid < G) paircnt[tid] = 0u;
  PairSync psync{paircnt + seq, 0u, (uint32_t)WPS, lane == 0};
  // (R = 8192, four waves per sequence: the hardware barrier of the eight waves beats the polled counters, K1 1.94 -> 1.84 ms)
  PairSync* const psp = (WPS > 1 && LOG2M < 5) ? &psync : nullptr;
  const cf* sig = sigl + seq * 16;

  // A3: frame arithmetic (multiply-shift division) + header strip; RB bytes per n2 row.
  // The rows of the NEXT block are fetched into registers while the current block is transformed.
  typedef typename std::conditional<RB == 1, uint8_t, typename std::conditional<RB == 2, uint16_t, typename std::conditional<RB == 4, uint32_t,
          typename std::conditional<RB == 8, uint2, uint4>::type>::type>::type>::type piece_t;
  piece_t nxt[NROW];
  // staged input (frbch_k0_stage): the R*RB bytes of this workgroup and block are contiguous and already in stage order
  // (row-major): thread tid copies bytes [tid*NROW*RB, +NROW*RB) -- one 8- or 16-byte load instead of NROW gathers
  constexpr bool staged = STG;
  typedef typename std::conditional<NROW * RB == 16, uint4, typename std::conditional<NROW * RB == 8, uint2, uint32_t>::type>::type chunk_t;
  static_assert(sizeof(chunk_t) == NROW * RB || NROW * RB == 4, "staged chunk per thread is 4, 8 or 16 bytes");
  chunk_t nxtc = chunk_t();
  uint32_t nxtbad = 0u;   // MSK: bit i = row tid * NROW + i of the fetched block lies in a flagged frame
  auto fetch = [&](int blk) {
    if constexpr (staged) {
      nxtc = *reinterpret_cast<const chunk_t*>(p.stg + ((size_t)blk * gridDim.x + grp) * (size_t)(R * RB) + (size_t)tid * (NROW * RB));
      if constexpr (MSK) {
        const uint32_t x0 = p.rel0 + (uint32_t)blk * (uint32_t)(p.hop >> 1) + (uint32_t)grp * RB;
        nxtbad = 0u;
#pragma unroll
        for (int i = 0; i < NROW; ++i) {
          const uint32_t x = x0 + (uint32_t)p.c * (uint32_t)(tid * NROW + i);
          const uint64_t f = p.fbad_frame0 + fastdiv(x, p.div_magic, p.div_shift);
          nxtbad |= ((p.fbad[f >> 5] >> (f & 31)) & 1u) << i;
        }
      }
      return;
    }
    const uint32_t x0 = p.rel0 + (uint32_t)blk * (uint32_t)(p.hop >> 1) + (uint32_t)grp * RB;   // hop = N, less with overlap-save (coherent)
#pragma unroll
    for (int i = 0; i < NROW; ++i) {
      const int row = tid + NT * i;
      const uint32_t x = x0 + (uint32_t)p.c * (uint32_t)row;
      const uint32_t fr = fastdiv(x, p.div_magic, p.div_shift);
      const uint32_t off = x - fr * p.payload_bytes;
      nxt[i] = *reinterpret_cast<const piece_t*>(p.frames + (size_t)fr * p.frame_bytes + p.header_bytes + off);
    }
  };
  auto refill = [&]() {
    if constexpr (staged) {
      *reinterpret_cast<chunk_t*>(stage + (size_t)tid * (NROW * RB)) = nxtc;
      if constexpr (MSK) {
        if constexpr (LOG2M >= 5) {
          reinterpret_cast<uint16_t*>(rowbad)[tid] = (uint16_t)nxtbad;
        } else {
#pragma unroll
          for (int i = 0; i < NROW; ++i) rowbad[tid * NROW + i] = (unsigned char)((nxtbad >> i) & 1u);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NROW; ++i) *reinterpret_cast<piece_t*>(stage + (size_t)(tid + NT * i) * RB) = nxt[i];
    }
  };
  fetch(blockIdx.y);
  refill();
  // staged input and a loop-free last pass: the rows are requested TWO blocks ahead, right behind the first barrier (in
  // front of the block's stores in the in-order queue), and consumed a whole trip later: no vector-memory instruction is
  // left in the middle of the transforms and the request's latency is hidden completely
  // PAIRED last pass: a lane owns TWO adjacent branches at one time index (16-byte row stores, one sweep, the twiddles
  // shared by the two transforms) when that tiles the sequence: 128/G time indices per wave
  constexpr bool PAIRED = !COH && (LOG2M == 3) && (WPS == 1) && (G == 8) && (TPS * G == NW * 128);
  constexpr bool AHEAD2 = STG && PAIRED;

  const cf* tw1 = p.ftw1_r;
  const cf* tw2 = p.ftw2_r;
  cf* s = lds + seq * SEQ;
  RegTw<LOG2M, VT> rtw;
  rtw.load(tw1, tw2, ql, LPS, TPS);
  if constexpr (LOG2M >= 5) {   // the radix-32 twiddles behind the arrival counters (visible after the barrier in front of the loop)
    cf* tl = reinterpret_cast<cf*>(paircnt + ((G + 1) & ~1));
    for (int i = tid; i < M * 16; i += NT) tl[i] = p.ftw2_r[i];
    rtw.tl = tl + (ql & 15);
  }
  // The fine part of the fractional delay, exp(-2 pi i n1 k0 / N) for bin k = k0 + 16M kc with k0 = ka + 16 kb, is
  // A^ka B^kb (A = exp(-2 pi i n1 / N), B = A^16): a factor per OUTPUT INDEX of the first and of the middle forward pass,
  // where that index is a register index.  So it rides on the forward twiddles for free: A^j, A^4i are multiplied into
  // the loop-invariant pass-1 bases once (the backward passes use other bases), B^(2^m) into a per-block copy of the
  // middle-pass bases (three products per virtual thread and block).  Left for the delay stage: the 15 coarse factors
  // sig[kc] -- one complex product per point instead of two (-136 VALU instructions of 2517 per wave and block).
  // (R = 8192, M = 32: the middle-pass twiddles lie in one LDS table shared by the branches, so nothing is folded; the delay
  // stage multiplies by the whole fine factor of the virtual thread, rho[vt], loaded once)
  cf bpow[4] = {cf{1.f, 0.f}, cf{1.f, 0.f}, cf{1.f, 0.f}, cf{1.f, 0.f}};
  cf rho[VT];
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) rho[vt] = cf{1.f, 0.f};
  if constexpr (LOG2M >= 5) {
    const cf* dl = p.td2 + (uint64_t)n1 * TPS;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const int q = ql + LPS * vt;
      rho[vt] = dl[(q / M) + 16 * (q % M)];
    }
  } else {
    const cf* dl = p.td2 + (uint64_t)n1 * TPS;     // [k0] = exp(-2 pi i n1 k0 / N), k0 < TPS
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        rtw.lo[vt][j] = mul(rtw.lo[vt][j], dl[j]);
        rtw.hi[vt][j] = mul(rtw.hi[vt][j], dl[4 * j]);
      }
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if ((1 << m) < M) bpow[m] = dl[16 << m];
  }
  // base twiddles of the remapped last pass (lane = branch gi x time index pl), loop-invariant: loaded once, so
  // that no vector-memory load of the loop body sits behind the stores of the previous block (vmcnt is in order)
  cf tlo0[4], thi0[4];
  {
    constexpr int PPW0 = PAIRED ? 128 / G : 64 / G, NSW0 = TPS / (NW * PPW0);
    const int pp0 = (wave * NSW0) * PPW0 + lane / (PAIRED ? G / 2 : G);
    const cf* twp = tw1 + pp0;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      tlo0[j] = twp[j * TPS];
      thi0[j] = twp[4 * j * TPS];
    }
  }
  if constexpr (AHEAD2) {
    if ((int)blockIdx.y + (int)gridDim.y < nblk) fetch(blockIdx.y + gridDim.y);   // the second block's rows wait in registers
  }
  __syncthreads();   // stage holds the rows of the first block

  for (int blk = blockIdx.y; blk < nblk; blk += gridDim.y) {
    const bool more = blk + (int)gridDim.y < nblk;
    // Placement of the vector-memory instructions of a trip (phase stamps, tools_stamps.py): the CU needs ~11000
    // cycles into the next trip to drain the 128 KB of row stores, its vector-memory queue is in order, and a load
    // issued while it drains blocks its wave (with the fetch at the loop top the waves left it up to 7000 cycles
    // apart and the first barrier charged that to all); a load issued later than ~4000 cycles before its use
    // exposes its latency.  So: the fetch of the next block's rows goes into the middle of the backward passes,
    // the s_dc store and the row stores behind the first barrier, and nothing else touches vector memory.
    // Waves released together by the barrier run the same phases at the same time (all VALU, then all LDS): the
    // resources take turns.  The second half of the waves (the SIMD partners of the first half) starts late so
    // that one partner computes while the other exchanges through the LDS.
    // Issue arbitration between the two waves of a SIMD goes by priority, then age: the second-dispatched half of
    // the workgroup (waves NW/2..) loses every phase (phase stamps: it reaches the first barrier ~3000 cycles after
    // the first half, which waits).  The halves take turns at priority 1, so that both arrive together.
    const bool young = wave >= NW / 2;
    if (young) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0);

    // ---- A4: 2-bit unpack (16-entry LUT: nibble -> both polarisations) --------------------------
    cf v[VT][16];
    {
      const uint32_t sh = (uint32_t)(seq & 1) << 2;
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) {
        const int q = ql + LPS * vt;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
          const uint32_t b = stage[(a * TPS + q) * RB + (seq >> 1)];
          v[vt][a] = lut16[(b >> sh) & 15u];
          if constexpr (MSK) {
            const int row = a * TPS + q;
            const bool bad = LOG2M >= 5 ? ((reinterpret_cast<const uint16_t*>(rowbad)[row >> 4] >> (row & 15)) & 1u) != 0u : rowbad[row] != 0;
            if (bad) v[vt][a] = cf{0.f, 0.f};
          }
        }
      }
    }
    if constexpr (LOG2M >= 5) {
      fwd_passes_w<LOG2M, WPS, VT, true, PairSync>(v, s, ql, tw1, tw2, &rtw, psp);
    } else {
      RegTw<LOG2M, VT> rtf = rtw;                  // forward bases: the middle pass carries B^kb as well
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if ((1 << m) < M) {
          asm volatile("" : "+v"(bpow[m].x), "+v"(bpow[m].y));   // (keeps the products inside the loop: no registers to spare)
#pragma unroll
          for (int vt = 0; vt < VT; ++vt) rtf.b2[vt][m] = mul(rtw.b2[vt][m], bpow[m]);
        }
      fwd_passes_w<LOG2M, WPS, VT, true, PairSync>(v, s, ql, tw1, tw2, &rtf, psp);
    }
    if (young) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(1);
    const cf sdc = v[0][0];
    if constexpr (LOG2M >= 5) {                    // whole fine factor here (nothing folded into the forward twiddles)
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) v[vt][0] = mul(v[vt][0], rho[vt]);
    }
#pragma unroll
    for (int kc = 1; kc < 16; ++kc) {              // (sig[0] = 1; the fine factors came with the forward twiddles)
      const cf sg = sig[kc];
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) v[vt][kc] = (LOG2M >= 5) ? mul(mul(v[vt][kc], sg), rho[vt]) : mul(v[vt][kc], sg);
    }
    if constexpr (COH) {
      if (more) fetch(blk + gridDim.y);
      if constexpr (WPS > 1) { if (psp) (*psp)(); else __syncthreads(); }   // the partner wave has read its rows of the image
#pragma unroll
      for (int vt = 0; vt < VT; ++vt) {
        const int q = ql + LPS * vt;
#pragma unroll
        for (int kc = 0; kc < 16; ++kc) s[pidx(q) + kc * (TPS + TPS / 8)] = v[vt][kc];
      }
    } else {
      auto mid = [&]() { if constexpr (!AHEAD2) { if (more) fetch(blk + gridDim.y); } };
      bwd_passes_w<LOG2M, WPS, VT, false, true, decltype(mid), PairSync>(v, s, ql, tw1, tw2, &rtw, mid, psp);
    }
    __syncthreads();  // all sequences of the workgroup are in the LDS, one pass short of natural order
    // every wave is past the unpack: refill the stage with the next block's rows now, i.e. BEFORE this
    // block's stores are queued (vmcnt retires in order: a later wait for these loads would drain the stores)
    if (more) refill();
    if constexpr (AHEAD2) {
      if (blk + 2 * (int)gridDim.y < nblk) fetch(blk + 2 * gridDim.y);
    }

    // ---- last backward pass with a remapped assignment: lanes = (branch gi, time index p), so that the
    //      16 outputs of a lane, x[a*TPS + p] of branch gi, are the [t][gi] rows of the spill layout: every
    //      store instruction writes 512 contiguous bytes straight from registers (no LDS transposition)
    if constexpr (PAIRED) {
      constexpr int H = G / 2, PPW = 64 / H;            // branch pairs; time indices per wave
      const int g2 = lane & (H - 1), pl = lane / H;
      const int pp = wave * PPW + pl;
      const int GL = p.g;
      const int lgrp = (grp * G) / GL, sub = (grp * G) % GL;
      cf* dst = p.spill + ((uint64_t)blk * (uint64_t)(p.c2 / GL) + lgrp) * p.gs + sub;   // wave-uniform
      const cf* sa = lds + (2 * g2) * SEQ + pidx(pp);
      const cf* sb = sa + SEQ;
      cf ua[16], ub[16];
#pragma unroll
      for (int ka = 0; ka < 16; ++ka) {
        ua[ka] = sa[ka * (TPS + TPS / 8)];
        ub[ka] = sb[ka * (TPS + TPS / 8)];
      }
#pragma unroll
      for (int ka = 1; ka < 16; ++ka) {   // one twiddle per ka for both branches (same time index)
        const cf w = (ka < 4) ? tlo0[ka] : (((ka & 3) == 0) ? thi0[ka >> 2] : mul(thi0[ka >> 2], tlo0[ka & 3]));
        ua[ka] = mulc(ua[ka], w);
        ub[ka] = mulc(ub[ka], w);
      }
      Dft<16, +1>::run(ua);
      Dft<16, +1>::run(ub);
      {
        // 16-byte stores: the 64 lanes of one instruction cover 16 rows x 64 bytes = 1 KB contiguous; half as many
        // entries in the CU's vector-memory queue as with one branch per lane
        if (p.tile_major == 2) {   // spill [blk][t/2][group][t%2][GL]: the K2 tile of two time samples is one contiguous run
          const uint32_t ng = (uint32_t)(p.c2 / GL);
          cf* dstT = p.spill + (uint64_t)blk * (uint64_t)ng * p.gs + (uint64_t)lgrp * (uint64_t)(2 * GL) + sub;
          const uint32_t loffT = (uint32_t)(pp >> 1) * (ng * 2u * (uint32_t)GL) + (uint32_t)((pp & 1) * GL + 2 * g2);
          const size_t strideT = (size_t)(TPS / 2) * (size_t)ng * (size_t)(2 * GL);
#pragma unroll
          for (int a = 0; a < 16; ++a) store_spill(reinterpret_cast<cf2*>(dstT + (size_t)a * strideT + loffT), ua[a], ub[a]);
        } else {
        const uint32_t loff = (uint32_t)(pp * GL + 2 * g2);
#pragma unroll
        for (int a = 0; a < 16; ++a) store_spill(reinterpret_cast<cf2*>(dst + (size_t)a * (size_t)(TPS * GL) + loff), ua[a], ub[a]);
        }
      }
    } else {
      constexpr int PPW = 64 / G;                       // time indices per wave and sweep
      constexpr int NSW = TPS / (NW * PPW);             // sweeps per wave
      static_assert(NSW >= 1 && NSW * NW * PPW == TPS, "remapped last pass does not tile the sequence");
      const int gi = lane & (G - 1), pl = lane / G;
      const int GL = p.g;
      const int lgrp = (grp * G) / GL, sub = (grp * G) % GL;
      cf* dst = p.spill + ((uint64_t)blk * (uint64_t)(p.c2 / GL) + lgrp) * p.gs + sub;   // wave-uniform
      const cf* sg_ = lds + gi * SEQ;
      // vmcnt retires loads and stores in issue order: a wait for a load issued after a store would also
      // wait for that store to complete.  So the twiddles of the NEXT sweep are fetched and drained before
      // the stores of the current sweep are queued; nothing in this iteration waits behind a store.
      // base twiddles of this lane's time index: tlo[j] = W^(j*pp), thi[i] = W^(4i*pp); W^(ka*pp) for the other
      // ka is one product thi[ka>>2] * tlo[ka&3].  The next sweep (pp + PPW) is reached by multiplying the six
      // bases with wave-uniform constants from the kernel arguments: no global load follows a store.
      cf tlo[4], thi[4];
#pragma unroll
      for (int j = 1; j < 4; ++j) {
        tlo[j] = tlo0[j];
        thi[j] = thi0[j];
      }
#pragma unroll 1
      for (int sw = 0; sw < NSW; ++sw) {
        const int pp = (wave * NSW + sw) * PPW + pl;
        cf u[16];
#pragma unroll
        for (int ka = 0; ka < 16; ++ka) u[ka] = sg_[pidx(pp) + ka * (TPS + TPS / 8)];
        if constexpr (!COH) {
#pragma unroll
        for (int ka = 1; ka < 16; ++ka) {
          const cf w = (ka < 4) ? tlo[ka] : (((ka & 3) == 0) ? thi[ka >> 2] : mul(thi[ka >> 2], tlo[ka & 3]));
          u[ka] = mulc(u[ka], w);
        }
        Dft<16, +1>::run(u);
        }
        if (!COH && sw + 1 < NSW) {
#pragma unroll
          for (int j = 1; j < 4; ++j) {
            tlo[j] = mul(tlo[j], p.rot6[j - 1]);
            thi[j] = mul(thi[j], p.rot6[2 + j]);
          }
        }
        {
          // 8-byte stores, 512 contiguous bytes per instruction.  Pairing lanes (v_permlane32_swap) into 16-byte
          // stores was measured slower (2.26 vs 2.05 ms): the limit is bytes per clock on the CU's write path
          // (~16 B/clk, the same with a cache-resident target), not the number of store instructions.
          // wave-uniform row base (scalar registers) + one 32-bit lane offset shared by the 16 stores
          if (LOG2M >= 5 && p.tile_major == 8) {   // chunks of eight time samples [blk][t/8][group][t%8][GL], t = a*TPS + pp: 64 lanes = 4 lines of 128 bytes
            const uint32_t ng = (uint32_t)(p.c2 / GL);
            cf* dst8 = p.spill + (uint64_t)blk * (uint64_t)ng * p.gs + (uint64_t)lgrp * (uint64_t)(8 * GL) + sub;
            const uint32_t loff8 = (uint32_t)(pp >> 3) * (ng * 8u * (uint32_t)GL) + (uint32_t)((pp & 7) * GL + gi);
            const size_t stride8 = (size_t)(TPS / 8) * (size_t)ng * (size_t)(8 * GL);
#pragma unroll
            for (int a = 0; a < 16; ++a) store_spill(dst8 + (size_t)a * stride8 + loff8, u[a]);
          } else {
          const uint32_t loff = (uint32_t)(pp * GL + gi);
#pragma unroll
          for (int a = 0; a < 16; ++a) store_spill(dst + (size_t)a * (size_t)(TPS * GL) + loff, u[a]);
          }
        }
      }
    }
    // (behind the row stores: in front of the sweep loop the compiler drains vmcnt, and a store waited for there costs
    // its round trip to the L2 in every block)
    if (ql == 0) p.s_dc[(uint64_t)blk * p.c2 + n1] = sdc;
    __syncthreads();  // the LDS images are consumed: the next block may overwrite them
  }
}

// PM: 2 = Stokes I (-d1), 4 = coherency products (-d4), 0 = the single-product modes decided at run time
// MSTAT: four products with the rescale statistics summed in the kernel (a thread owns several column groups: 32 more
// registers, one wave less per SIMD; used only while a rescale interval is being measured)
template <int LOG2M, int NW, int PM, int WPS = 1, bool MSTAT = false>
__global__ void __launch_bounds__(64 * NW, (LOG2M >= 5 ? 1 : ((WPS > 1 && LOG2M < 4 && !MSTAT) ? 3 : 2))) frbch_k2_wave(KParams p) {
  using GE = GeoW<LOG2M, WPS>;
  constexpr int M = GE::M, C2 = GE::L, C = C2 / 2, TPS = GE::TPS, SEQ = GE::SEQ, LPS = GE::LPS, VT = GE::VT, SPW = GE::SPW;
  constexpr int NT = 64 * NW;
  constexpr int TT = (NW / WPS) * SPW;
  constexpr int ROT = 32 / M;
  constexpr int NIF = PM == 4 ? 4 : 1;
  constexpr int NCOL = NIF * C;
  constexpr int NLD = TT * C2 / 2 / NT;      // 16-B pieces of the tile per thread
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int ql = WPS > 1 ? (wave % WPS) * 64 + lane : lane % LPS;   // (the loop body derives its own copies from the laundered thread index)
  __builtin_assume(ql >= 0 && ql < LPS);
  // all sizes are powers of two: shifts instead of divisions
  const int lg_g = p.log2_g;                       // log2(G1), G1 = branches per K1 workgroup
  const int lg_h = lg_g - 1;                       // 16-B pairs per (group, t) row
  const int lg_ppg = lg_h + (31 - __builtin_clz(TT));   // pairs per group in this tile
  const int R = p.r;
  // Persistent over the tiles of the launch (tile = TT rows of one block): while a tile is transformed the
  // next one is already on its way from HBM into registers, so every resident workgroup keeps 16 B x NLD x NT
  // in flight all the time (one shot per workgroup left the memory system idle during the transforms).
  const int lg_tpb = p.log2_r - (31 - __builtin_clz(TT));          // log2(tiles per block)
  const uint32_t ntiles = p.nblk << lg_tpb;
  // chunks of eight time samples (spill [blk][t/8][group][t%8][G1], written by frbch_k1_fast<5>; 2C = 8192): the 8/TT
  // neighbouring tiles of a chunk read TT*16-byte pieces of the same lines, so they must run on ONE XCD at about the same
  // time -- workgroup slots go round-robin over the XCDs, hence the XCD bits [2:0] of the slot index move above the
  // tile-in-chunk bits
  const bool chunk8 = LOG2M >= 5 && p.tile_major == 8;
  constexpr int CB = TT >= 8 ? 0 : (TT == 4 ? 1 : (TT == 2 ? 2 : 3));   // log2(tiles per chunk)
  auto tile_of = [&](uint32_t idx) {
    return chunk8 ? ((idx & ~((8u << CB) - 1u)) | ((idx & 7u) << CB) | ((idx >> 3) & ((1u << CB) - 1u))) : idx;
  };
  uint32_t slot = blockIdx.x;
  if (slot >= ntiles) return;
  uint32_t tile = tile_of(slot);

  // The tile is TT rows x 2C branches = NLD*NT 16-byte pieces (2 branches each).  Piece id = tid + NT*i:
  // the NT pieces of one trip cover 2*NT/TT consecutive branches, whatever the group size, so only
  // trip 0 needs index arithmetic: every later trip is a uniform step in HBM and a constant step in LDS.
  constexpr int INC = 2 * NT / TT;                   // branches per trip
  static_assert(INC % 16 == 0, "LDS step must keep the 16-point padding phase");
  const uint32_t grp_stride = chunk8 ? (4u << lg_g) : (uint32_t)(p.gs >> 1);     // 16-B units between consecutive groups
  const int grp0 = tid >> lg_ppg, rem = tid & ((1 << lg_ppg) - 1);
  const bool tile_major = TT == 2 && p.tile_major == 2;   // spill [blk][t/2][group][t%2][GL] (written by the paired-branch K1): this tile is one run of 16*C2 bytes
  const uint32_t voff = tile_major ? (uint32_t)tid * 16u : ((uint32_t)grp0 * grp_stride + (uint32_t)rem) * 16u;      // bytes inside the block's slab (< 8N)
  const uint64_t step = tile_major ? (uint64_t)NT * 16u : (uint64_t)(NT >> lg_ppg) * (uint64_t)grp_stride * 16u;    // uniform
  cf* const dst0 = lds + (rem >> lg_h) * SEQ + pidx((grp0 << lg_g) + 2 * (rem & ((1 << lg_h) - 1)));
  cf2 buf[NLD];
  auto fetch_base = [&](uint32_t tl) {
    const uint32_t b_ = tl >> lg_tpb, t_ = (tl & ((1u << lg_tpb) - 1)) * TT;
    return reinterpret_cast<const char*>(p.spill + ((uint64_t)b_ * (uint64_t)(C2 >> lg_g)) * p.gs +
                                         (tile_major ? (uint64_t)(t_ >> 1) * (uint64_t)(2 * C2)
                                          : chunk8 ? ((uint64_t)(t_ >> 3) * (uint64_t)(8 * C2) + ((uint64_t)(t_ & 7u) << lg_g))
                                                   : ((uint64_t)t_ << lg_g)));
  };
  auto fetch_part = [&](const char* base, int i0, int i1) {   // pieces [i0, i1) of the tile at `base`
#pragma unroll
    for (int i = 0; i < NLD; ++i) {   // streamed once: non-temporal (not at 2C = 8192: neighbouring tiles share the lines)
      if (i < i0 || i >= i1) continue;
      nf4 t4;
      if constexpr (LOG2M >= 5) t4 = *reinterpret_cast<const nf4*>(base + (uint64_t)i * step + voff);
      else t4 = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(base + (uint64_t)i * step + voff));
      buf[i] = cf2{cf{t4.x, t4.y}, cf{t4.z, t4.w}};
    }
  };
  auto fetch = [&](uint32_t tl) { fetch_part(fetch_base(tl), 0, NLD); };
  // 32 points per lane at 2C <= 4096 (16 waves per CU): no registers left for a second tile.  2C = 8192 runs eight waves per
  // CU (the LDS holds two images): 256 registers, and the radix-32 pass occupies exactly one virtual thread per lane
  // SPREAD: the prefetch is requested two pieces at a time from hooks inside the transform instead of in one go -- a wave
  // that issues many loads at once sits in the issue stage until the CU's memory pipe has taken them all (2C = 8192, 16
  // scattered pieces per lane: for the whole gather; 2C = 2048: K2 1.21 -> 1.17 ms)
  constexpr bool SPREAD = LOG2M >= 5 && NLD == 16;
  constexpr bool SPREAD3 = LOG2M == 3 && WPS == 2 && VT == 1 && NLD == 8;   // hooks 0, 1, 2 inside the passes, 3 behind them
  // (2C = 4096, 32 points per lane, with a spread prefetch: measured no gain, 1.97 ms either way)
  constexpr bool PREFETCH = VT == 1 || LOG2M >= 5;
  if constexpr (PREFETCH) fetch(tile);
  // vmcnt retires in issue order: any vector-memory load issued after the prefetch would make its wait a
  // wait for the prefetched tile too.  So the loop body issues none after it: the twiddles come from
  // loop-invariant base factors in registers, dP of the current tile is requested BEFORE the prefetch, and
  // (one column group per thread) the frozen offset/scale are loaded once, up here.
  RegTw<LOG2M, VT> rtw;
  rtw.load(p.ftw1_c, p.ftw2_c, ql, LPS, TPS);
  if constexpr (LOG2M >= 5) {   // the radix-32 twiddles behind the image (visible after the first barrier of the loop)
    cf* tl = lds + TT * SEQ;
    for (int i = tid; i < M * 16; i += NT) tl[i] = p.ftw2_c[i];
    rtw.tl = tl + (ql & 15);
  }
  constexpr bool FIXED_COLS = (NCOL / 4 <= NT) && (NT % (NCOL / 4) == 0);
  // The same eight registers serve both output modes.  Codes: the frozen offset / scale of this thread's four
  // columns.  Float power while a rescale interval is measured: running sum and sum of squares of those columns
  // over all rows this workgroup emits below p.stat_limit (A9 fused: no second pass over the power buffer).
  float4 of4_fix = make_float4(0.f, 0.f, 0.f, 0.f), sc4_fix = make_float4(0.f, 0.f, 0.f, 0.f);
  // More column groups than threads (four products): a thread owns CGT = NCOL/4/NT groups, tid + NT*g, and keeps their
  // running sums too (codes mode then loads offset / scale per group as before)
  constexpr bool MULTI_COLS = MSTAT && (NCOL / 4 > NT) && ((NCOL / 4) % NT == 0) && (NCOL / 4 / NT <= 4);
  constexpr int CGT = MULTI_COLS ? NCOL / 4 / NT : 1;
  float4 macc1[CGT], macc2[CGT];
#pragma unroll
  for (int g = 0; g < CGT; ++g) macc1[g] = macc2[g] = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool stat_on = (FIXED_COLS || MULTI_COLS) && p.out_mode == FRBCH_OUT_FLOAT_POWER && p.stat_partial != nullptr;
  if (FIXED_COLS && p.out_mode != FRBCH_OUT_FLOAT_POWER) {
    const int col0 = (tid % (NCOL / 4)) * 4, prod = col0 / C, cout0 = col0 - prod * C;
    const int kbase = p.flip ? (C - 4 - cout0) : cout0;
    of4_fix = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
    sc4_fix = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
  }
  if (MULTI_COLS && p.out_mode != FRBCH_OUT_FLOAT_POWER) {   // codes: the sum registers hold the frozen offset / scale instead
#pragma unroll
    for (int g = 0; g < CGT; ++g) {
      const int col0 = (tid + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
      const int kbase = p.flip ? (C - 4 - cout0) : cout0;
      macc1[g] = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
      macc2[g] = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
    }
  }

  const int tid_outer = tid;
  for (;;) {
  // 2C = 8192: the thread index is laundered per trip -- the compiler would otherwise hold every per-lane LDS offset of the
  // body (pass strides, mirror slots, 16 swizzled power columns) in registers across the loop, beside the prefetched tile
  int tid_l = tid_outer;
  if constexpr (LOG2M >= 5) asm volatile("" : "+v"(tid_l));
  const int tid = tid_l, lane = tid & 63, wave = tid >> 6;
  const int seq = WPS > 1 ? wave / WPS : wave * SPW + lane / LPS;
  const int ql = WPS > 1 ? (wave % WPS) * 64 + lane : lane % LPS;
  __builtin_assume(ql >= 0 && ql < LPS);
  const int blk = (int)(tile >> lg_tpb);
  const int t0 = (int)(tile & ((1u << lg_tpb) - 1)) * TT;
  if constexpr (!PREFETCH) fetch(tile);
#pragma unroll
  for (int i = 0; i < NLD; ++i) *reinterpret_cast<cf2*>(dst0 + i * (INC + INC / 8)) = buf[i];
  __syncthreads();
  cf dpv[VT][8];
  auto load_dp = [&]() {
    const cf* dP = p.p0 + (size_t)blk * C2;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const int q = ql + LPS * vt;
      const int k0 = (q / M) + 16 * (q % M);
#pragma unroll
      for (int i = 0; i < 8; ++i) dpv[vt][i] = dP[k0 + TPS * (8 + i)];
    }
  };
  // 2C = 8192: no registers for dP beside the prefetched tile during the transform -- requested behind it (the wait then
  // covers the prefetch as well, which was issued a whole transform earlier)
  constexpr bool DP_LATE = false;
  if constexpr (!DP_LATE) load_dp();
  const uint32_t next_slot = slot + gridDim.x;
  const uint32_t next = tile_of(next_slot);
  // unconditional (the last trip fetches its own tile again): behind a branch the compiler's wait-count bookkeeping merges
  // the "no prefetch in flight" path into every later s_waitcnt -- the wait for dP then waited for the whole prefetch
  const char* const pf_base = fetch_base(next_slot < ntiles ? next : tile);
  if constexpr (PREFETCH && !SPREAD && !SPREAD3) fetch_part(pf_base, 0, NLD);
  auto pf_hook = [&](int n) { fetch_part(pf_base, 2 * n, 2 * n + 2); };   // hooks 0..6 inside the passes, 7 behind them

  float* pw = reinterpret_cast<float*>(lds);
  {
  cf* s = lds + seq * SEQ;
  cf v[VT][16];
  if constexpr (LOG2M >= 5) {
    if constexpr (SPREAD) {
      fwd_passes_w<LOG2M, WPS, VT, true, WgSync, true>(v, s, ql, p.ftw1_c, p.ftw2_c, &rtw, (WgSync*)nullptr, pf_hook);
      __builtin_amdgcn_sched_barrier(0);
      pf_hook(7);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      fwd_passes_w<LOG2M, WPS, VT, true, WgSync, true>(v, s, ql, p.ftw1_c, p.ftw2_c, &rtw);
    }
  } else {
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
#pragma unroll
    for (int a = 0; a < 16; ++a) v[vt][a] = s[pidx(q) + a * (TPS + TPS / 8)];
  }
  if constexpr (SPREAD3) {
    fwd_passes_w<LOG2M, WPS, VT, true, WgSync, false>(v, s, ql, p.ftw1_c, p.ftw2_c, &rtw, (WgSync*)nullptr, pf_hook);
    __builtin_amdgcn_sched_barrier(0);
    pf_hook(3);
    __builtin_amdgcn_sched_barrier(0);
  } else {
  fwd_passes_w<LOG2M, WPS, VT, true>(v, s, ql, p.ftw1_c, p.ftw2_c, &rtw);
  }
  }
  if constexpr (DP_LATE) load_dp();

  // mirror exchange inside the wave (partner virtual thread TPS-1-q belongs to the same sequence)
#pragma unroll
  for (int vt = 0; vt < VT; ++vt) {
    const int q = ql + LPS * vt;
    if constexpr (LOG2M >= 5) {   // the last pass here, one virtual thread at a time (a thread's 16 points are its own LDS row)
      if (vt) __builtin_amdgcn_sched_barrier(0);
      const cf2* src = reinterpret_cast<const cf2*>(s + q * 18);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const cf2 t = src[i];
        v[vt][2 * i] = t.a;
        v[vt][2 * i + 1] = t.b;
      }
      Dft<16, -1>::run(v[vt]);
    }
    cf2* dst = reinterpret_cast<cf2*>(s + q * 18 + 8);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const cf a = add(v[vt][8 + 2 * i], dpv[vt][2 * i]);
      const cf b = add(v[vt][9 + 2 * i], dpv[vt][2 * i + 1]);
      dst[i] = cf2{a, b};
    }
  }
  if constexpr (WPS > 1) __syncthreads();   // the partner may live in the other wave of the sequence
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
  __syncthreads();  // all waves are done with the FFT image: re-use the LDS for the power rows

  {
    float* row = pw + (size_t)seq * NCOL;
    const int pm = p.pol_mode;
#pragma unroll
    for (int vt = 0; vt < VT; ++vt) {
      const int q = ql + LPS * vt;
      const int k0 = (q / M) + 16 * (q % M);
#pragma unroll
      for (int kc = 0; kc < 8; ++kc) {
        const int k = k0 + TPS * kc;
        const cf wk = v[vt][kc];
        const cf d = cf{wm[vt][kc].x, -wm[vt][kc].y};
        const int ks = pw_swz(k, ROT);
        if constexpr (PM == 2) {
          row[ks] = 0.5f * ((wk.x * wk.x + wk.y * wk.y) + (d.x * d.x + d.y * d.y));
        } else if constexpr (PM == 4) {
          // pol0 = (wk + d) / 2, pol1 = -i (wk - d) / 2.  With s1 = |wk|^2, s2 = |d|^2, c = wk d* the four products need neither
          // polarisation spelled out (12 operations per channel instead of 20); the SAME expressions, in the same order, as
          // frbch_k2_priv (kernels_k2priv.inc): the two K2 families of 2C = 2048 produce bit-identical floats
          //   PP = (s1 + s2) / 4 + Re c / 2,  QQ = (s1 + s2) / 4 - Re c / 2,  PQ* = Im c / 2 + i (s1 - s2) / 4
          //   I = (s1 + s2) / 2,  Q = 2 Re PQ* = Im c,  U = 2 Im PQ* = (s1 - s2) / 2,  V = PP - QQ = Re c
          const float s1 = wk.x * wk.x + wk.y * wk.y, s2 = d.x * d.x + d.y * d.y;
          const float cr = wk.x * d.x + wk.y * d.y, ci = wk.y * d.x - wk.x * d.y;
          if (pm == 5) {   // Stokes I, Q, U, V of circular feeds (wave-uniform: a branch, not eight selects per channel)
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
      }
    }
  }
  }
  __syncthreads();

  {
    const int lg_t = 31 - __builtin_clz(p.tscr);
    const int T = 1 << lg_t;
    const int rows_here = TT >> lg_t;
    const uint64_t row_base = p.row0 + (uint64_t)blk * (uint64_t)(R >> lg_t) + (uint64_t)(t0 >> lg_t);
    const int flip = p.flip;
    const int om = p.out_mode, nbit = p.nbit;
    auto emit = [&](const int id, float4& a1, float4& a2) {
      const int rr = id / (NCOL / 4);
      const int col0 = (id - rr * (NCOL / 4)) * 4;
      const int prod = col0 / C;
      const int cout0 = col0 - prod * C;
      float sv[4];
      float lin[4] = {0.f, 0.f, 0.f, 0.f};   // the group in the order it lies in the LDS (input channel order), ROT % 4 == 0 only
      if constexpr (ROT % 4 == 0) {
        // the swizzle rotates 32-channel groups by multiples of 4: an aligned group of 4 channels stays one 16-B piece
        const int kb = flip ? (C - 4 - cout0) : cout0;
        const float* src = pw + (size_t)(rr << lg_t) * NCOL + prod * C + pw_swz(kb, ROT);
        float4 acc = *reinterpret_cast<const float4*>(src);
        for (int tt = 1; tt < T; ++tt) {
          const float4 x = *reinterpret_cast<const float4*>(src + (size_t)tt * NCOL);
          acc.x += x.x; acc.y += x.y; acc.z += x.z; acc.w += x.w;
        }
        lin[0] = acc.x; lin[1] = acc.y; lin[2] = acc.z; lin[3] = acc.w;
        sv[0] = flip ? acc.w : acc.x;
        sv[1] = flip ? acc.z : acc.y;
        sv[2] = flip ? acc.y : acc.z;
        sv[3] = flip ? acc.x : acc.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int cout = cout0 + e;
          const int k = flip ? (C - 1 - cout) : cout;
          const int ks = pw_swz(k, ROT);
          float acc = 0.0f;
          for (int tt = rr << lg_t; tt < ((rr + 1) << lg_t); ++tt) acc += pw[(size_t)tt * NCOL + prod * C + ks];
          sv[e] = acc;
        }
      }
      const uint64_t o = (row_base + rr) * (uint64_t)NCOL + col0;
      const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, row_base + rr, NIF, prod, cout0);
      if constexpr (ROT % 4 == 0) {
        if (om != FRBCH_OUT_FLOAT_POWER && nbit == 8) {
          // 8-bit codes: rescale in the order the row lies in the LDS (= the order of offset / scale: input channels); a flipped
          // band only reverses the four bytes of the word, which the pack instruction does by its byte select -- no selects per
          // value (12 v_cndmask per group of four before)
          const int kbase = flip ? (C - 4 - cout0) : cout0;
          const float4 of4 = (FIXED_COLS || MULTI_COLS) ? a1 : *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
          const float4 sc4 = (FIXED_COLS || MULTI_COLS) ? a2 : *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
          const float x[4] = {FMUL_RN(FADD_RN(lin[0], of4.x), sc4.x), FMUL_RN(FADD_RN(lin[1], of4.y), sc4.y),
                              FMUL_RN(FADD_RN(lin[2], of4.z), sc4.z), FMUL_RN(FADD_RN(lin[3], of4.w), sc4.w)};
          *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale, flip != 0);
          return;
        }
      }
      if (om == FRBCH_OUT_FLOAT_POWER) {
        {   // read again only by the statistics / digitiser passes, gigabytes later: non-temporal (K2 -1.5 %, digitiser -2 %)
          const nf4 t4 = {sv[0], sv[1], sv[2], sv[3]};
          __builtin_nontemporal_store(t4, reinterpret_cast<nf4*>(p.power_out + o));
        }
        if (stat_on && row_base + rr < p.stat_limit) {
          a1.x += sv[0]; a1.y += sv[1]; a1.z += sv[2]; a1.w += sv[3];
          a2.x = fmaf(sv[0], sv[0], a2.x); a2.y = fmaf(sv[1], sv[1], a2.y);
          a2.z = fmaf(sv[2], sv[2], a2.z); a2.w = fmaf(sv[3], sv[3], a2.w);
        }
      } else {
        // four consecutive channels (descending when flipped): one 16-byte load of offset and of scale
        const int kbase = flip ? (C - 4 - cout0) : cout0;
        const float4 of4 = (FIXED_COLS || MULTI_COLS) ? a1 : *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
        const float4 sc4 = (FIXED_COLS || MULTI_COLS) ? a2 : *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
        const float ofv[4] = {of4.x, of4.y, of4.z, of4.w}, scv[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
        float x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = FMUL_RN(FADD_RN(sv[e], ofv[flip ? 3 - e : e]), scv[flip ? 3 - e : e]);
        if (nbit == -32) {
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.code_out) + oc) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
          if (nbit == 8) {
            *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale);
          } else {
            uint32_t code[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) code[e] = digitise(x[e], p.digi_mean, p.digi_scale, p.digi_max);
            if (nbit == 16)
              *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.code_out) + oc) =
                  make_uint2(code[0] | (code[1] << 16), code[2] | (code[3] << 16));
            else
              p.code_out[oc >> 2] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
          }
        }
      }
    };
    // 8-bit codes or float power with the tile's time samples either kept apart (no tscrunch) or all summed into one row (tscrunch =
    // the tile's height): the tile's groups of a thread in three sweeps -- every LDS read requested first, then the arithmetic, then
    // the stores.  (The general form below waits for each read where it is issued and walks a chain of mode branches per group: a
    // quarter of this kernel's time with four products.)  Sums run over the time samples in ascending order, as there.
    const bool sweeps = ROT % 4 == 0 && (lg_t == 0 || (1 << lg_t) == TT) &&
                        (om == FRBCH_OUT_FLOAT_POWER || nbit == 8);
    const int nr = lg_t == 0 ? TT : 1;            // output rows of the tile on that path
    if constexpr (MULTI_COLS) {
      bool done = false;
      if constexpr (ROT % 4 == 0) {
        if (sweeps) {
          float4 accs[TT * CGT];
#pragma unroll
          for (int e8 = 0; e8 < TT * CGT; ++e8) {
            const int tt = e8 / CGT, g = e8 % CGT;
            const int col0 = (tid + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
            const int kb = flip ? (C - 4 - cout0) : cout0;
            accs[e8] = *reinterpret_cast<const float4*>(pw + (size_t)tt * NCOL + prod * C + pw_swz(kb, ROT));
          }
          if (nr == 1) {
#pragma unroll
            for (int tt = 1; tt < TT; ++tt)
#pragma unroll
              for (int g = 0; g < CGT; ++g) {
                accs[g].x += accs[tt * CGT + g].x; accs[g].y += accs[tt * CGT + g].y;
                accs[g].z += accs[tt * CGT + g].z; accs[g].w += accs[tt * CGT + g].w;
              }
          }
#pragma unroll
          for (int e8 = 0; e8 < TT * CGT; ++e8) {
            const int rr = e8 / CGT, g = e8 % CGT;
            if (rr >= nr) continue;
            const int col0 = (tid + NT * g) * 4, prod = col0 / C, cout0 = col0 - prod * C;
            const float4 a = accs[e8];
            if (om != FRBCH_OUT_FLOAT_POWER) {
              const float4 of4 = macc1[g], sc4 = macc2[g];
              const float x[4] = {FMUL_RN(FADD_RN(a.x, of4.x), sc4.x), FMUL_RN(FADD_RN(a.y, of4.y), sc4.y),
                                  FMUL_RN(FADD_RN(a.z, of4.z), sc4.z), FMUL_RN(FADD_RN(a.w, of4.w), sc4.w)};
              const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, row_base + rr, NIF, prod, cout0);
              *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale, flip != 0);
            } else {
              const nf4 t4 = {flip ? a.w : a.x, flip ? a.z : a.y, flip ? a.y : a.z, flip ? a.x : a.w};
              __builtin_nontemporal_store(t4, reinterpret_cast<nf4*>(p.power_out + (row_base + rr) * (uint64_t)NCOL + col0));
              if (stat_on && row_base + rr < p.stat_limit) {
                macc1[g].x += t4.x; macc1[g].y += t4.y; macc1[g].z += t4.z; macc1[g].w += t4.w;
                macc2[g].x = fmaf(t4.x, t4.x, macc2[g].x); macc2[g].y = fmaf(t4.y, t4.y, macc2[g].y);
                macc2[g].z = fmaf(t4.z, t4.z, macc2[g].z); macc2[g].w = fmaf(t4.w, t4.w, macc2[g].w);
              }
            }
          }
          done = true;
        }
      }
      if (!done)
      for (int rr = 0; rr < rows_here; ++rr) {
#pragma unroll
        for (int g = 0; g < CGT; ++g) emit(tid + NT * (rr * CGT + g), macc1[g], macc2[g]);
      }
    } else {
      bool done = false;
      if constexpr (FIXED_COLS && ROT % 4 == 0 && (TT * (NCOL / 4)) % NT == 0 && TT * (NCOL / 4) >= NT) {
        constexpr int NE = TT * (NCOL / 4) / NT;   // groups of this thread per tile: the same column group in NE time samples
        constexpr int RSTEP = NT / (NCOL / 4);     // ... RSTEP apart (1: the thread holds the column group of every time sample)
        if (sweeps && (nr == TT || RSTEP == 1)) {
          float4 accs[NE];
          const int cgi = tid % (NCOL / 4), rr0 = tid / (NCOL / 4);
          const int col0 = cgi * 4, prod = col0 / C, cout0 = col0 - prod * C;
          const int kb = flip ? (C - 4 - cout0) : cout0;
#pragma unroll
          for (int e8 = 0; e8 < NE; ++e8)
            accs[e8] = *reinterpret_cast<const float4*>(pw + (size_t)(rr0 + e8 * RSTEP) * NCOL + prod * C + pw_swz(kb, ROT));
          if (nr == 1) {
#pragma unroll
            for (int e8 = 1; e8 < NE; ++e8) {
              accs[0].x += accs[e8].x; accs[0].y += accs[e8].y; accs[0].z += accs[e8].z; accs[0].w += accs[e8].w;
            }
          }
#pragma unroll
          for (int e8 = 0; e8 < NE; ++e8) {
            if (nr == 1 && e8 > 0) continue;
            const uint64_t row = row_base + (nr == 1 ? 0 : rr0 + e8 * RSTEP);
            const float4 a = accs[e8];
            if (om != FRBCH_OUT_FLOAT_POWER) {
              const float x[4] = {FMUL_RN(FADD_RN(a.x, of4_fix.x), sc4_fix.x), FMUL_RN(FADD_RN(a.y, of4_fix.y), sc4_fix.y),
                                  FMUL_RN(FADD_RN(a.z, of4_fix.z), sc4_fix.z), FMUL_RN(FADD_RN(a.w, of4_fix.w), sc4_fix.w)};
              const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, row, NIF, prod, cout0);
              *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale, flip != 0);
            } else {
              const nf4 t4 = {flip ? a.w : a.x, flip ? a.z : a.y, flip ? a.y : a.z, flip ? a.x : a.w};
              __builtin_nontemporal_store(t4, reinterpret_cast<nf4*>(p.power_out + row * (uint64_t)NCOL + col0));
              if (stat_on && row < p.stat_limit) {
                of4_fix.x += t4.x; of4_fix.y += t4.y; of4_fix.z += t4.z; of4_fix.w += t4.w;
                sc4_fix.x = fmaf(t4.x, t4.x, sc4_fix.x); sc4_fix.y = fmaf(t4.y, t4.y, sc4_fix.y);
                sc4_fix.z = fmaf(t4.z, t4.z, sc4_fix.z); sc4_fix.w = fmaf(t4.w, t4.w, sc4_fix.w);
              }
            }
          }
          done = true;
        }
      }
      if (!done)
      for (int id = tid; id < rows_here * (NCOL / 4); id += NT) emit(id, of4_fix, sc4_fix);
    }
  }
  if (next_slot >= ntiles) break;
  __syncthreads();   // the power rows are consumed: the next tile may overwrite the LDS image
  slot = next_slot;
  tile = next;
  }
  if (MULTI_COLS && stat_on) {   // one row of partial sums per workgroup, CGT column groups per thread
#pragma unroll
    for (int g = 0; g < CGT; ++g) {
      double* dst = p.stat_partial + ((size_t)blockIdx.x * NCOL + (size_t)(tid + NT * g) * 4) * 2;
      const float s1[4] = {macc1[g].x, macc1[g].y, macc1[g].z, macc1[g].w}, s2[4] = {macc2[g].x, macc2[g].y, macc2[g].z, macc2[g].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dst[2 * e] += (double)s1[e];
        dst[2 * e + 1] += (double)s2[e];
      }
    }
  }
  if (FIXED_COLS && stat_on) {   // this workgroup's row of the partial sums: exclusive, so a plain read-modify-write
    constexpr int CGS = NCOL / 4;
    const int chunk = (int)blockIdx.x * (NT / CGS) + tid / CGS;
    double* dst = p.stat_partial + ((size_t)chunk * NCOL + (size_t)(tid % CGS) * 4) * 2;
    const float s1[4] = {of4_fix.x, of4_fix.y, of4_fix.z, of4_fix.w}, s2[4] = {sc4_fix.x, sc4_fix.y, sc4_fix.z, sc4_fix.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      dst[2 * e] += (double)s1[e];
      dst[2 * e + 1] += (double)s2[e];
    }
  }
}


// =================================================================================================
// Second stage of the two-stage tscrunch (tscrunch beyond the wave K2's tile: > 2 at 2C = 8192, > 4 at 4096, else > 8
// sequences): the wave K2 above ran with its largest tile per row into a scratch buffer (float, output column order);
// scr_fact consecutive rows of it make one output row: float power, or A9 + A10 with the frozen scale.
// grid-stride over groups of four columns, 256 threads.
// =================================================================================================
__global__ void __launch_bounds__(256) frbch_k2_scrunch(KParams p) {
  const int C = p.c, ncol = p.nif * C, cg = ncol / 4, flip = p.flip;
  const uint64_t ngroups = p.scr_rows * (uint64_t)cg;
  const int fact = (int)p.scr_fact;
  for (uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x; id < ngroups; id += (uint64_t)gridDim.x * 256) {
    const uint64_t row = id / (uint64_t)cg;
    const int col0 = (int)(id - row * (uint64_t)cg) * 4;
    const int prod = col0 / C, cout0 = col0 - prod * C;
    const float* src = p.scr_in + (row * (uint64_t)fact) * (uint64_t)ncol + col0;
    nf4 acc = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(src));
    for (int f = 1; f < fact; ++f) {
      const nf4 x = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(src + (size_t)f * ncol));
      acc += x;
    }
    const float sv[4] = {acc.x, acc.y, acc.z, acc.w};
    const uint64_t o = (p.row0 + row) * (uint64_t)ncol + col0;
    const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, p.row0 + row, p.nif, prod, cout0);
    if (p.out_mode == FRBCH_OUT_FLOAT_POWER) {
      __builtin_nontemporal_store(acc, reinterpret_cast<nf4*>(p.power_out + o));
    } else {
      const int kbase = flip ? (C - 4 - cout0) : cout0;
      const float4 of4 = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
      const float4 sc4 = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
      const float ofv[4] = {of4.x, of4.y, of4.z, of4.w}, scv[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
      float x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = FMUL_RN(FADD_RN(sv[e], ofv[flip ? 3 - e : e]), scv[flip ? 3 - e : e]);
      if (p.nbit == -32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.code_out) + oc) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
        if (p.nbit == 8) {
          *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale);
        } else {
          uint32_t code[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) code[e] = digitise(x[e], p.digi_mean, p.digi_scale, p.digi_max);
          if (p.nbit == 16)
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.code_out) + oc) =
                make_uint2(code[0] | (code[1] << 16), code[2] | (code[3] << 16));
          else
            p.code_out[oc >> 2] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
        }
      }
    }
  }
}

// =================================================================================================
// Lean digitiser of a buffered rescale interval, 8-bit codes (A9 + A10 of the first interval; frbch_quantise is the
// generic form): the same four separately rounded fp32 operations per value, as a pure stream.
//   * a thread keeps ONE group of four columns for the whole launch (threads = row phases x column groups): offset / scale
//     live in registers, every address is a wave-uniform base (scalar arithmetic) plus a per-lane 32-bit offset;
//   * U 16-byte loads in flight per thread, the loads of trip i + 1 requested before the arithmetic of trip i (a bare
//     stream reads fastest at 8 waves per CU with 8 loads in flight, tools/micro/stream_cus: 5.8 - 6.2 TB/s; at that
//     occupancy the kernel can also live on a small share of the CUs beside another kernel, DESIGN.md section 4b);
//   * floor(t + 0.5) with the sum EXACT (digitise() in kernels_generic.inc) is floor(RTN(t + 0.5)): rounding the sum
//     toward -infinity cannot cross an integer (integers below 2^24 are representable), so one v_add_f32 issued while
//     MODE.FP_ROUND says "toward -infinity" replaces fract / compare / select; v_cvt_pk_u8_f32 then clips, converts and
//     packs a value per instruction: it saturates (below 0 -> 0, above 255 and +inf -> 255, NaN -> 0) and rounds to nearest
//     EVEN (tools/micro/cvt_probe, measured on the MI355X), so it gets the integer v_floor leaves -- nothing to round.
// 7 VALU instructions per value (frbch_quantise: ~15).  Bit-identical to frbch_quantise (GPU test).
// grid: `grid_x` workgroups of NT threads with grid_x * NT = rphases * ncol / 4; rows r = phase, phase + rphases, ...
// (NT = 512 with an LDS reservation it never touches: one workgroup per CU, on CUs no wave K1 workgroup fits beside it)
// =================================================================================================
FI void quant8_two_groups(const nf4& a, const nf4& b, const float (&of)[4], const float (&sc)[4], float ds, float dm,
                          uint32_t& ca, uint32_t& cb) {
  float x[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[e] = FMUL_RN(FADD_RN(a[e], of[e]), sc[e]);
    x[4 + e] = FMUL_RN(FADD_RN(b[e], of[e]), sc[e]);
  }
  digitise8_u8(x, dm, ds, ca, cb);
}

template <int U, int NT = 256>
__global__ void __launch_bounds__(NT) frbch_quantise_fast(QuantParams p) {
  static_assert(U % 2 == 0, "groups are digitised two at a time");
  const uint32_t log2_cg = (uint32_t)p.log2_ncol - 2u;
  const uint32_t lin = blockIdx.x * (uint32_t)NT + threadIdx.x;
  const uint32_t cgi = lin & ((1u << log2_cg) - 1u), ph = lin >> log2_cg;
  const uint32_t RP = p.rphases;
  const int col = (int)(cgi * 4u), prod = col >> p.log2_c, cout = col & (p.c - 1);
  const int kb = p.flip ? (p.c - 4 - cout) : cout;
  const float4 of4 = *reinterpret_cast<const float4*>(p.offset + (prod << p.log2_c) + kb);
  const float4 sc4 = *reinterpret_cast<const float4*>(p.scale + (prod << p.log2_c) + kb);
  float of[4] = {of4.x, of4.y, of4.z, of4.w}, sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
  if (p.flip) {
    float t;
    t = of[0]; of[0] = of[3]; of[3] = t;
    t = of[1]; of[1] = of[2]; of[2] = t;
    t = sc[0]; sc[0] = sc[3]; sc[3] = t;
    t = sc[1]; sc[1] = sc[2]; sc[2] = t;
  }
  const float ds = p.digi_scale, dm = p.digi_mean;
  // byte offsets: lane part (32 bits) + wave-uniform step part (64 bits, scalar)
  const uint32_t in_lane = ph * ((uint32_t)p.ncol * 4u) + cgi * 16u;
  const uint32_t out_lane = (uint32_t)((ph * (uint32_t)p.nif + (uint32_t)prod) * p.pitch + (uint64_t)cout);
  const uint64_t in_step = (uint64_t)RP * (uint64_t)p.ncol * 4u;
  const uint64_t out_step = (uint64_t)RP * (uint64_t)p.nif * p.pitch;
  const char* const in = reinterpret_cast<const char*>(p.power);
  uint8_t* const out = p.out;
  const uint64_t nsteps = p.rows / RP;          // steps in which every row phase has a row
  const uint64_t ntrips = (nsteps / U) & ~1ull; // trips of U steps, an even number of them (two register sets, no copies)
  auto fetch = [&](nf4 (&x)[U], uint64_t trip) {
    const char* b = in + trip * (uint64_t)U * in_step;
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(b + (uint64_t)u * in_step + in_lane));
  };
  auto emit = [&](const nf4 (&x)[U], uint64_t trip) {
    uint8_t* b = out + trip * (uint64_t)U * out_step;
#pragma unroll
    for (int u = 0; u < U; u += 2) {
      uint32_t c0, c1;
      quant8_two_groups(x[u], x[u + 1], of, sc, ds, dm, c0, c1);
      __builtin_nontemporal_store(c0, reinterpret_cast<uint32_t*>(b + (uint64_t)u * out_step + out_lane));
      __builtin_nontemporal_store(c1, reinterpret_cast<uint32_t*>(b + (uint64_t)(u + 1) * out_step + out_lane));
    }
  };
  if (ntrips) {
    nf4 xa[U], xb[U];
    fetch(xa, 0);
    for (uint64_t trip = 0; trip < ntrips; trip += 2) {
      fetch(xb, trip + 1);
      emit(xa, trip);
      // (unconditional: a load behind a branch would merge "nothing in flight" into every later wait; the last trip
      // requests its own first half again)
      fetch(xa, trip + 2 < ntrips ? trip + 2 : trip);
      emit(xb, trip + 1);
    }
  }
  // the steps left over (fewer than 2 U) and the rows of a last, partial step: two at a time, checked per row
  for (uint64_t st = ntrips * U; st * RP < p.rows; st += 2) {
    const uint64_t r0 = st * RP + ph, r1 = r0 + RP;
    const bool v0 = r0 < p.rows, v1 = r1 < p.rows;
    nf4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
    if (v0) x0 = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(in + st * in_step + in_lane));
    if (v1) x1 = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(in + (st + 1) * in_step + in_lane));
    uint32_t c0, c1;
    quant8_two_groups(x0, x1, of, sc, ds, dm, c0, c1);
    if (v0) __builtin_nontemporal_store(c0, reinterpret_cast<uint32_t*>(out + st * out_step + out_lane));
    if (v1) __builtin_nontemporal_store(c1, reinterpret_cast<uint32_t*>(out + (st + 1) * out_step + out_lane));
  }
}

// =================================================================================================
// Coherent dedispersion inside the filterbank (-D <dm> -F C:D, process_vdif.py:177-180), register-pass kernels.
// K1 (frbch_k1_fast, coherent mode) leaves the delayed branch spectra A'[n1][pos]; K2c turns the 2C branches into
// 2C channel rows and multiplies by the kernel; K3 brings the rows k and 2C-1-k back to the time domain, separates
// the polarisations, detects, drops the overlap-save margins and scrunches (K4, generic, makes time-major rows).
// =================================================================================================
// K2c: one workgroup = TT = NT/TPS consecutive positions x all 2C branches, for EVERY block of the launch (round 4: the workgroup
// keeps its positions and walks the blocks -- the kernel factors of its tile, 8 B per sample of table traffic that every (tile, block)
// workgroup used to fetch again, are loaded once and stay in registers: 24 -> 16.4 B per sample at 19 blocks per launch).
// grid (R/TT, <= nblk): blockIdx.y strides over the blocks.  LDS TT*SEQ cf.
template <int LOG2M, int NT>
__global__ void __launch_bounds__(NT) frbch_k2c_fast(KParams p) {
  using GE = Geo<LOG2M>;
  constexpr int M = GE::M, C2 = GE::L, TPS = GE::TPS;
  constexpr int SEQ = LOG2M >= 5 ? GE::L + GE::L / 8 : GE::SEQ;
  constexpr int TT = NT / TPS;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x;
  const int seq = tid / TPS, q = tid % TPS;
  const int G1 = p.g, R = p.r;
  const int ngrp = C2 / G1;
  const int ntile_ = gridDim.x;
  const int tile = (ntile_ % 8 == 0) ? (int)(blockIdx.x % 8) * (ntile_ / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int pos0 = tile * TT;
  const int pairs_per_grp = TT * G1 / 2;
  const bool whole_lines = pairs_per_grp >= 8;   // a group's piece of this tile is at least one 128-byte line
  constexpr int NLD = TT * C2 / 2 / NT;
  // four channels x one position per item: consecutive items walk the TT positions of one channel group, i.e.
  // 32*TT contiguous bytes of the grouped layout, in the kernel table and in the second spill.  Every thread has
  // C2 / (4 TPS) = 4 items; their kernel factors do not depend on the block: loaded once
  constexpr int NIT = TT * (C2 / 4) / NT;
  cf2 ha[NIT], hb[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int id = tid + NT * it;
    const int tt = id % TT, g = id / TT;
    const cf2* h = reinterpret_cast<const cf2*>(p.chirp + S2_INDEX(4 * g, pos0 + tt, R));
    ha[it] = h[0];
    hb[it] = h[1];
  }
  const cf* tw2 = p.ftw2_c;
  if constexpr (LOG2M >= 4) {   // radix-M twiddles from the LDS, behind the images (see frbch_k1_fast)
    cf* tl = lds + TT * SEQ;
    if (tid < M * 16) tl[tid] = p.ftw2_c[tid];
    tw2 = tl;
  }
  const int tid_outer = tid;
  for (int blk = blockIdx.y; blk < (int)p.nblk; blk += gridDim.y) {
    // the thread index is laundered per block: the compiler would otherwise hold every per-lane address of the body (tile pieces,
    // LDS slots of the three exchanges, row items) in registers across the loop, beside the kernel factors and the twiddles (it did:
    // 54 - 102 spilled registers)
    int tid_l = tid_outer;
    asm volatile("" : "+v"(tid_l));
    const int tid = tid_l;
    const int seq = tid / TPS, q = tid % TPS;
    {
      cf2 buf[NLD];
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int id = tid + NT * i;
        const int grp = id / pairs_per_grp, rem = id - grp * pairs_per_grp;
        const cf2* src = reinterpret_cast<const cf2*>(p.spill + ((uint64_t)blk * ngrp + grp) * p.gs + (uint64_t)pos0 * G1);
        if (whole_lines) {   // read once, nothing shared with the neighbouring tiles: non-temporal (K2c 3.10 -> 2.82 ms at M = 16)
          const nf4 t4 = __builtin_nontemporal_load(reinterpret_cast<const nf4*>(src + rem));
          buf[i] = cf2{cf{t4.x, t4.y}, cf{t4.z, t4.w}};
        } else {
          buf[i] = src[rem];
        }
      }
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int id = tid + NT * i;
        const int grp = id / pairs_per_grp, rem = id - grp * pairs_per_grp;
        const int tt = rem / (G1 / 2), pr = rem - tt * (G1 / 2);
        *reinterpret_cast<cf2*>(lds + tt * SEQ + pidx(grp * G1 + 2 * pr)) = buf[i];
      }
    }
    // (the first pass's twiddles per block, from the L2-resident table: held across the loop beside the kernel factors they spill)
    cf t1r[16];
    load_tw1<LOG2M>(t1r, p.ftw1_c, q);   // behind the gather in the queue, in front of the first barrier in time
    __syncthreads();
    cf* s = lds + seq * SEQ;
    cf v[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) v[a] = s[pidx(a * TPS + q)];
    fwd_passes_t<LOG2M>(v, s, q, Tw1Reg{t1r}, tw2);
    __syncthreads();   // the last pass has read the image: re-use it for the channel-ordered rows
    {
      const int k0 = (q / M) + 16 * (q % M);
#pragma unroll
      for (int kc = 0; kc < 16; ++kc) s[pidx(k0 + TPS * kc)] = v[kc];
    }
    __syncthreads();
    cf* dst = p.spill2 + (uint64_t)blk * C2 * R;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int id = tid + NT * it;
      const int tt = id % TT, g = id / TT;
      const cf2* src = reinterpret_cast<const cf2*>(lds + tt * SEQ + pidx(4 * g));
      const cf2 a = src[0], b = src[1];
      cf2* d = reinterpret_cast<cf2*>(dst + S2_INDEX(4 * g, pos0 + tt, R));
      store_spill(d, mul(a.a, ha[it].a), mul(a.b, ha[it].b));
      store_spill(d + 1, mul(b.a, hb[it].a), mul(b.b, hb[it].b));
    }
    __syncthreads();   // the rows are consumed: the next block's tile may overwrite the images
  }
}

// K3: one workgroup = NP = NT/(2*TPS) channels k (consecutive) with their mirror rows 2C-1-k.  grid (C/NP, nblk).
// LDS 2*NP*SEQ cf.  Sequence 2i holds row k_i, sequence 2i+1 its mirror.
template <int LOG2M, int NT>
__global__ void __launch_bounds__(NT, NT == 512 ? 2 : 1) frbch_k3_fast(KParams p) {   // (512 threads: two workgroups per CU)
  using GE = Geo<LOG2M>;
  constexpr int R = GE::L, TPS = GE::TPS;
  constexpr int SEQ = LOG2M >= 5 ? GE::L + GE::L / 8 : GE::SEQ;
  constexpr int NS = NT / TPS, NP = NS / 2;
  static_assert(NP >= 1, "a workgroup holds at least one channel and its mirror");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  const int tid = threadIdx.x;
  const int seq = tid / TPS, q = tid % TPS;
  const int blk = blockIdx.y;
  const int C2 = p.c2, C = p.c, T = p.tscr, NIF = p.nif;
  // XCD-aware: neighbouring channels (which share the 32-byte groups of the second spill) on one XCD
  const int nwg_ = gridDim.x;
  const int wg = (nwg_ % 8 == 0) ? (int)(blockIdx.x % 8) * (nwg_ / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int k = wg * NP + (seq >> 1);
  const int m = C2 - 1 - k;
  const int row = (seq & 1) ? m : k;
  const cf* base = p.spill2 + (uint64_t)blk * C2 * R;
  cf v[16];
#pragma unroll
  for (int kc = 0; kc < 16; ++kc) v[kc] = base[S2_INDEX(row, kc * TPS + q, R)];   // (plain loads: four channels share every 32 bytes)
  // requested with the gather instead of where it is used (behind the passes: a whole L2 round trip exposed per tile):
  // the DC correction of the mirror row
  cf dp = cf{0.f, 0.f};
  if (!(seq & 1)) dp = sub(base[S2_INDEX((m + 1) & (C2 - 1), 0, R)], base[S2_INDEX(m, 0, R)]);
  cf* s = lds + seq * SEQ;
  const cf* tw2 = p.ftw2_r;
  if constexpr (LOG2M >= 4) {   // radix-M twiddles from the LDS, behind the images (see frbch_k1_fast)
    cf* tl = lds + NS * SEQ;
    if (tid < GE::M * 16) tl[tid] = p.ftw2_r[tid];
    tw2 = tl;
  }
  bwd_passes<LOG2M>(v, s, q, p.ftw1_r, tw2);      // v[a] = x[a*TPS + q], natural time order
  __syncthreads();
  // the mirror sequence parks its series in its own image; its partner separates the polarisations
  if (seq & 1) {
#pragma unroll
    for (int a = 0; a < 16; ++a) s[pidx(a * TPS + q)] = v[a];
  }
  __syncthreads();
  float* pw = reinterpret_cast<float*>(lds + (seq & ~1) * SEQ);     // [prod][R] floats across the pair's two images (16 R <= 18 R bytes)
  cf wm[16];
  if (!(seq & 1)) {
    const cf* sm = lds + (seq + 1) * SEQ;
#pragma unroll
    for (int a = 0; a < 16; ++a) wm[a] = sm[pidx(a * TPS + q)];
  }
  __syncthreads();   // the parked series are in registers: the power rows may overwrite both images
  if (!(seq & 1)) {
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int t = a * TPS + q;
      const cf wk = v[a];
      const cf d = cf{wm[a].x + dp.x, -(wm[a].y + dp.y)};
      const cf y0 = cf{0.5f * (wk.x + d.x), 0.5f * (wk.y + d.y)};
      const cf y1 = cf{0.5f * (wk.y - d.y), -0.5f * (wk.x - d.x)};
      const float pp = y0.x * y0.x + y0.y * y0.y;
      const float qq = y1.x * y1.x + y1.y * y1.y;
      if (p.pol_mode == 0) pw[t] = pp;
      else if (p.pol_mode == 1) pw[t] = qq;
      else if (p.pol_mode == 2) pw[t] = pp + qq;
      else if (p.pol_mode == 3) pw[t] = (pp + qq) * (pp + qq);
      else {
        const cf pq = mulc(y0, y1);
        const bool iquv = p.pol_mode == 5;   // Stokes I, Q, U, V of circular feeds
        pw[t] = iquv ? pp + qq : pp;
        pw[R + t] = iquv ? 2.0f * pq.x : qq;
        pw[2 * R + t] = iquv ? 2.0f * pq.y : pq.x;
        pw[3 * R + t] = iquv ? pp - qq : pq.y;
      }
    }
  }
  __syncthreads();
  {   // overlap-save discard + tscrunch: both sequences of the pair write the channel's rows, coalesced
    const int rows = p.keep / T;
    const int lt = tid % (2 * TPS);
    for (int idx = lt; idx < NIF * rows; idx += 2 * TPS) {
      const int prod = idx / rows, r_ = idx - prod * rows;
      const float* src = pw + prod * R + p.nfilt_pos + r_ * T;
      float acc = 0.f;
      for (int e = 0; e < T; ++e) acc += src[e];
      p.ptmp[(((uint64_t)blk * NIF + prod) * C + k) * (uint64_t)rows + r_] = acc;
    }
  }
}

// K3, wave form (R = 4096): one workgroup = one channel k and its mirror row 2C-1-k, two waves (128 lanes x two virtual
// threads) per row, 74 KB of LDS: two workgroups per CU, 256 registers.  Persistent over the (block, channel) tiles of the
// launch (slot -> tile permuted so that the four channels of a 32-byte group of the second spill run on ONE XCD at the
// same time); the next tile's 32 points per lane are requested four at a time from eight points of the current tile's
// passes (see fwd_passes_w: a wave that issues its scattered loads in one go sits in the issue stage for the whole gather;
// the barrier kernel above overlaps nothing inside a workgroup).  Detection is shared: sequence 0 detects the positions of
// virtual thread 0, sequence 1 those of virtual thread 1 -- each parks the other half for its partner.
template <int LOG2M>
__global__ void __launch_bounds__(256, 2) frbch_k3_wave(KParams p) {
  using GE = GeoW<LOG2M, 2>;
  constexpr int R = GE::L, TPS = GE::TPS, LPS = GE::LPS, VT = GE::VT, SEQ = GE::SEQ;
  static_assert(VT == 2 && LPS == 128, "written for R = 4096");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  const int tid_outer = threadIdx.x;
  const int C2 = p.c2, C = p.c, T = p.tscr, NIF = p.nif;
  const uint32_t ntiles = p.nblk * (uint32_t)C;
  const bool perm = (ntiles % 32u == 0u) && (gridDim.x % 8u == 0u);
  auto tile_of = [&](uint32_t idx) { return perm ? ((idx & ~31u) | ((idx & 7u) << 2) | ((idx >> 3) & 3u)) : idx; };
  uint32_t slot = blockIdx.x;
  if (slot >= ntiles) return;
  const int lg_c = 31 - __builtin_clz(C);
  RegTw<LOG2M, VT> rtw;
  {
    const int lane0 = tid_outer & 63, wave0 = tid_outer >> 6;
    rtw.load(p.ftw1_r, p.ftw2_r, (wave0 & 1) * 64 + lane0, LPS, TPS);
  }
  // row pointer of a tile for this thread's sequence: position pos of the row lies at ptr[pos * 4] (S2_INDEX)
  auto row_ptr = [&](uint32_t tile, int sq) {
    const uint32_t b = tile >> lg_c, k = tile & (uint32_t)(C - 1);
    const uint32_t row = sq ? (uint32_t)(C2 - 1) - k : k;
    return p.spill2 + (uint64_t)b * C2 * R + S2_INDEX(row, 0, R);
  };
  cf buf[VT][16];
  auto fetch_part = [&](const cf* ptr, int qlane, int i0, int i1) {
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      if (i < i0 || i >= i1) continue;
      const int vt = i >> 4, kc = i & 15;
      buf[vt][kc] = ptr[(size_t)(kc * TPS + qlane + LPS * vt) * 4];   // (plain loads: four channels share every 32 bytes)
    }
  };
  uint32_t tile = tile_of(slot);
  {
    const int lane0 = tid_outer & 63, wave0 = tid_outer >> 6;
    fetch_part(row_ptr(tile, wave0 >> 1), (wave0 & 1) * 64 + lane0, 0, 32);
  }
  for (;;) {
    int tid_l = tid_outer;
    asm volatile("" : "+v"(tid_l));   // (per-lane LDS offsets are recomputed per trip instead of held across the loop)
    const int tid = tid_l, lane = tid & 63, wave = tid >> 6;
    const int seq = wave >> 1, ql = (wave & 1) * 64 + lane;
    __builtin_assume(ql >= 0 && ql < LPS);
    const uint32_t blk = tile >> lg_c;
    const int k = (int)(tile & (uint32_t)(C - 1));
    const int m = C2 - 1 - k;
    const cf* base = p.spill2 + (uint64_t)blk * C2 * R;
    cf v[VT][16];
#pragma unroll
    for (int vt = 0; vt < VT; ++vt)
#pragma unroll
      for (int a = 0; a < 16; ++a) v[vt][a] = buf[vt][a];
    // the DC correction of the mirror row: requested in front of the prefetch (its wait then leaves the prefetch in flight)
    const cf dpa = base[S2_INDEX((m + 1) & (C2 - 1), 0, R)], dpb = base[S2_INDEX(m, 0, R)];
    const uint32_t next_slot = slot + gridDim.x;
    const uint32_t next = tile_of(next_slot < ntiles ? next_slot : slot);
    const cf* const pf = row_ptr(next, seq);
    auto hook = [&](int n) { fetch_part(pf, ql, 4 * n, 4 * n + 4); };
    auto hk = [&](int n) {
      __builtin_amdgcn_sched_barrier(0);
      hook(n);
      __builtin_amdgcn_sched_barrier(0);
    };
    cf* s = lds + seq * SEQ;
    __builtin_amdgcn_s_setprio(1);   // the transforms and the detection win the issue arbitration against the partner workgroup's row output (K3 1.877 -> 1.85 ms)
    bwd_passes_w<LOG2M, 2, VT, true, true, NoMid, WgSync, decltype(hook)>(v, s, ql, p.ftw1_r, p.ftw2_r, &rtw, NoMid(), (WgSync*)nullptr, hook);   // hooks 0..4
    __syncthreads();   // every wave has read its last-pass inputs: the images take the parked halves
    // v[vt][a] = x[a*TPS + ql + LPS*vt].  Sequence 0 (row k) parks virtual thread 1, sequence 1 (mirror row) virtual thread 0
    if (seq == 0) {
#pragma unroll
      for (int a = 0; a < 16; ++a) s[pidx(a * TPS + ql + LPS)] = v[1][a];
    } else {
#pragma unroll
      for (int a = 0; a < 16; ++a) s[pidx(a * TPS + ql)] = v[0][a];
    }
    hk(5);
    __syncthreads();
    cf w[16];
    {
      const cf* so = lds + (seq ^ 1) * SEQ;
      const int qo = ql + LPS * seq;   // sequence 0 detects the positions of virtual thread 0, sequence 1 those of virtual thread 1
#pragma unroll
      for (int a = 0; a < 16; ++a) w[a] = so[pidx(a * TPS + qo)];
    }
    hk(6);
    __syncthreads();   // the parked halves are in registers: the power rows may overwrite both images
    {
      float* pw = reinterpret_cast<float*>(lds);     // [prod][R] floats across the two images
      const cf dp = sub(dpa, dpb);
      const int pm = p.pol_mode;
#pragma unroll
      for (int a = 0; a < 16; ++a) {
        const int t = a * TPS + ql + LPS * seq;
        const cf wk = seq ? w[a] : v[0][a];
        const cf wmv = seq ? v[1][a] : w[a];
        const cf d = cf{wmv.x + dp.x, -(wmv.y + dp.y)};
        const cf y0 = cf{0.5f * (wk.x + d.x), 0.5f * (wk.y + d.y)};
        const cf y1 = cf{0.5f * (wk.y - d.y), -0.5f * (wk.x - d.x)};
        const float pp = y0.x * y0.x + y0.y * y0.y;
        const float qq = y1.x * y1.x + y1.y * y1.y;
        if (pm == 0) pw[t] = pp;
        else if (pm == 1) pw[t] = qq;
        else if (pm == 2) pw[t] = pp + qq;
        else if (pm == 3) pw[t] = (pp + qq) * (pp + qq);
        else {
          const cf pq = mulc(y0, y1);
          const bool iquv = pm == 5;   // Stokes I, Q, U, V of circular feeds
          pw[t] = iquv ? pp + qq : pp;
          pw[R + t] = iquv ? 2.0f * pq.x : qq;
          pw[2 * R + t] = iquv ? 2.0f * pq.y : pq.x;
          pw[3 * R + t] = iquv ? pp - qq : pq.y;
        }
      }
    }
    hk(7);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    // rescale statistics of the interval being measured, summed here (A9 fused: no second pass over the power buffer):
    // per product the channel's sum and sum of squares over the rows below stat_limit, into this workgroup's own row of
    // the partial sums (exclusive: plain read-modify-write)
    const bool stat_on = p.stat_partial != nullptr && p.out_mode == FRBCH_OUT_FLOAT_POWER;
    float* red = reinterpret_cast<float*>(lds + 2 * SEQ);   // [NIF][4 waves][2], behind the images
    {   // overlap-save discard + tscrunch: the channel's rows, coalesced
      const float* pw = reinterpret_cast<const float*>(lds);
      const int rows = p.keep / T;
      const uint64_t row_abs0 = p.row0 + (uint64_t)blk * (uint64_t)rows;
      for (int prod = 0; prod < NIF; ++prod) {
        float s1 = 0.f, s2 = 0.f;
        int r_ = tid;
        if (T == 1) {   // no tscrunch: four rows per trip, their LDS reads requested together (one read, one wait, one store per row before)
          float* const dstp = p.ptmp + (((uint64_t)blk * NIF + prod) * C + k) * (uint64_t)rows;
          const float* const srcp = pw + prod * R + p.nfilt_pos;
          for (; r_ + 3 * 256 < rows; r_ += 4 * 256) {
            float x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = srcp[r_ + 256 * u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              dstp[r_ + 256 * u] = x[u];
              if (stat_on && row_abs0 + (uint64_t)(r_ + 256 * u) < p.stat_limit) {
                s1 += x[u];
                s2 = fmaf(x[u], x[u], s2);
              }
            }
          }
        }
        for (; r_ < rows; r_ += 256) {
          const float* src = pw + prod * R + p.nfilt_pos + r_ * T;
          float acc = 0.f;
          for (int e = 0; e < T; ++e) acc += src[e];
          p.ptmp[(((uint64_t)blk * NIF + prod) * C + k) * (uint64_t)rows + r_] = acc;
          if (stat_on && row_abs0 + (uint64_t)r_ < p.stat_limit) {
            s1 += acc;
            s2 = fmaf(acc, acc, s2);
          }
        }
        if (stat_on) {
#pragma unroll
          for (int off = 32; off >= 1; off >>= 1) {
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
          }
          if (lane == 0) {
            red[(prod * 4 + wave) * 2] = s1;
            red[(prod * 4 + wave) * 2 + 1] = s2;
          }
        }
      }
    }
    __syncthreads();   // the power rows are consumed (the next tile may overwrite the images); the wave sums are in place
    if (stat_on && tid < NIF) {
      double S = 0.0, SS = 0.0;
      for (int w_ = 0; w_ < 4; ++w_) {
        S += (double)red[(tid * 4 + w_) * 2];
        SS += (double)red[(tid * 4 + w_) * 2 + 1];
      }
      const int col = tid * C + (p.flip ? (C - 1 - k) : k);
      double* dst = p.stat_partial + ((size_t)blockIdx.x * (size_t)(NIF * C) + (size_t)col) * 2;
      dst[0] += S;
      dst[1] += SS;
    }
    if (next_slot >= ntiles) break;
    slot = next_slot;
    tile = next;
  }
}

// K4, vector form: channel-major power [blk][prod][chan][rows] -> time-major rows [row][prod][chan] (float power, or A9 +
// A10), 64 x 64 tiles through the LDS like the generic kernel, but 8-byte loads along the rows (rows even: every
// channel row starts 8-byte aligned) and 16-byte accesses along the channels: a quarter of the vector-memory
// instructions (the generic kernel moves 4 bytes per lane and instruction: 3.4 TB/s).  grid (ceil(rows/64) * ncol/64, nblk),
// 256 threads, LDS 64 x 65 floats.  Needs ncol % 64 == 0 and rows % 2 == 0.
__global__ void __launch_bounds__(256) frbch_k4_fast(KParams p) {
  __shared__ float tile[64 * 65];
  const int tid = threadIdx.x;
  const int C = p.c, NIF = p.nif, ncol = NIF * C, rows = p.keep / p.tscr;
  const int ctiles = ncol / 64;
  const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles, by = blockIdx.y;
  {
    nf2 r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u;             // 64 columns x 32 row pairs
      const int cl = idx >> 5, rp = idx & 31;
      const int col = ct * 64 + cl, row = rt * 64 + 2 * rp;
      const int prod = col / C, cout = col - prod * C;
      const int k = p.flip ? (C - 1 - cout) : cout;
      r[u] = nf2{0.f, 0.f};
      if (row < rows)
        r[u] = __builtin_nontemporal_load(reinterpret_cast<const nf2*>(p.ptmp + (((uint64_t)by * NIF + prod) * C + k) * (uint64_t)rows + row));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + 256 * u;
      const int cl = idx >> 5, rp = idx & 31;
      tile[cl * 65 + 2 * rp] = r[u].x;
      tile[cl * 65 + 2 * rp + 1] = r[u].y;
    }
  }
  __syncthreads();
  const int flip = p.flip;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int idx = tid + 256 * u;               // 64 rows x 16 groups of four columns
    const int rr = idx >> 4, cg = idx & 15;
    const int row = rt * 64 + rr;
    if (row >= rows) continue;
    const int col0 = ct * 64 + 4 * cg;
    const int prod = col0 / C, cout0 = col0 - prod * C;
    float sv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) sv[e] = tile[(4 * cg + e) * 65 + rr];
    const uint64_t o = (p.row0 + (uint64_t)by * rows + row) * (uint64_t)ncol + col0;
    const uint64_t oc = FRBCH_CODE_INDEX(p.out_pitch, p.row0 + (uint64_t)by * rows + row, p.nif, prod, cout0);
    if (p.out_mode == FRBCH_OUT_FLOAT_POWER) {
      const nf4 t4 = {sv[0], sv[1], sv[2], sv[3]};
      __builtin_nontemporal_store(t4, reinterpret_cast<nf4*>(p.power_out + o));
    } else {
      const int kbase = flip ? (C - 4 - cout0) : cout0;
      const float4 of4 = *reinterpret_cast<const float4*>(p.offset + prod * C + kbase);
      const float4 sc4 = *reinterpret_cast<const float4*>(p.scale + prod * C + kbase);
      const float ofv[4] = {of4.x, of4.y, of4.z, of4.w}, scv[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
      float x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = FMUL_RN(FADD_RN(sv[e], ofv[flip ? 3 - e : e]), scv[flip ? 3 - e : e]);
      if (p.nbit == -32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.code_out) + oc) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
        if (p.nbit == 8) {
          *reinterpret_cast<uint32_t*>(p.code_out + oc) = digitise4_u8(x, p.digi_mean, p.digi_scale);
        } else {
          uint32_t code[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) code[e] = digitise(x[e], p.digi_mean, p.digi_scale, p.digi_max);
          if (p.nbit == 16)
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.code_out) + oc) =
                make_uint2(code[0] | (code[1] << 16), code[2] | (code[3] << 16));
          else
            p.code_out[oc >> 2] = (uint8_t)(code[0] | (code[1] << 2) | (code[2] << 4) | (code[3] << 6));
        }
      }
    }
  }
}

// Kc fast: dP = diff(FFT_2C(S)) per block with the register passes; grid (1, nblk), TPS threads.
template <int LOG2M>
__global__ void __launch_bounds__(16 << LOG2M) frbch_kc_fast(KParams p) {
  using GE = Geo<LOG2M>;
  constexpr int M = GE::M, C2 = GE::L, TPS = GE::TPS, SEQ = GE::SEQ;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cf* lds = reinterpret_cast<cf*>(smem);
  cf* nat = lds + SEQ;
  const int q = threadIdx.x, blk = blockIdx.y;
  cf v[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) v[a] = p.s_dc[(uint64_t)blk * C2 + a * TPS + q];
  fwd_passes<LOG2M>(v, lds, q, p.ftw1_c, p.ftw2_c);
  const int k0 = (q / M) + 16 * (q % M);
#pragma unroll
  for (int kc = 0; kc < 16; ++kc) nat[k0 + TPS * kc] = v[kc];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = q + TPS * j;
    p.p0[(uint64_t)blk * C2 + k] = sub(nat[(k + 1) & (C2 - 1)], nat[k]);
  }
}


// =================================================================================================
// K2 for FEW channels: 2C = 64 or 128 (nchan 32 / 64 -- what the online chain cuts an IF into, submit_job.py:74-105
// `MinChanPerIF = 32`).  The across-branch transform is so short that ONE LANE keeps a whole 64-point sequence in
// registers: no LDS, no barrier, no cross-lane traffic inside the transform.  lane = one time sample t of one block
// (NH = 2, 2C = 128: a lane PAIR, one decimation-in-frequency stage splits the bins by parity: lane h holds bins 2m + h).
//   load   the 2C branches of sample t: G1 = 16 consecutive branches are 128 contiguous bytes per lane (slab layout
//          [blk][n1/16][t][n1%16] of the R = 512 wave K1), lanes 128 bytes apart: every 16-byte load is fully coalesced
//   FFT    64 points per lane, radix 8 x 8, twiddles compile-time constants
//   mirror W[2C-1-k] + dP[2C-1-k] sits in the same lane (NH = 1) or in the partner lane (NH = 2: one shuffle per value)
//   detect, tscrunch across neighbouring lanes (shuffles: T <= 64 / NH), float power or rescale + digitise; a lane writes
//          32 consecutive channels of its row
// grid: R * nblk * NH / 256 workgroups of 256 threads; LDS 4 x 9216 bytes (one transposing strip per wave).
// =================================================================================================
constexpr float kCos64[64] = {1.000000000e+00f, 9.951847267e-01f, 9.807852804e-01f, 9.569403357e-01f, 9.238795325e-01f, 8.819212643e-01f, 8.314696123e-01f, 7.730104534e-01f, 7.071067812e-01f, 6.343932842e-01f, 5.555702330e-01f, 4.713967368e-01f, 3.826834324e-01f, 2.902846773e-01f, 1.950903220e-01f, 9.801714033e-02f, 0.000000000e+00f, -9.801714033e-02f, -1.950903220e-01f, -2.902846773e-01f, -3.826834324e-01f, -4.713967368e-01f, -5.555702330e-01f, -6.343932842e-01f, -7.071067812e-01f, -7.730104534e-01f, -8.314696123e-01f, -8.819212643e-01f, -9.238795325e-01f, -9.569403357e-01f, -9.807852804e-01f, -9.951847267e-01f, -1.000000000e+00f, -9.951847267e-01f, -9.807852804e-01f, -9.569403357e-01f, -9.238795325e-01f, -8.819212643e-01f, -8.314696123e-01f, -7.730104534e-01f, -7.071067812e-01f, -6.343932842e-01f, -5.555702330e-01f, -4.713967368e-01f, -3.826834324e-01f, -2.902846773e-01f, -1.950903220e-01f, -9.801714033e-02f, 0.000000000e+00f, 9.801714033e-02f, 1.950903220e-01f, 2.902846773e-01f, 3.826834324e-01f, 4.713967368e-01f, 5.555702330e-01f, 6.343932842e-01f, 7.071067812e-01f, 7.730104534e-01f, 8.314696123e-01f, 8.819212643e-01f, 9.238795325e-01f, 9.569403357e-01f, 9.807852804e-01f, 9.951847267e-01f};
constexpr float kSin64[64] = {0.000000000e+00f, 9.801714033e-02f, 1.950903220e-01f, 2.902846773e-01f, 3.826834324e-01f, 4.713967368e-01f, 5.555702330e-01f, 6.343932842e-01f, 7.071067812e-01f, 7.730104534e-01f, 8.314696123e-01f, 8.819212643e-01f, 9.238795325e-01f, 9.569403357e-01f, 9.807852804e-01f, 9.951847267e-01f, 1.000000000e+00f, 9.951847267e-01f, 9.807852804e-01f, 9.569403357e-01f, 9.238795325e-01f, 8.819212643e-01f, 8.314696123e-01f, 7.730104534e-01f, 7.071067812e-01f, 6.343932842e-01f, 5.555702330e-01f, 4.713967368e-01f, 3.826834324e-01f, 2.902846773e-01f, 1.950903220e-01f, 9.801714033e-02f, 0.000000000e+00f, -9.801714033e-02f, -1.950903220e-01f, -2.902846773e-01f, -3.826834324e-01f, -4.713967368e-01f, -5.555702330e-01f, -6.343932842e-01f, -7.071067812e-01f, -7.730104534e-01f, -8.314696123e-01f, -8.819212643e-01f, -9.238795325e-01f, -9.569403357e-01f, -9.807852804e-01f, -9.951847267e-01f, -1.000000000e+00f, -9.951847267e-01f, -9.807852804e-01f, -9.569403357e-01f, -9.238795325e-01f, -8.819212643e-01f, -8.314696123e-01f, -7.730104534e-01f, -7.071067812e-01f, -6.343932842e-01f, -5.555702330e-01f, -4.713967368e-01f, -3.826834324e-01f, -2.902846773e-01f, -1.950903220e-01f, -9.801714033e-02f};
constexpr float kCos128[64] = {1.000000000e+00f, 9.987954562e-01f, 9.951847267e-01f, 9.891765100e-01f, 9.807852804e-01f, 9.700312532e-01f, 9.569403357e-01f, 9.415440652e-01f, 9.238795325e-01f, 9.039892931e-01f, 8.819212643e-01f, 8.577286100e-01f, 8.314696123e-01f, 8.032075315e-01f, 7.730104534e-01f, 7.409511254e-01f, 7.071067812e-01f, 6.715589548e-01f, 6.343932842e-01f, 5.956993045e-01f, 5.555702330e-01f, 5.141027442e-01f, 4.713967368e-01f, 4.275550934e-01f, 3.826834324e-01f, 3.368898534e-01f, 2.902846773e-01f, 2.429801799e-01f, 1.950903220e-01f, 1.467304745e-01f, 9.801714033e-02f, 4.906767433e-02f, 0.000000000e+00f, -4.906767433e-02f, -9.801714033e-02f, -1.467304745e-01f, -1.950903220e-01f, -2.429801799e-01f, -2.902846773e-01f, -3.368898534e-01f, -3.826834324e-01f, -4.275550934e-01f, -4.713967368e-01f, -5.141027442e-01f, -5.555702330e-01f, -5.956993045e-01f, -6.343932842e-01f, -6.715589548e-01f, -7.071067812e-01f, -7.409511254e-01f, -7.730104534e-01f, -8.032075315e-01f, -8.314696123e-01f, -8.577286100e-01f, -8.819212643e-01f, -9.039892931e-01f, -9.238795325e-01f, -9.415440652e-01f, -9.569403357e-01f, -9.700312532e-01f, -9.807852804e-01f, -9.891765100e-01f, -9.951847267e-01f, -9.987954562e-01f};
constexpr float kSin128[64] = {0.000000000e+00f, 4.906767433e-02f, 9.801714033e-02f, 1.467304745e-01f, 1.950903220e-01f, 2.429801799e-01f, 2.902846773e-01f, 3.368898534e-01f, 3.826834324e-01f, 4.275550934e-01f, 4.713967368e-01f, 5.141027442e-01f, 5.555702330e-01f, 5.956993045e-01f, 6.343932842e-01f, 6.715589548e-01f, 7.071067812e-01f, 7.409511254e-01f, 7.730104534e-01f, 8.032075315e-01f, 8.314696123e-01f, 8.577286100e-01f, 8.819212643e-01f, 9.039892931e-01f, 9.238795325e-01f, 9.415440652e-01f, 9.569403357e-01f, 9.700312532e-01f, 9.807852804e-01f, 9.891765100e-01f, 9.951847267e-01f, 9.987954562e-01f, 1.000000000e+00f, 9.987954562e-01f, 9.951847267e-01f, 9.891765100e-01f, 9.807852804e-01f, 9.700312532e-01f, 9.569403357e-01f, 9.415440652e-01f, 9.238795325e-01f, 9.039892931e-01f, 8.819212643e-01f, 8.577286100e-01f, 8.314696123e-01f, 8.032075315e-01f, 7.730104534e-01f, 7.409511254e-01f, 7.071067812e-01f, 6.715589548e-01f, 6.343932842e-01f, 5.956993045e-01f, 5.555702330e-01f, 5.141027442e-01f, 4.713967368e-01f, 4.275550934e-01f, 3.826834324e-01f, 3.368898534e-01f, 2.902846773e-01f, 2.429801799e-01f, 1.950903220e-01f, 1.467304745e-01f, 9.801714033e-02f, 4.906767433e-02f};

template <int DIR>
FI void fft64_lane(cf (&x)[64]) {
  // n = 8 n1 + n0, k = k1 + 8 k0: DFT-8 over n1, twiddle W64^(n0 k1), DFT-8 over n0; natural order in and out
#pragma unroll
  for (int n0 = 0; n0 < 8; ++n0) {
    cf a[8];
#pragma unroll
    for (int n1 = 0; n1 < 8; ++n1) a[n1] = x[8 * n1 + n0];
    Dft<8, DIR>::run(a);
#pragma unroll
    for (int k1 = 0; k1 < 8; ++k1) {
      const int m = (n0 * k1) & 63;
      const cf w = cf{kCos64[m], DIR < 0 ? -kSin64[m] : kSin64[m]};
      x[8 * k1 + n0] = (m == 0) ? a[k1] : mul(a[k1], w);           // A[n0][k1] kept at slot 8 k1 + n0
    }
  }
#pragma unroll
  for (int k1 = 0; k1 < 8; ++k1) {
    cf b[8];
#pragma unroll
    for (int n0 = 0; n0 < 8; ++n0) b[n0] = x[8 * k1 + n0];
    Dft<8, DIR>::run(b);
#pragma unroll
    for (int k0 = 0; k0 < 8; ++k0) x[8 * k1 + k0] = b[k0];          // X[k1 + 8 k0] at slot 8 k1 + k0
  }
}
// slot of spectrum bin m (= k1 + 8 k0) after fft64_lane
#define FFT64_SLOT(m) (8 * ((m) & 7) + ((m) >> 3))

template <int NH, int PM>
__global__ void __launch_bounds__(256) frbch_k2_lane(KParams p) {   // (capped at 168 registers for three waves per SIMD: 3 spills, same time)
  constexpr int C2 = 64 * NH, C = C2 / 2, G1 = 16, NGRP = C2 / G1;
  constexpr int NPROD = PM == 4 ? 4 : 1;
  const uint32_t gtid = blockIdx.x * 256u + threadIdx.x;
  const int h = NH == 2 ? (int)(gtid & 1u) : 0;
  const uint32_t ts = NH == 2 ? gtid >> 1 : gtid;                     // (block, time sample)
  const int blk = (int)(ts >> p.log2_r);
  const int t = (int)(ts & (uint32_t)(p.r - 1));
  // (the grid covers whole blocks: R * NH is a multiple of 256, checked by the plan -- every lane is live, shuffles are safe)
  // Gather through the LDS: read straight, a lane's 128 bytes of a group would be 16 bytes of each of eight load
  // instructions whose 64 lanes touch 64 different lines (the address unit takes them one line at a time: measured 2 TB/s).
  // Instead the wave reads the 8 KB its 64 time samples occupy in one group as eight fully coalesced 1-KB loads (lane =
  // 16-byte piece), parks them in its own 9-KB strip of the LDS (rows of 128 + 16 bytes: the per-lane 16-byte reads that
  // follow hit distinct banks) and every lane picks up its own row.  Wave-private: no workgroup barrier.
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int ROWB = G1 * 8 + 16;                                   // bytes per (time sample) row of the strip
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* strip = smem + (size_t)wave * (64 * ROWB);
  // the wave's 64 lanes = 64 / NH consecutive time samples (x NH lanes each); t0 = first of them
  const int t0 = t - (NH == 2 ? (lane >> 1) : lane);
  const cf* base = p.spill + (uint64_t)blk * (uint64_t)NGRP * p.gs + (uint64_t)t0 * G1;
  constexpr int TSW = 64 / NH;                                        // time samples per wave
  constexpr int NLD = TSW * G1 * 8 / (64 * 16);                       // 16-byte loads per lane and group (8, or 4 for a lane pair)
  cf x[64];
  auto fetch_group = [&](int g, cf2 (&v)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i)
      v[i] = *reinterpret_cast<const cf2*>(reinterpret_cast<const char*>(base + (uint64_t)g * p.gs) + (size_t)(i * 64 + lane) * 16);
  };
  auto park_group = [&](const cf2 (&v)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int piece = i * 64 + lane;                                // 16-byte piece of the 8-KB (4-KB) run: row = piece / 8
      *reinterpret_cast<cf2*>(strip + (size_t)(piece >> 3) * ROWB + (size_t)(piece & 7) * 16) = v[i];
    }
  };
  const int myrow = NH == 2 ? (lane >> 1) : lane;
  auto pick_group = [&](cf (&out)[G1]) {
#pragma unroll
    for (int s = 0; s < G1; s += 2) {
      const cf2 v = *reinterpret_cast<const cf2*>(strip + (size_t)myrow * ROWB + (size_t)s * 8);
      out[s] = v.a;
      out[s + 1] = v.b;
    }
  };
  if constexpr (NH == 1) {
    cf2 nxt[NLD];
    fetch_group(0, nxt);
#pragma unroll
    for (int g = 0; g < NGRP; ++g) {
      park_group(nxt);
      if (g + 1 < NGRP) fetch_group(g + 1, nxt);
      __builtin_amdgcn_wave_barrier();
      cf tmp[G1];
      pick_group(tmp);
#pragma unroll
      for (int s = 0; s < G1; ++s) x[g * G1 + s] = tmp[s];
      __builtin_amdgcn_wave_barrier();
    }
  } else {
    // one decimation-in-frequency stage: lane h keeps y[n] = (a[n] + (-1)^h a[n + 64]) W128^(n h); FFT64(y) = bins 2m + h
#pragma unroll
    for (int g = 0; g < NGRP / 2; ++g) {
      cf2 va[NLD], vb[NLD];
      fetch_group(g, va);
      fetch_group(g + NGRP / 2, vb);
      cf a[G1], b[G1];
      park_group(va);
      __builtin_amdgcn_wave_barrier();
      pick_group(a);
      __builtin_amdgcn_wave_barrier();
      park_group(vb);
      __builtin_amdgcn_wave_barrier();
      pick_group(b);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < G1; ++s) {
        const int n = g * G1 + s;
        const cf sum = add(a[s], b[s]), dif = mul(sub(a[s], b[s]), cf{kCos128[n], -kSin128[n]});
        x[n] = h ? dif : sum;
      }
    }
  }
  fft64_lane<-1>(x);
  // ---- mirror partner wm = W[2C-1-k] + dP[2C-1-k] and detection, bin by bin (no array of partners: the four-product
  //      instantiation has no registers for one).  This lane's 32 lower-half channels, index m: k = m (NH = 1) or 2m + h
  const cf* dP = p.p0 + (size_t)__builtin_amdgcn_readfirstlane(blk) * C2;   // (a wave lies inside one block: scalar loads)
  float pw[NPROD][32];
  const int pm = p.pol_mode;
#pragma unroll
  for (int m = 0; m < 32; ++m) {
    const int mm = 63 - m;
    cf wm;
    if constexpr (NH == 1) {
      wm = add(x[FFT64_SLOT(mm)], dP[mm]);                             // k = m, mirror 63 - m: the same lane
    } else {
      // k = 2m + h; its mirror 127 - k = 2 (63 - m) + (1 - h) lives in the partner lane, register 63 - m
      const cf mine = add(x[FFT64_SLOT(mm)], dP[2 * mm + h]);          // what the PARTNER needs for its bin 2m + (1 - h)
      wm = cf{__shfl_xor(mine.x, 1), __shfl_xor(mine.y, 1)};
    }
    const cf wk = x[FFT64_SLOT(m)];
    const cf d = cf{wm.x, -wm.y};
    if constexpr (PM == 2) {
      pw[0][m] = 0.5f * ((wk.x * wk.x + wk.y * wk.y) + (d.x * d.x + d.y * d.y));
    } else {
      const cf y0 = cf{0.5f * (wk.x + d.x), 0.5f * (wk.y + d.y)};
      const cf y1 = cf{0.5f * (wk.y - d.y), -0.5f * (wk.x - d.x)};
      const float pp = y0.x * y0.x + y0.y * y0.y;
      const float qq = y1.x * y1.x + y1.y * y1.y;
      if constexpr (PM == 4) {
        const cf pq = mulc(y0, y1);
        const bool iquv = pm == 5;
        pw[0][m] = iquv ? pp + qq : pp;
        pw[1][m] = iquv ? 2.0f * pq.x : qq;
        pw[2][m] = iquv ? 2.0f * pq.y : pq.x;
        pw[3][m] = iquv ? pp - qq : pq.y;
      } else {
        const float i1 = pp + qq;
        pw[0][m] = pm == 0 ? pp : (pm == 1 ? qq : i1 * i1);
      }
    }
  }
  // ---- A8: tscrunch over T neighbouring time samples = lanes NH apart (a wave holds 64 / NH consecutive samples) ------
  const int T = p.tscr;
  for (int s = 1; s < T; s <<= 1) {
#pragma unroll
    for (int pr = 0; pr < NPROD; ++pr)
#pragma unroll
      for (int m = 0; m < 32; ++m) pw[pr][m] += __shfl_xor(pw[pr][m], s * NH);
  }
  // NH = 2: the pair re-sorts its interleaved bins so that lane h owns the 32 CONSECUTIVE channels 32 h .. 32 h + 31
  float row[NPROD][32];
#pragma unroll
  for (int pr = 0; pr < NPROD; ++pr) {
    if constexpr (NH == 1) {
#pragma unroll
      for (int m = 0; m < 32; ++m) row[pr][m] = pw[pr][m];
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const float send = h ? pw[pr][j] : pw[pr][16 + j];
        const float recv = __shfl_xor(send, 1);
        // lane 0: k = 2j (own, register j), 2j + 1 (partner's register j); lane 1: k = 32 + 2j (partner's 16 + j), 33 + 2j (own)
        row[pr][2 * j] = h ? recv : pw[pr][j];
        row[pr][2 * j + 1] = h ? pw[pr][16 + j] : recv;
      }
    }
  }
  // ---- emit through the wave's LDS strip: a lane's run of 32 channels is 128 bytes of floats (32 / 64 / 8 bytes of codes),
  //      lanes 128+ bytes apart -- stored straight, every store instruction would touch 64 different lines with 16 bytes
  //      each (SQ counters: the waves spent 69 % of their life waiting to issue).  The valid lanes park their runs as rows
  //      of the strip, then all 64 lanes copy the rows out in 16-byte pieces: consecutive lanes, consecutive addresses.
  const int lg_t = 31 - __builtin_clz(T);
  const bool valid = (t & (T - 1)) == 0;
  const int rloc = myrow >> lg_t;                                      // this lane's row among the wave's output rows
  const int nrows = TSW >> lg_t;
  const uint64_t orow0 = p.row0 + (uint64_t)blk * (uint64_t)(p.r >> lg_t) + (uint64_t)(t0 >> lg_t);
  const int k0 = 32 * h;                                               // first input channel of this lane's run
  const int flip = p.flip;
  const int cout0 = flip ? (C - 32 - k0) : k0;                         // first output column of the run
  constexpr int ROWB2 = NH * 128 + 16;
  const bool fl = p.out_mode == FRBCH_OUT_FLOAT_POWER;
  const int nbit = fl ? 32 : (p.nbit == -32 ? 32 : p.nbit);            // bits per stored value
  const int lane_bytes = 32 * nbit / 8, row_bytes = NH * lane_bytes;
  const int pb = row_bytes >= 16 ? 16 : row_bytes;                     // bytes per copied piece (8: 2-bit codes of 32 channels)
  const int ppr = row_bytes / pb;                                      // pieces per row
#pragma unroll
  for (int pr = 0; pr < NPROD; ++pr) {
    float sv[32];                                                      // in output column order
#pragma unroll
    for (int e = 0; e < 32; ++e) sv[e] = flip ? row[pr][31 - e] : row[pr][e];
    __builtin_amdgcn_wave_barrier();                                   // (the strip's previous rows are copied out)
    unsigned char* lrow = strip + (size_t)rloc * ROWB2 + (size_t)(cout0 >> 5) * lane_bytes;
    if (fl) {
      if (valid) {
#pragma unroll
        for (int e = 0; e < 32; e += 4) *reinterpret_cast<float4*>(lrow + e * 4) = make_float4(sv[e], sv[e + 1], sv[e + 2], sv[e + 3]);
      }
    } else {
      float xs[32];
#pragma unroll
      for (int e = 0; e < 32; ++e) {
        const int k = flip ? (C - 1 - (cout0 + e)) : (cout0 + e);
        xs[e] = FMUL_RN(FADD_RN(sv[e], p.offset[pr * C + k]), p.scale[pr * C + k]);
      }
      if (nbit == 32) {
        if (valid) {
#pragma unroll
          for (int e = 0; e < 32; e += 4) *reinterpret_cast<float4*>(lrow + e * 4) = make_float4(xs[e], xs[e + 1], xs[e + 2], xs[e + 3]);
        }
      } else {
        uint32_t code[32];
        if (nbit != 8) {
#pragma unroll
          for (int e = 0; e < 32; ++e) code[e] = digitise(xs[e], p.digi_mean, p.digi_scale, p.digi_max);
        }
        if (nbit == 8) {
          uint32_t w[8];
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            const float x8[8] = {xs[4 * j], xs[4 * j + 1], xs[4 * j + 2], xs[4 * j + 3], xs[4 * j + 4], xs[4 * j + 5], xs[4 * j + 6], xs[4 * j + 7]};
            digitise8_u8(x8, p.digi_mean, p.digi_scale, w[j], w[j + 1]);
          }
          if (valid) {
            *reinterpret_cast<uint4*>(lrow) = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint4*>(lrow + 16) = make_uint4(w[4], w[5], w[6], w[7]);
          }
        } else if (nbit == 16) {
          uint32_t w[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) w[j] = code[2 * j] | (code[2 * j + 1] << 16);
          if (valid) {
#pragma unroll
            for (int j = 0; j < 16; j += 4) *reinterpret_cast<uint4*>(lrow + j * 4) = make_uint4(w[j], w[j + 1], w[j + 2], w[j + 3]);
          }
        } else {
          uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
          for (int e = 0; e < 16; ++e) { w0 |= code[e] << (2 * e); w1 |= code[16 + e] << (2 * e); }
          if (valid) *reinterpret_cast<uint2*>(lrow) = make_uint2(w0, w1);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    // byte address of (row orow0 + r, product pr), first column
    const int total = nrows * ppr;
    for (int i = lane; i < total; i += 64) {
      const int r = i / ppr, part = i - r * ppr;
      unsigned char* out;
      if (fl) out = reinterpret_cast<unsigned char*>(p.power_out + ((orow0 + r) * NPROD + pr) * (uint64_t)C);
      else out = p.code_out + FRBCH_CODE_INDEX(p.out_pitch, orow0 + r, NPROD, pr, 0) * (uint64_t)nbit / 8;
      const unsigned char* src = strip + (size_t)r * ROWB2 + (size_t)part * pb;
      if (pb == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(src);
        if (fl) { const nf4 t4 = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
                  __builtin_nontemporal_store(t4, reinterpret_cast<nf4*>(out + (size_t)part * 16)); }
        else *reinterpret_cast<uint4*>(out + (size_t)part * 16) = v;
      } else {
        *reinterpret_cast<uint2*>(out + (size_t)part * pb) = *reinterpret_cast<const uint2*>(src);
      }
    }
  }
}

// Kc for 2C = 64 (frbch_k2_lane's companion): P0 = FFT_64(S), dP[k'] = P0[(k'+1) mod 64] - P0[k'] -- one LANE per filterbank
// block, the same in-register transform (the generic Kc spends a 256-thread workgroup and an LDS radix-2 FFT on 64 points).
// grid (ceil(nblk / 64), 1), 64 threads.
__global__ void __launch_bounds__(64) frbch_kc_lane(KParams p) {
  const uint32_t blk = blockIdx.x * 64u + threadIdx.x;
  if (blk >= p.nblk) return;
  const cf2* src = reinterpret_cast<const cf2*>(p.s_dc + (size_t)blk * 64);
  cf x[64];
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const cf2 v = src[i];
    x[2 * i] = v.a;
    x[2 * i + 1] = v.b;
  }
  fft64_lane<-1>(x);
  cf2* dst = reinterpret_cast<cf2*>(p.p0 + (size_t)blk * 64);
#pragma unroll
  for (int k = 0; k < 64; k += 2) {
    const cf a = sub(x[FFT64_SLOT((k + 1) & 63)], x[FFT64_SLOT(k)]);
    const cf b = sub(x[FFT64_SLOT((k + 2) & 63)], x[FFT64_SLOT(k + 1)]);
    dst[k >> 1] = cf2{a, b};
  }
}

#undef FI
}  // namespace fast
