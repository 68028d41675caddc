// fp32-accurate GEMMs on the bf16 matrix pipes ("bf16x6").  Included by gemm.hip inside its
// anonymous namespace (uses GemmArgs, Seg3, FastEpi / wave_epilogue).
//
// Every fp32 operand element x is decomposed EXACTLY into three bf16 values
//     x = h + m + l,   h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)      (round to nearest)
// (8 + 8 + 8 significand bits; both subtractions are exact in fp32 and the last residual has at
// most 8 significant bits, so nothing is lost).  A product a*b is then accumulated as the six
// leading partial products  ah*bh + ah*bm + am*bh + am*bm + ah*bl + al*bh  by
// v_mfma_f32_16x16x32_bf16 (products exact, fp32 accumulation).  Worst-case bound of what is dropped: with
// u = 2^-8 (bf16 unit round-off under round-to-nearest) |m| <= u|x| and |l| <= u^2|x|, so the three dropped
// terms am*bl + al*bm + al*bl are at most (2u^3 + u^4)|a*b| < 2^-23 |a*b| per product (two terms of 2^-24,
// one of 2^-32) -- the size of ONE fp32 rounding of that product -- and typically 2^-26 |a*b| (the residuals
// are uniformly distributed, not maximal).  Summed over k the dropped part is <= 2^-23 sum|a_k b_k|, against
// the K * 2^-24 sum|a_k b_k| worst case of any fp32 accumulation chain, which both kernels share.
// tests/test_kernels_gpu.py::test_linear_bf16x6_adversarial_vs_fp64 asserts |err| <= (2^-23 + 1.5 r32) sum|a_k b_k|
// per output (r32 = the fp32-MFMA kernel's worst relative error on the same data, i.e. the accumulation term) on
// cancelling sums, 2^+-60 per-k scales, all-ones significands and 2^-112-scaled gradients.
// Measured against fp64
// (tools/gemm_x6_proto.hip): mean error 1.4e-8 * sum|a_k b_k| versus 1.7e-8 for the fp32 fma
// chain of the v_mfma_f32_32x32x2_f32 kernel -- fp32-class results at 6 x 32 cycles per
// 32x32x16 block instead of 8 x 64.  The 16x16x32 shape is used because the chip sustains a higher
// clock on it: the same loop ran 20-29 % faster than with 32x32x16 (tools/gemm_x6_proto.hip).
//
// bf16x3 (opt-in, GCT_GEMM_BF16X3; the same kernels instantiated with NP = 2 pieces): x is split as x ~ h + m, the
// first two pieces of the same exact split, and a*b is accumulated as the three leading products am*bh + ah*bm + ah*bh.
// Bound of what is dropped, from the same piece bounds (|x - h| <= u|x|, so |m| <= u|x|, |l| <= u^2|x|, and
// |h| <= (1 + u)|x|): am*bm + ah*bl + al*bh + am*bl + al*bm + al*bl  <=  (u^2 + 2(1 + u)u^2 + 2u^3 + u^4)|a*b|
// = (3u^2 + 4u^3 + u^4)|a*b| < 3.02 * 2^-16 |a*b| per product -- about 16 good bits instead of 24 (TF32 rounds each
// product by about 2^-10).  Summed over k: <= 3.02 * 2^-16 sum|a_k b_k| on top of the shared fp32 accumulation term.
// tests/test_gemm_x3_gpu.py asserts |err| <= (3.02 * 2^-16 + 1.5 r32) sum|a_k b_k| (+ the flush floor) on the same
// adversarial data as the bf16x6 test.  The weight planes are those of bf16x6 (planes 0 and 1 are read), so a mode
// switch needs no re-split.
//
// Range notes: an infinite operand (or one that rounds to +-inf in bf16, |x| > 3.39e38) turns its residual
// into NaN, so inf inputs give NaN where fp32 arithmetic could give inf; pieces below the bf16 normal range
// (|x| < 2^-110 or so) are flushed, an absolute error under 1e-38.  Neither occurs in this model.
//
// Shape of the machine mapping:
//   * block tile 128 x 256 x 32, 8 waves (2 x 4), each wave 64 x 64 = 4 x 4 MFMA tiles of 16 x 16;
//   * LDS: two stages of {A planes 3 x 8 KB, B planes 3 x 16 KB} = 144 KB (one workgroup per
//     CU, two waves per SIMD), one barrier per K-tile;
//   * activations are split on the fly while they are staged (VALU work interleaved with the
//     MFMA stream); weights arrive pre-split (gct_split_planes, once per step), so only one
//     operand of the forward / dgrad GEMMs costs VALU time;
//   * K-contiguous operands are read from a 64-B-row image with ds_read_b128; operands whose
//     reduction index is the slow one (W for dgrad, dY and X for wgrad) keep their natural
//     [k][free] layout in LDS and are read with the transposing ds_read_b64_tr_b16;
//   * software pipeline per K-tile; four fragment sets of two tiles each (A01, A23, B01, B23 = 96 VGPRs),
//     quarter phases ordered so that every set is reloaded while another phase's MFMAs run:
//       first half : MFMAs (A01,B01) (A23,B01) | reads of A23, B23; split + LDS stores of tile t+1
//       barrier
//       second half: MFMAs (A01,B23) (A23,B23) | reads of B01, A01 of tile t+1; global loads of tile t+2

typedef __bf16 x6_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 x6_bf16x2 __attribute__((ext_vector_type(2)));
typedef float x6_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned x6_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned x6_u32x2 __attribute__((ext_vector_type(2)));
typedef short x6_s16x4 __attribute__((ext_vector_type(4)));
typedef short x6_s16x8 __attribute__((ext_vector_type(8)));

enum { X6_FWD = 0, X6_DGRAD = 1, X6_WGRAD = 2 };
constexpr int XBM = 128, XBN = 256, XBK = 32;
constexpr int X_APL = 8192, X_BPL = 16384, X_STAGE = 3 * X_APL + 3 * X_BPL;  // 72 KB per stage
constexpr int X_KLIST_MAX = 1024;                       // wgrad tile-list entries cached per workgroup
constexpr int X_LDS_BYTES = 2 * X_STAGE + X_KLIST_MAX * 4;

__device__ __forceinline__ unsigned x6_pk(float a, float b) {
  x6_f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, x6_bf16x2));
}
__device__ __forceinline__ float x6_sub(float a, float b) {
  float r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// two fp32 -> three packed bf16 pairs; element 0 in the low half
__device__ __forceinline__ void x6_split2(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
  // plain v_sub_f32 on purpose: hipcc SLP-packs these pairs into v_pk_add_f32, which is slower than two
  // scalar subtractions next to MFMAs
  h = x6_pk(a, b);
  const float ra = x6_sub(a, __uint_as_float(h << 16)), rb = x6_sub(b, __uint_as_float(h & 0xffff0000u));
  m = x6_pk(ra, rb);
  const float sa = x6_sub(ra, __uint_as_float(m << 16)), sb = x6_sub(rb, __uint_as_float(m & 0xffff0000u));
  l = x6_pk(sa, sb);
}
__device__ __forceinline__ void x6_split4(const float4 v, x6_u32x2& h, x6_u32x2& m, x6_u32x2& l) {
  unsigned h0, m0, l0, h1, m1, l1;
  x6_split2(v.x, v.y, h0, m0, l0);
  x6_split2(v.z, v.w, h1, m1, l1);
  h = x6_u32x2{h0, h1}; m = x6_u32x2{m0, m1}; l = x6_u32x2{l0, l1};
}
// the first NP pieces (NP = 3: h, m, l; NP = 2: h, m -- the last residual is not formed) of four fp32 values
template <int NP>
__device__ __forceinline__ void x6_split4n(const float4 v, x6_u32x2 (&pc)[NP]) {
  if constexpr (NP == 3) {
    x6_split4(v, pc[0], pc[1], pc[2]);
  } else {
    static_assert(NP == 2, "bf16x6 (3 pieces) or bf16x3 (2 pieces)");
    unsigned h0, h1;
    h0 = x6_pk(v.x, v.y);
    h1 = x6_pk(v.z, v.w);
    const float r0 = x6_sub(v.x, __uint_as_float(h0 << 16)), r1 = x6_sub(v.y, __uint_as_float(h0 & 0xffff0000u));
    const float r2 = x6_sub(v.z, __uint_as_float(h1 << 16)), r3 = x6_sub(v.w, __uint_as_float(h1 & 0xffff0000u));
    pc[0] = x6_u32x2{h0, h1};
    pc[1] = x6_u32x2{x6_pk(r0, r1), x6_pk(r2, r3)};
  }
}

// row image: [rows][32 k] bf16 = 64-B rows; 16-B chunk c (8 k-values) of row r.  A 16x16x32 fragment read
// takes row (lane & 15), chunk (lane >> 4); the per-4-rows permutation {0,2,3,1} keeps every 16-lane group
// of the ds_read_b128 on 16 distinct 16-B slots.  Adding 16 rows leaves the permutation unchanged, so the
// four row tiles of a wave share one address register (+1024 B each).
__device__ __forceinline__ int x6_row_off(int r, int c) {
  const int g = (0x78 >> (2 * ((r >> 2) & 3))) & 3;
  return r * 64 + ((c ^ g) << 4);
}
// transposed image: [32 k][W free] bf16, `stride` bytes per k-row, byte column cb.  One half-wave of a
// transposed read touches rows k..k+3 and k+8..k+11 at the same 32-B column block: the XOR spreads the four
// rows over the 256-B bank row (64 B apart) and moves the second group to the neighbouring 32 B.
__device__ __forceinline__ int x6_tr_off(int k, int cb, int stride) {
  return k * stride + (cb ^ (((k & 3) << 6) | (((k >> 3) & 1) << 5)));
}

__device__ __forceinline__ x6_bf16x8 x6_tr_frag(const unsigned char* p, int stride) {
  typedef __attribute__((address_space(3))) x6_s16x4 lds_s16x4;
  const x6_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  const x6_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p + 4 * stride));
  const x6_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(x6_bf16x8, v);
}

typedef float x6_f32x4 __attribute__((ext_vector_type(4)));
#define X6_MFMA(a_, b_, c_) c_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a_, b_, c_, 0, 0, 0)

// MODE  A operand (split on the fly)              B operand
// FWD   x  [M][K]   K-contiguous, row reads       W planes [N][K]   K-contiguous, row reads
// DGRAD dY [M][K']  K'-contiguous (segmented)     W planes [K'][N]  natural, transposed reads
// WGRAD dY [K'][M]  natural, transposed reads     X fp32 [K'][N]    natural, split on the fly, transposed reads
// NP = pieces per operand element: 3 (bf16x6, six products) or 2 (bf16x3, three products; the LDS layout and the
// stage size stay those of NP = 3, the third plane slots are left unused)
// The body of one workgroup: block `bid` of a (sub-)grid of `nblk` blocks that covers the problem g.  The XCD remap is
// applied within that sub-grid, so the blocks that share an operand panel stay on one XCD whether the problem has the
// launch to itself (gemm_x6_kernel) or shares it (gemm_x6_bwd_pair_kernel).
template <int MODE, int NP>
__device__ __forceinline__ void gemm_x6_body(const GemmArgs& g, const unsigned bid, const unsigned nblk) {
  static_assert(NP == 2 || NP == 3, "bf16x3 or bf16x6");
  extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
  constexpr bool A_TR = MODE == X6_WGRAD, B_TR = MODE != X6_FWD, B_PL = MODE != X6_WGRAD;
  constexpr int NB = B_PL ? 2 : 4;  // B loads per thread (x NP planes when pre-split)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 2) * 64, wn = (wave & 3) * 64;

  const unsigned tiles_n = (unsigned)((g.N + XBN - 1) / XBN);
  const unsigned tiles_m = (unsigned)((g.M + XBM - 1) / XBM);
  const unsigned per_split = tiles_m * tiles_n;
  const unsigned lid = gct_xcd_remap(bid, nblk);
  const unsigned z = lid / per_split, rest = lid - z * per_split;
  const int64_t m0 = (int64_t)(rest / tiles_n) * XBM, n0 = (int64_t)(rest % tiles_n) * XBN;
  const int64_t kbeg = (int64_t)z * g.ksplit;
  const int64_t kend = (kbeg + g.ksplit < g.K) ? kbeg + g.ksplit : g.K;

  // ---- per-thread invariant 32-bit element offsets (edges clamped into valid memory: they only
  //      feed accumulator rows / columns that are never stored) and LDS store offsets
  uint32_t offa[2], offb[NB];
  int sta[2], stb[NB];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (!A_TR) {
      int64_t r = (tid >> 3) + 64 * j;
      sta[j] = x6_row_off((int)r, (tid & 7) >> 1) + (tid & 1) * 8;
      if (m0 + r > g.M - 1) r = g.M - 1 - m0;
      offa[j] = (uint32_t)(r * g.lda + (tid & 7) * 4);
    } else {
      const int kr = (tid >> 5) + 16 * j;
      int64_t c = (tid & 31) * 4;
      sta[j] = x6_tr_off(kr, (tid & 31) * 8, 256);
      if (m0 + c > g.M - 4) c = g.M - 4 - m0;
      offa[j] = (uint32_t)(kr * g.lda + c);
    }
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (MODE == X6_FWD) {
      int64_t r = (tid >> 2) + 128 * j;
      stb[j] = x6_row_off((int)r, tid & 3);
      if (n0 + r > g.N - 1) r = g.N - 1 - n0;
      offb[j] = (uint32_t)(r * g.ldb + (tid & 3) * 8);
    } else if (MODE == X6_DGRAD) {
      const int kr = (tid >> 5) + 16 * j;
      int64_t c = (tid & 31) * 8;
      stb[j] = x6_tr_off(kr, (tid & 31) * 16, 512);
      if (n0 + c > g.N - 8) c = g.N - 8 - n0;
      offb[j] = (uint32_t)(kr * g.ldb + c);
    } else {
      const int kr = (tid >> 6) + 8 * j;
      int64_t c = (tid & 63) * 4;
      stb[j] = x6_tr_off(kr, (tid & 63) * 8, 512);
      if (n0 + c > g.N - 4) c = g.N - 4 - n0;
      offb[j] = (uint32_t)(kr * g.ldb + c);
    }
  }
  // ---- wave-uniform tile bases; a K-tile (resp. the row / column tile) lies in ONE segment
  auto seg_off = [](const Seg3& s, int64_t idx, int64_t nper, int64_t& local) -> int64_t {
    const bool g1 = idx >= nper, g2 = idx >= 2 * nper;
    local = idx - (g2 ? 2 * nper : (g1 ? nper : 0));
    return g2 ? s.d2 : (g1 ? s.d1 : 0);
  };
  int64_t a_fix = 0, b_fix = 0;   // k-independent part of the base offsets
  {
    int64_t loc;
    if (A_TR) { a_fix = seg_off(g.a, m0, g.a_nper, loc); a_fix += loc; }
    else a_fix = m0 * g.lda;
    if (MODE == X6_FWD) { b_fix = seg_off(g.b, n0, g.b_nper, loc); b_fix += loc * g.ldb; }
    else b_fix = n0;
  }
  auto abase = [&](int64_t k0) -> const float* {
    if (A_TR) return g.a.p0 + a_fix + k0 * g.lda;
    int64_t loc;
    const int64_t so = seg_off(g.a, k0, g.a_nper, loc);
    return g.a.p0 + so + a_fix + loc;
  };
  auto boff = [&](int64_t k0) -> int64_t {
    if (MODE == X6_FWD) return b_fix + k0;
    int64_t loc;
    const int64_t so = seg_off(g.b, k0, g.b_nper, loc);
    return so + loc * g.ldb + b_fix;
  };

  x6_f32x4 acc[4][4];   // 4 x 4 tiles of 16 x 16: C[row = 4 * (lane >> 4) + r][col = lane & 15]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = x6_f32x4{0.f, 0.f, 0.f, 0.f};

  float4 pa[2];
  x6_u32x4 pbp[NP][2];  // B_PL
  float4 pbf[4];        // !B_PL
#define X6_GLOAD(k0_)                                                                          \
  do {                                                                                         \
    const float* ab__ = abase(k0_);                                                            \
    const int64_t bo__ = boff(k0_);                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
        pa[j] = *reinterpret_cast<const float4*>(ab__ + offa[j]);                              \
    if (B_PL) {                                                                                \
      _Pragma("unroll") for (int p = 0; p < NP; ++p)                                           \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                            \
          pbp[p][j] = *reinterpret_cast<const x6_u32x4*>(g.bp0 + p * g.bp_stride + bo__ + offb[j]); \
    } else {                                                                                   \
      _Pragma("unroll") for (int j = 0; j < 4; ++j)                                            \
          pbf[j] = *reinterpret_cast<const float4*>(g.b.p0 + bo__ + offb[j]);                  \
    }                                                                                          \
  } while (0)
#define X6_LSTORE(st_)                                                                         \
  do {                                                                                         \
    unsigned char* s__ = (st_);                                                                \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                            \
      x6_u32x2 pc__[NP];                                                                       \
      x6_split4n<NP>(pa[j], pc__);                                                             \
      _Pragma("unroll") for (int p = 0; p < NP; ++p)                                           \
          *reinterpret_cast<x6_u32x2*>(s__ + p * X_APL + sta[j]) = pc__[p];                    \
    }                                                                                          \
    if (B_PL) {                                                                                \
      _Pragma("unroll") for (int p = 0; p < NP; ++p)                                           \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                            \
          *reinterpret_cast<x6_u32x4*>(s__ + 3 * X_APL + p * X_BPL + stb[j]) = pbp[p][j];      \
    } else {                                                                                   \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                          \
        x6_u32x2 pc__[NP];                                                                     \
        x6_split4n<NP>(pbf[j], pc__);                                                          \
        _Pragma("unroll") for (int p = 0; p < NP; ++p)                                         \
            *reinterpret_cast<x6_u32x2*>(s__ + 3 * X_APL + p * X_BPL + stb[j]) = pc__[p];      \
      }                                                                                        \
    }                                                                                          \
  } while (0)

  // Balanced schedule (pre-split B: forward, dgrad): the A tile is split in the SECOND half of the
  // iteration before it is written, so the two halves carry about the same non-MFMA issue load
  // (first half: LDS writes + B loads; second half: split VALU + A loads).  Stamps before: 2127 / 1643
  // cycles per half against 1536 of MFMAs.
  constexpr bool BAL = B_PL;
  x6_u32x2 pk[2][NP];   // packed pieces of the A tile (BAL)
#define X6_GLOAD_A(k0_)                                                                        \
  do {                                                                                         \
    const float* ab__ = abase(k0_);                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
        pa[j] = *reinterpret_cast<const float4*>(ab__ + offa[j]);                              \
  } while (0)
#define X6_GLOAD_B(k0_)                                                                        \
  do {                                                                                         \
    const int64_t bo__ = boff(k0_);                                                            \
    _Pragma("unroll") for (int p = 0; p < NP; ++p)                                             \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
        pbp[p][j] = *reinterpret_cast<const x6_u32x4*>(g.bp0 + p * g.bp_stride + bo__ + offb[j]); \
  } while (0)
#define X6_SPLIT_A()                                                                           \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) x6_split4n<NP>(pa[j], pk[j]);
#define X6_LSTORE_PK(st_)                                                                      \
  do {                                                                                         \
    unsigned char* s__ = (st_);                                                                \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
    _Pragma("unroll") for (int p = 0; p < NP; ++p)                                             \
        *reinterpret_cast<x6_u32x2*>(s__ + p * X_APL + sta[j]) = pk[j][p];                     \
    _Pragma("unroll") for (int p = 0; p < NP; ++p)                                             \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
        *reinterpret_cast<x6_u32x4*>(s__ + 3 * X_APL + p * X_BPL + stb[j]) = pbp[p][j];        \
  } while (0)

  // ---- fragment addresses.  v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) + 0..7]
  //      and B[k = 8 (l >> 4) + 0..7][col l & 15].
  const int fr = lane & 15, fc = lane >> 4;
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  int fao[4], fbo[4];   // row images use [0] + 1024 * tile; transposed images one address per tile
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    fao[i] = A_TR ? x6_tr_off(8 * fc + tq, (wm + 16 * i + 4 * tp) * 2, 256) : x6_row_off(wm + 16 * i + fr, fc);
    fbo[i] = 3 * X_APL + (B_TR ? x6_tr_off(8 * fc + tq, (wn + 16 * i + 4 * tp) * 2, 512)
                               : x6_row_off(wn + 16 * i + fr, fc));
  }
  // four fragment sets of two tiles each; quarter-phase order (A01,B01) (A23,B01) | (A01,B23) (A23,B23):
  // every set is reloaded while the MFMAs of another phase run, 96 fragment VGPRs in all
  x6_bf16x8 fA01[2][NP], fA23[2][NP], fB01[2][NP], fB23[2][NP];   // NP = 2: 64 fragment VGPRs
#define X6_LD_A(dst_, st_, i0_)                                                                \
  _Pragma("unroll") for (int ii = 0; ii < 2; ++ii)                                             \
  _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                             \
    if (A_TR) dst_[ii][p] = x6_tr_frag((st_) + p * X_APL + fao[(i0_) + ii], 256);              \
    else dst_[ii][p] = *reinterpret_cast<const x6_bf16x8*>((st_) + p * X_APL + fao[0] + ((i0_) + ii) * 1024); \
  }
#define X6_LD_B(dst_, st_, j0_)                                                                \
  _Pragma("unroll") for (int jj = 0; jj < 2; ++jj)                                             \
  _Pragma("unroll") for (int p = 0; p < NP; ++p) {                                             \
    if (B_TR) dst_[jj][p] = x6_tr_frag((st_) + p * X_BPL + fbo[(j0_) + jj], 512);              \
    else dst_[jj][p] = *reinterpret_cast<const x6_bf16x8*>((st_) + p * X_BPL + fbo[0] + ((j0_) + jj) * 1024); \
  }
// 2 x 2 tiles x 6 (NP = 3) or 3 (NP = 2) partial products, smallest first, the MFMAs of one accumulator back to back
// (chained MFMAs on one accumulator issue fastest; interleaving accumulators cost 26 %)
#define X6_MM(a_, b_, i0_, j0_)                                                                \
  _Pragma("unroll") for (int ii = 0; ii < 2; ++ii)                                             \
  _Pragma("unroll") for (int jj = 0; jj < 2; ++jj) {                                           \
    if constexpr (NP == 3) {                                                                   \
      X6_MFMA(a_[ii][NP - 1], b_[jj][0], acc[(i0_) + ii][(j0_) + jj]);                         \
      X6_MFMA(a_[ii][0], b_[jj][NP - 1], acc[(i0_) + ii][(j0_) + jj]);                         \
      X6_MFMA(a_[ii][1], b_[jj][1], acc[(i0_) + ii][(j0_) + jj]);                              \
    }                                                                                          \
    X6_MFMA(a_[ii][1], b_[jj][0], acc[(i0_) + ii][(j0_) + jj]);                                \
    X6_MFMA(a_[ii][0], b_[jj][1], acc[(i0_) + ii][(j0_) + jj]);                                \
    X6_MFMA(a_[ii][0], b_[jj][0], acc[(i0_) + ii][(j0_) + jj]);                                \
  }

  // wgrad only: db[n] = sum_m dY[m][n] falls out of the A tiles already in registers (weights 0/1
  // instead of branches; only the first column of workgroups contributes)
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  const float bw0 = (MODE == X6_WGRAD && g.bias_slab && n0 == 0) ? 1.f : 0.f;
#define X6_BSUM(w_)                                                                            \
  _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                              \
    bsum.x = fmaf(w_, pa[j].x, bsum.x); bsum.y = fmaf(w_, pa[j].y, bsum.y);                    \
    bsum.z = fmaf(w_, pa[j].z, bsum.z); bsum.w = fmaf(w_, pa[j].w, bsum.w);                    \
  }

#ifdef GCT_STAMPS
  unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory");
#endif
  // K-tiles of this workgroup: the range [kbeg, kend), or -- wgrad with a tile list -- an equal share of the
  // listed 32-row tiles (the tiles of the token rows whose gradient is not identically zero; the count lives
  // in device memory so that no host round trip is needed)
  int64_t nkt = (kend - kbeg) / XBK;
  int64_t lt0 = 0;
  const int32_t* klist = (MODE == X6_WGRAD) ? g.kt_list : nullptr;
  if (klist) {
    const int64_t cnt = *g.kt_count;
    const int64_t per = (cnt + g.nsplit - 1) / g.nsplit;
    lt0 = (int64_t)z * per;
    nkt = cnt - lt0 < per ? cnt - lt0 : per;
    if (nkt < 0) nkt = 0;
  }
  // the workgroup's share of the list is copied into LDS once: a scalar (SMEM) load per K-tile would make the
  // loop wait on lgkmcnt(0), i.e. on every LDS fragment read in flight
  int32_t* kl_s = reinterpret_cast<int32_t*>(xlds + 2 * X_STAGE);
  const bool kl_cached = klist && nkt <= X_KLIST_MAX;
  if (kl_cached) {
    for (int i = tid; i < nkt; i += 512) kl_s[i] = klist[lt0 + i];
    __syncthreads();
  }
  auto ktile = [&](int64_t t) -> int64_t {
    const int64_t tc = t < nkt ? t : nkt - 1;
    if (kl_cached) return (int64_t)__builtin_amdgcn_readfirstlane(kl_s[tc]) * XBK;
    return klist ? (int64_t)klist[lt0 + tc] * XBK : kbeg + tc * XBK;
  };
  if (nkt > 0) {
    if (BAL) {
      X6_GLOAD_A(ktile(0));
      X6_GLOAD_B(ktile(0));
      X6_SPLIT_A()
      X6_LSTORE_PK(xlds);
      X6_GLOAD_A(ktile(1));
      X6_GLOAD_B(ktile(1));
      X6_SPLIT_A()              // pk / pbp: tile 1
      X6_GLOAD_A(ktile(2));     // pa: tile 2, split in the second half of iteration 0
    } else {
      X6_GLOAD(ktile(0));
      if (MODE == X6_WGRAD) { X6_BSUM(bw0) }
      X6_LSTORE(xlds);
      X6_GLOAD(ktile(1));
    }
  }
  __syncthreads();
  if (nkt > 0) {
    X6_LD_A(fA01, xlds, 0)
    X6_LD_B(fB01, xlds, 0)
  }
  STAMP(0);
  constexpr int RA = 2 * NP * (A_TR ? 2 : 1), RB = 2 * NP * (B_TR ? 2 : 1);   // LDS reads per two-tile fragment set
  constexpr int NWR = B_PL ? 4 * NP : 6 * NP;             // LDS stores per K-tile
  // issue-order hints below: the NP = 3 counts are the tuned ones; NP = 2 has half the MFMAs and about half the
  // split VALU work per K-tile, and its groups are scaled to match (not retuned)
  constexpr int NG = 2 * NP;                              // MFMA / LDS-read groups per fragment-set load
  constexpr int MPW = NP == 3 ? 2 : 1;                    // MFMAs per LDS store (BAL, first half)
  // ... inside the steady state every index is below nkt: no clamp
  auto ktile_in = [&](int64_t t) -> int64_t { return kbeg + t * XBK; };
  int64_t k2n = nkt > 0 ? ktile(2) : 0;   // K index of tile t+2, looked up one iteration ahead: the scalar load
                                          // of a tile-list entry never sits in front of the loads that use it
  // One K-tile.  TAIL = 0 is the steady state.  The balanced schedule peels its last three K-tiles, so that nothing is
  // loaded, split, written to LDS or read from it for a tile that does not exist: tile t of nkt stores and reads tile
  // t+1 (NEXT1), loads B of and splits tile t+2 (NEXT2) and loads A of tile t+3 (NEXT3):
  //   TAIL 3 (t = nkt-3): no A load            TAIL 2 (t = nkt-2): LDS stores and fragment reads of tile nkt-1 only
  //   TAIL 1 (t = nkt-1): the MFMAs and the reads of A23 / B23; TAIL 4 is TAIL 1 with the epilogue's own operand reads
  //   (epi_ahead_issue) in the issue slots that the B loads leave free: one patch in the first half, one in the third
  //   quarter (B01 fragments dead), two in the last (A01 dead too): any earlier and the 64 operand registers do not fit
  //   in 256 VGPRs next to the accumulators and the fragments
  // The issue-order hints are those of the steady state with the groups of the missing work left out.
  const int64_t mw = m0 + wm, nw = n0 + wn;
  constexpr int SIDE = MODE == X6_FWD ? 1 : (MODE == X6_DGRAD ? 2 : 3);
  EpiLane el;
  EpiAhead ah;
  float4 ex[4][4];
  int qv[4];
  if (BAL) epi_ahead_quads<SIDE>(g, lane, mw, nw, qv);
  auto ktile_iter = [&](auto tail_c, const int64_t kt) __attribute__((always_inline)) {
    constexpr int TAIL = decltype(tail_c)::value;
    constexpr bool NEXT1 = TAIL != 1 && TAIL != 4, NEXT2 = TAIL == 0 || TAIL == 3, NEXT3 = TAIL == 0, AHEAD = TAIL == 4;
    unsigned char* st = xlds + (kt & 1) * X_STAGE;
    unsigned char* stn = xlds + ((kt + 1) & 1) * X_STAGE;
    const int64_t k2 = k2n;
    if (TAIL == 0) k2n = BAL ? ktile_in(kt + 3) : ktile(kt + 3);
    __builtin_amdgcn_sched_barrier(0);
    // ---- first half: phases (A01,B01) (A23,B01) | reads of A23, B23; split + LDS stores of tile t+1
    X6_LD_A(fA23, st, 2)
    X6_LD_B(fB23, st, 2)
    if (MODE == X6_WGRAD) {
      const float bw = (kt + 1 < nkt) ? bw0 : 0.f;
      X6_BSUM(bw)
    }
    if (BAL) {
      if (NEXT1) { X6_LSTORE_PK(stn); }   // tile t+1: A pieces split last iteration, B pieces as loaded
      if (NEXT2) { X6_GLOAD_B(k2); }
      if (AHEAD) epi_ahead_issue<0, 1>(g, ah, ex);
    } else {
      X6_LSTORE(stn);
    }
    X6_MM(fA01, fB01, 0, 0)
    X6_MM(fA23, fB01, 2, 0)
#pragma unroll
    for (int q = 0; q < NG; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, (RA + RB) / NG, 0);
    }
    if (BAL) {
#pragma unroll
      for (int q = 0; q < (NEXT1 ? NWR : 0); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, MPW, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
#pragma unroll
      for (int q = 0; q < (NEXT2 ? 2 * NP : (AHEAD ? 4 : 0)); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < (NP == 3 ? 21 : 8); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, NP == 3 ? 6 : 9, 0);
      }
#pragma unroll
      for (int q = 0; q < NWR; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(1);
    __syncthreads();
    STAMP(2);
    // ---- second half: phases (A01,B23) (A23,B23) | reads of B01, A01 of tile t+1; global loads of tile t+2
    if (NEXT1) { X6_LD_B(fB01, stn, 0) }
    if (BAL) {
      if (NEXT2) { X6_SPLIT_A() }   // pa holds tile t+2 (loaded one iteration ago)
      if (NEXT3) { X6_GLOAD_A(k2n); }
      if (AHEAD) epi_ahead_issue<1, 2>(g, ah, ex);
    } else {
      X6_GLOAD(k2);
    }
    X6_MM(fA01, fB23, 0, 2)
#pragma unroll
    for (int q = 0; q < (NEXT1 ? NG : 0); ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, RB / NG, 0);
    }
    if (BAL) {
#pragma unroll
      for (int q = 0; q < (NEXT2 ? (NP == 3 ? 14 : 6) : 0); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, NP == 3 ? 3 : 4, 0);
      }
      if (NEXT3) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
      }
#pragma unroll
      for (int q = 0; q < (AHEAD ? 4 : 0); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < (NP == 3 ? 8 : 4); ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (NEXT1) { X6_LD_A(fA01, stn, 0) }
    if (AHEAD) epi_ahead_issue<2, 4>(g, ah, ex);
    X6_MM(fA23, fB23, 2, 2)
#pragma unroll
    for (int q = 0; q < (AHEAD ? 8 : 0); ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
#pragma unroll
    for (int q = 0; q < (NEXT1 ? NG : 0); ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, RA / NG, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(3);
    };
  if (BAL) {
    int64_t kt = 0;
    for (; kt < nkt - 3; ++kt) ktile_iter(std::integral_constant<int, 0>{}, kt);
    // the epilogue's lane mapping depends on the block origin and the lane alone: resolved here, its loads (bias,
    // quad map) are in flight under the last K-tiles
    el = epi_lane(g, lane, nw, z);
    const bool ahead = nkt > 0 && epi_ahead_ok<SIDE>(g);
    ah.have = 0;
    if (ahead) ah = epi_ahead_plan<SIDE>(g, el, lane, mw, qv);
    if (nkt >= 3) ktile_iter(std::integral_constant<int, 3>{}, nkt - 3);
    if (nkt >= 2) ktile_iter(std::integral_constant<int, 2>{}, nkt - 2);
    if (ahead) ktile_iter(std::integral_constant<int, 4>{}, nkt - 1);
    else if (nkt >= 1) ktile_iter(std::integral_constant<int, 1>{}, nkt - 1);
    // No workgroup barrier here: after the barrier in the middle of the last K-tile no wave reads or writes a stage
    // (the A23 / B23 reads of that tile are issued before the barrier, which waits for them), so a wave may overwrite
    // LDS with its staging block as soon as its own MFMAs are done, while slower waves still run theirs.
  } else {
    for (int64_t kt = 0; kt < nkt; ++kt) ktile_iter(std::integral_constant<int, 0>{}, kt);
    __syncthreads();  // speculative fragment reads / stores of the idle stage must finish before LDS is reused
  }
#undef X6_GLOAD
#undef X6_GLOAD_A
#undef X6_GLOAD_B
#undef X6_SPLIT_A
#undef X6_LSTORE_PK
#undef X6_LSTORE
#undef X6_LD_A
#undef X6_LD_B
#undef X6_MM
#undef X6_BSUM
  if (MODE == X6_WGRAD) {
    if (g.bias_slab && n0 == 0) {            // block-uniform: combine the 16 k-row groups, fixed order
      float4* red = reinterpret_cast<float4*>(xlds);
      red[tid] = bsum;
      __syncthreads();
      if (tid < 32) {
        float4 t4 = red[tid];
        for (int r = 1; r < 16; ++r) {
          const float4 u = red[r * 32 + tid];
          t4.x += u.x; t4.y += u.y; t4.z += u.z; t4.w += u.w;
        }
        const int64_t col = m0 + tid * 4;
        if (col + 3 < g.M) *reinterpret_cast<float4*>(g.bias_slab + (int64_t)z * g.M + col) = t4;
      }
      __syncthreads();
    }
  }
  STAMP(4);
  {
    // 16 x 16 accumulator tiles -> the wave's 64 x 64 staging block, then the shared epilogue tail
    float* stg = reinterpret_cast<float*>(xlds) + wave * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[(16 * i + 4 * fc + r) * 64 + 16 * j + fr] = acc[i][j][r];
#ifdef GCT_LAB_NO_EPI         // tools/gemm_lab.hip: main loop only
    if (acc[0][0][0] == 123456.789f)
#endif
    {
      if (BAL) wave_epilogue_finish<SIDE>(g, stg, lane, mw, el, ex, ah.have);
      else wave_epilogue_tail<SIDE>(g, stg, lane, mw, nw, z);
    }
  }
#ifdef GCT_STAMPS
  __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0): include the stores' completion
  STAMP(5);
  if (g.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 64) {
    for (int i = 0; i < 8; ++i) g.stamps[((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * 8 + i] = seg[i];
  }
#endif
}

template <int MODE, int NP = 3>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void
gemm_x6_kernel(const GemmArgs g) {
  gemm_x6_body<MODE, NP>(g, blockIdx.x, gridDim.x);
}

// One Linear's backward as ONE grid: blocks [0, n_wgrad_blocks) are the weight-gradient workgroups of gw (the longer
// ones, so they start first; they also pull dY through the L2 before the dgrad tiles read it), the rest the dgrad tiles
// of gd.  The branch is block-uniform and taken once; each side runs exactly the code of its own kernel (same MFMA and
// accumulation order), so dX, db and -- at equal split counts -- dW are bit-identical to the separate launches.
template <int NP = 3>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void
gemm_x6_bwd_pair_kernel(const GemmArgs gw, const GemmArgs gd, const unsigned n_wgrad_blocks) {
  if (blockIdx.x < n_wgrad_blocks) gemm_x6_body<X6_WGRAD, NP>(gw, blockIdx.x, n_wgrad_blocks);
  else gemm_x6_body<X6_DGRAD, NP>(gd, blockIdx.x - n_wgrad_blocks, gridDim.x - n_wgrad_blocks);
}

// "this launch can take gemm_x6_kernel<MODE>" -- everything else stays on the fp32-MFMA kernels
template <int MODE>
bool x6_ok(const GemmArgs& g, bool vec, int fwd_bn = XBN) {     // fwd_bn: weight rows of one tile (segments are whole tiles)
  auto seg_ok = [](int64_t nper, int64_t extent, int64_t gran) { return nper >= extent || nper % gran == 0; };
  const bool common = vec && g.K % XBK == 0 && g.ksplit % XBK == 0 && g.K >= XBK && g.M >= 8 && g.N >= 8 &&
      g.N % 4 == 0 && g.ldc % 4 == 0 && gct_aligned16(g.c0) && g.c_d1 % 4 == 0 && g.c_d2 % 4 == 0 &&
      (g.c_nper >= g.N || g.c_nper % 4 == 0) && g.slab_stride % 4 == 0 &&
      (!g.bias0 || (gct_aligned16(g.bias0) && g.bias_d1 % 4 == 0 && g.bias_d2 % 4 == 0)) &&
      (!g.resid || gct_aligned16(g.resid)) && (!g.pre || gct_aligned16(g.pre)) &&
      (!g.pre_in || gct_aligned16(g.pre_in)) && 130 * g.lda < (1ll << 31) && 260 * g.ldb < (1ll << 31);
  if (!common) return false;
  if (MODE == X6_FWD)
    return g.bp0 && seg_ok(g.a_nper, g.K, XBK) && seg_ok(g.b_nper, g.N, fwd_bn) && g.ldb % 8 == 0 &&
           g.b.d1 % 8 == 0 && g.b.d2 % 8 == 0 && g.bp_stride % 8 == 0 && (((uintptr_t)g.bp0) & 15u) == 0;
  if (MODE == X6_DGRAD)
    return g.bp0 && seg_ok(g.a_nper, g.K, XBK) && seg_ok(g.b_nper, g.K, XBK) && g.N % 8 == 0 && g.ldb % 8 == 0 &&
           g.b.d1 % 8 == 0 && g.b.d2 % 8 == 0 && g.bp_stride % 8 == 0 && (((uintptr_t)g.bp0) & 15u) == 0;
  return seg_ok(g.a_nper, g.M, XBM) && g.M % 4 == 0;
}

template <int MODE, int NP>
int launch_x6(const GemmArgs& g, hipStream_t st) {
  const int64_t tiles = ((g.M + XBM - 1) / XBM) * ((g.N + XBN - 1) / XBN) * g.nsplit;
  if (tiles <= 0) return GCT_OK;
  if (tiles > INT_MAX) {
    gct_set_error("gemm_x6: grid too large");
    return GCT_ERR_ARG;
  }
  static bool attr_set = false;   // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)gemm_x6_kernel<MODE, NP>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, X_LDS_BYTES);
    if (e != hipSuccess) {
      gct_set_error("gemm_x6: cannot reserve %d bytes of LDS: %s", X_LDS_BYTES, hipGetErrorString(e));
      return GCT_ERR_HIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm_x6_kernel<MODE, NP>), dim3((unsigned)tiles), dim3(512), X_LDS_BYTES, st, g);
  ++(NP == 3 ? g_x6_kernel_launches : g_x3_kernel_launches);
  GCT_LAUNCH_CHECK("gemm_x6");
  return GCT_OK;
}

// =====================================================================================
// Small-tile forward variant: 64 x 128 x 32 tiles, 8 waves (2 x 4) of 32 x 32 = 2 x 2 MFMA tiles.  For forward GEMMs
// whose 128 x 256 tiling would leave most CUs idle -- the N = 512 / 1 024 projections of a decode step with 2 000-4 000
// rows, or of a training step at batch 64 -- four times as many workgroups, 72 KB of LDS (two stages of {A 3 x 4 KB,
// B 3 x 8 KB}: two workgroups per CU).  Same arithmetic (six bf16 partial products of the exact 3-way split, fp32
// accumulate), same operand layout (x fp32 [M][K] split on the fly, W pre-split planes [N][K]), same epilogues;
// a plain two-stage pipeline (loads of tile t+2 and LDS stores of tile t+1 during the MFMAs of tile t, one barrier
// per K-tile) -- these launches are a few microseconds long, the large kernel's hand-placed schedule is not needed.
// =====================================================================================
constexpr int SBM = 64, SBN = 128;
constexpr int XS_APL = SBM * 64, XS_BPL = SBN * 64, XS_STAGE = 3 * XS_APL + 3 * XS_BPL;   // 36 KB per stage
constexpr int XS_LDS_BYTES = 2 * XS_STAGE;

// MODE = X6_FWD: B = W planes [N][K] (row reads); X6_DGRAD: A = dY [M][K'] (K' segmented), B = W planes [K'][N] natural,
// transposed reads -- the tail rows of a tail-balanced dgrad launch (gemm.hip launch_x6_tail_split).  NP as for
// gemm_x6_kernel (3: bf16x6, 2: bf16x3; same LDS layout).
template <int MODE, int NP = 3>
__global__ __launch_bounds__(512) void gemm_x6s_kernel(const GemmArgs g) {
  static_assert(NP == 2 || NP == 3, "bf16x3 or bf16x6");
  extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
  constexpr bool B_TR = MODE == X6_DGRAD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 2) * 32, wn = (wave & 3) * 32;
  const unsigned tiles_n = (unsigned)((g.N + SBN - 1) / SBN);
  const unsigned lid = gct_xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (int64_t)(lid / tiles_n) * SBM, n0 = (int64_t)(lid % tiles_n) * SBN;
  // one float4 of A and one 16-B chunk of each B plane per thread and K-tile (edge rows / columns clamped into valid
  // memory: they only feed accumulator rows / columns that are never stored)
  int64_t ra = tid >> 3, rb = tid >> 2;
  const int sta = x6_row_off((int)ra, (tid & 7) >> 1) + (tid & 1) * 8;
  const int stb = B_TR ? x6_tr_off(tid >> 4, (tid & 15) * 16, 256) : x6_row_off((int)rb, tid & 3);
  if (m0 + ra > g.M - 1) ra = g.M - 1 - m0;
  if (n0 + rb > g.N - 1) rb = g.N - 1 - n0;
  const float* ap = g.a.p0 + (m0 + ra) * g.lda + (tid & 7) * 4;
  int64_t bo;
  if (B_TR) {
    int64_t c = (tid & 15) * 8;
    if (n0 + c > g.N - 8) c = g.N - 8 - n0;
    bo = (int64_t)(tid >> 4) * g.ldb + n0 + c;
  } else {
    const bool s1 = n0 >= g.b_nper, s2 = n0 >= 2 * g.b_nper;   // the 128 weight rows lie in one segment
    bo = (s2 ? g.b.d2 : (s1 ? g.b.d1 : 0)) + (n0 - (s2 ? 2 * g.b_nper : (s1 ? g.b_nper : 0)) + rb) * g.ldb + (tid & 3) * 8;
  }
  const uint16_t* bp = g.bp0 + bo;
  // K-tile k0 -> element offsets of its A columns / B rows (DGRAD: K' is segmented like the forward's outputs; a K-tile
  // lies in one segment)
  auto koff = [&](int64_t k0, int64_t& ao, int64_t& bko) {
    if (!B_TR) { ao = k0; bko = k0; return; }
    const bool a1 = k0 >= g.a_nper, a2 = k0 >= 2 * g.a_nper;
    ao = (a2 ? g.a.d2 : (a1 ? g.a.d1 : 0)) + (k0 - (a2 ? 2 * g.a_nper : (a1 ? g.a_nper : 0)));
    const bool b1 = k0 >= g.b_nper, b2 = k0 >= 2 * g.b_nper;
    bko = (b2 ? g.b.d2 : (b1 ? g.b.d1 : 0)) + (k0 - (b2 ? 2 * g.b_nper : (b1 ? g.b_nper : 0))) * g.ldb;
  };

  x6_f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = x6_f32x4{0.f, 0.f, 0.f, 0.f};
  float4 pa;
  x6_u32x4 pb[NP];
  auto gload = [&](int64_t k0) {
    int64_t ao, bko;
    koff(k0, ao, bko);
    pa = *reinterpret_cast<const float4*>(ap + ao);
#pragma unroll
    for (int p = 0; p < NP; ++p) pb[p] = *reinterpret_cast<const x6_u32x4*>(bp + p * g.bp_stride + bko);
  };
  auto lstore = [&](unsigned char* st) {
    x6_u32x2 pc[NP];
    x6_split4n<NP>(pa, pc);
#pragma unroll
    for (int p = 0; p < NP; ++p) *reinterpret_cast<x6_u32x2*>(st + p * XS_APL + sta) = pc[p];
#pragma unroll
    for (int p = 0; p < NP; ++p) *reinterpret_cast<x6_u32x4*>(st + 3 * XS_APL + p * XS_BPL + stb) = pb[p];
  };
  const int fr = lane & 15, fc = lane >> 4;
  const int tq = (lane & 15) >> 2, tp = lane & 3;
  const int fao = x6_row_off(wm + fr, fc);                     // + 1024 per 16-row tile
  int fbo[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    fbo[j] = 3 * XS_APL + (B_TR ? x6_tr_off(8 * fc + tq, (wn + 16 * j + 4 * tp) * 2, 256)
                                : x6_row_off(wn + fr, fc) + j * 1024);
  const int64_t nkt = g.K / XBK;
  gload(0);
  lstore(xlds);
  if (nkt > 1) gload(XBK);
  __syncthreads();
  for (int64_t kt = 0; kt < nkt; ++kt) {
    const unsigned char* st = xlds + (kt & 1) * XS_STAGE;
    x6_bf16x8 fa[2][NP], fb[2][NP];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        fa[i][p] = *reinterpret_cast<const x6_bf16x8*>(st + p * XS_APL + fao + i * 1024);
        if (B_TR) fb[i][p] = x6_tr_frag(st + p * XS_BPL + fbo[i], 256);
        else fb[i][p] = *reinterpret_cast<const x6_bf16x8*>(st + p * XS_BPL + fbo[i]);
      }
    if (kt + 1 < nkt) lstore(xlds + ((kt + 1) & 1) * XS_STAGE);      // tile t+1 (loaded one iteration ago)
    if (kt + 2 < nkt) gload((kt + 2) * XBK);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (NP == 3) {
          X6_MFMA(fa[i][NP - 1], fb[j][0], acc[i][j]);
          X6_MFMA(fa[i][0], fb[j][NP - 1], acc[i][j]);
          X6_MFMA(fa[i][1], fb[j][1], acc[i][j]);
        }
        X6_MFMA(fa[i][1], fb[j][0], acc[i][j]);
        X6_MFMA(fa[i][0], fb[j][1], acc[i][j]);
        X6_MFMA(fa[i][0], fb[j][0], acc[i][j]);
      }
#ifndef GCT_X6S_PLAIN
    // issue order: the MFMAs of the first row tile start as soon as its fragments are in; the second row tile's
    // fragments, the split of tile t+1, its LDS stores and the loads of tile t+2 go between the MFMAs (NP = 2: 12
    // MFMAs, 8 / 12 reads, 4 stores, 3 loads per K-tile -- the same order with scaled counts, not retuned)
    __builtin_amdgcn_sched_group_barrier(0x100, NP == 3 ? (B_TR ? 15 : 9) : (B_TR ? 10 : 6), 0);
#pragma unroll
    for (int q = 0; q < (NP == 3 ? 3 : 2); ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, NP == 3 ? 2 : 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
#pragma unroll
    for (int q = 0; q < (NP == 3 ? 6 : 3); ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, NP == 3 ? 5 : 4, 0);
    }
#pragma unroll
    for (int q = 0; q < 2 * NP; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
#pragma unroll
    for (int q = 0; q < NP + 1; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    if constexpr (NP == 3) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#endif
    __syncthreads();
  }
  // epilogue: per-wave 32 x 32 transpose through LDS (the stages are free after the last barrier), 4 x 4 patch per lane
  float* stg = reinterpret_cast<float*>(xlds) + wave * 1024;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) stg[(16 * i + 4 * fc + r) * 32 + 16 * j + fr] = acc[i][j][r];
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  const FastEpiT<MODE == X6_FWD ? 1 : 2> ep{g};
  const int rg = lane >> 3, c4 = lane & 7;
  const int64_t row0 = m0 + wm + rg * 4, col0 = n0 + wn + c4 * 4;
  if (row0 < g.M && col0 < g.N) {
    float4 v[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) v[rr] = *reinterpret_cast<const float4*>(stg + (rg * 4 + rr) * 32 + c4 * 4);
    const bool q1 = col0 >= g.c_nper, q2 = col0 >= 2 * g.c_nper;
    const int64_t cloc = col0 - (q2 ? 2 * g.c_nper : (q1 ? g.c_nper : 0));
    float* cbase = g.c0 + (q2 ? g.c_d2 : (q1 ? g.c_d1 : 0));
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g.epi < EPI_D0 && g.bias0)
      bias = *reinterpret_cast<const float4*>(g.bias0 + (q2 ? g.bias_d2 : (q1 ? g.bias_d1 : 0)) + cloc);
    ep.apply(v, row0, col0, cbase, cloc, bias);
  }
}

// "this forward launch can take gemm_x6s_kernel": everything x6_ok<X6_FWD> asks, one K range, plain A, 128-row weight
// tiles inside one segment
inline bool x6s_ok(const GemmArgs& g, bool vec) {
  return x6_ok<X6_FWD>(g, vec, SBN) && g.nsplit == 1 && g.a_nper >= g.K && (g.b_nper >= g.N || g.b_nper % SBN == 0) &&
         (g.c_nper >= g.N || g.c_nper % 4 == 0) && g.epi < EPI_D0 && 70 * g.lda < (1ll << 31);
}
// ... and the dgrad variant (dense dX, any dgrad epilogue)
inline bool x6s_dgrad_ok(const GemmArgs& g, bool vec) {
  return x6_ok<X6_DGRAD>(g, vec) && g.nsplit == 1 && g.c_nper >= g.N && g.epi >= EPI_D0 && g.epi < EPI_SLAB &&
         70 * g.lda < (1ll << 31) && 40 * g.ldb < (1ll << 31);
}

template <int MODE, int NP>
inline int launch_x6s(const GemmArgs& g, hipStream_t st) {
  const int64_t tiles = ((g.M + SBM - 1) / SBM) * ((g.N + SBN - 1) / SBN);
  if (tiles <= 0) return GCT_OK;
  static bool attr_set = false;        // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)gemm_x6s_kernel<MODE, NP>, hipFuncAttributeMaxDynamicSharedMemorySize, XS_LDS_BYTES);
    if (e != hipSuccess) {
      gct_set_error("gemm_x6s: cannot reserve %d bytes of LDS: %s", XS_LDS_BYTES, hipGetErrorString(e));
      return GCT_ERR_HIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm_x6s_kernel<MODE, NP>), dim3((unsigned)tiles), dim3(512), XS_LDS_BYTES, st, g);
  ++(NP == 3 ? g_x6_kernel_launches : g_x3_kernel_launches);
  GCT_LAUNCH_CHECK("gemm_x6s");
  return GCT_OK;
}

// fp32 -> three bf16 planes (elementwise over a flat buffer; tensor boundaries are irrelevant)
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ src, uint16_t* __restrict__ planes,
                                                           int64_t n4, int64_t pstride) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(src)[i];
  x6_u32x2 h, m, l;
  x6_split4(v, h, m, l);
  *reinterpret_cast<x6_u32x2*>(planes + 4 * i) = h;
  *reinterpret_cast<x6_u32x2*>(planes + pstride + 4 * i) = m;
  *reinterpret_cast<x6_u32x2*>(planes + 2 * pstride + 4 * i) = l;
}
