// K3: nn.Linear forward / dgrad / wgrad as one LDS-tiled fp32-input MFMA GEMM family.
//
// Reference call sites: Model/sublayers.py:54-59,64-66,70,81-88 ; Model/vaetf.py:81,133.
//
// Machine mapping (gfx950):
//   * v_mfma_f32_32x32x2_f32: exact fp32 fma chains (parity with the fp32 reference),
//     64 FLOP/clk/SIMD => 157 TFLOP/s chip peak (the roofline these kernels are priced on).
//   * block tile 128x128x32, 4 waves (2x2), each wave 64x64 = 2x2 MFMA tiles, 64 acc VGPRs.
//   * operands staged HBM -> VGPR -> LDS (two LDS buffers, register prefetch of tile t+1
//     issued before the MFMAs of tile t, written after them: one barrier per K-tile).
//   * K-contiguous operands use a 16-B-chunk XOR swizzle so the ds_read_b128 fragment
//     reads are bank-conflict free; row-contiguous operands are read with ds_read_b32.
//   * lane half h owns k = 16h..16h+15 of every 32-wide K-tile for BOTH operands, so each
//     lane's fragment is 16 contiguous floats (4 x ds_read_b128) -- any k permutation is
//     legal as long as A and B agree.
//   * 1-D grid with the bijective XCD remap: the N-tiles that share an A row-panel get
//     consecutive logical ids => same XCD L2.
//   * "segmented" operands: q/k/v (mu/log_var) weights stay separate checkpoint tensors,
//     the kernel selects the base pointer per 4-element chunk.
#include <limits.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int TILE_FLOATS = BM * BK;  // 4096 floats = 16 KB per operand tile

// A segmented matrix is addressed as base + {0, d1, d2}[segment] + ...: ONE pointer plus integer
// element offsets (computed on the host).  Selecting among integer offsets compiles to
// v_cndmask; selecting among pointers made hipcc either reload the pointer from kernarg memory
// in front of every tile load or build an LDS lookup table and fall back to flat_load.
struct Seg3 {
  const float* p0;
  int64_t d1, d2;
};

struct GemmArgs {
  int64_t M, N, K;  // logical C[M][N] = A[M][K] B[K][N]
  Seg3 a;
  int64_t lda;
  int64_t a_nper;
  Seg3 b;
  int64_t ldb;
  int64_t b_nper;
  float* c0;
  int64_t c_d1, c_d2;
  int64_t ldc;
  int64_t c_nper;
  int64_t slab_stride;  // split-K: C written to c.p[0] + z*slab_stride
  int64_t ksplit;       // K range per split (multiple of BK), == K when no split
  int nsplit;
  int epi;              // fwd: GCT_EPI_* ; dgrad: 16 + GCT_DEPI_* ; slab: 32
  const float* bias0;  // nullptr: no bias
  int64_t bias_d1, bias_d2;
  const float* resid;
  float* pre;
  const float* pre_in;
  float keep_scale;
  uint32_t thr;
  GctRng rng;
  float* bias_slab;  // wgrad fast path: per-split column sums of dY, [nsplit][M] (nullptr: off)
  int64_t row_base;  // rows in front of this launch's row 0 (a launch on a row range keeps the dropout coordinates)
  const int32_t* quad_map;  // rows are a quad compaction (csrc/liverows.hip): dropout coordinates of compact quad q are
                            // those of original quad quad_map[q] (nullptr: identity)
  int64_t pre_rows;         // > 0 (with quad_map): pre_in keeps the forward's row space (pre_rows rows) and is read
                            // through the quad map -- no gathered copy of the 4d-wide pre-activation is needed
  const int32_t* kt_list;   // bf16x6 wgrad: ascending 32-row K-tile indices to reduce over (nullptr: all)
  const int32_t* kt_count;  // device scalar: entries of kt_list
  const uint16_t* bp0;  // bf16x6 kernels: pre-split planes of the B operand (same element offsets as b)
  int64_t bp_stride;    // elements between the hi / mid / lo planes
#ifdef GCT_STAMPS
  unsigned long long* stamps;  // diagnostic build only (tools/gemm_stamps.hip)
#endif
};

enum { EPI_SLAB = 32, EPI_D0 = 16 };

// row of pre_in that belongs to row `row` (+0..3, row % 4 == 0) of this launch; -1: none (padding)
__device__ __forceinline__ int64_t pre_row0(const GemmArgs& g, int64_t row) {
  if (g.pre_rows <= 0 || !g.quad_map) return row;
  const int v = g.quad_map[(row + g.row_base) >> 2];
  return v < 0 ? -1 : (int64_t)v * 4;
}

// quad (row >> 2) whose Philox stream covers `row` of this launch
__device__ __forceinline__ uint32_t drop_quad(const GemmArgs& g, int64_t row) {
  int64_t q = (row + g.row_base) >> 2;
  if (g.quad_map) {
    const int v = g.quad_map[q];
    q = v < 0 ? 0 : v;                 // padding quads: their rows are zero whatever the mask says
  }
  return (uint32_t)q;
}

#ifdef GCT_STAMPS
#define STAMP(i)                                                                       \
  do {                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    unsigned long long t__;                                                            \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");         \
    __builtin_amdgcn_sched_barrier(0);                                                 \
    seg[i] += t__ - tprev;                                                             \
    tprev = t__;                                                                       \
  } while (0)
#else
#define STAMP(i)
#endif

__device__ __forceinline__ const float* seg_ptr(const Seg3& s, int64_t idx, int64_t nper,
                                                int64_t& local) {
  // nseg <= 3: two compares instead of a 64-bit division
  const bool g1 = idx >= nper, g2 = idx >= 2 * nper;
  local = idx - (g2 ? 2 * nper : (g1 ? nper : 0));
  return s.p0 + (g2 ? s.d2 : (g1 ? s.d1 : 0));
}

// ---- global -> register tile loaders ------------------------------------------------
// "KC": tile rows indexed by the free dim (m or n), K contiguous in memory.
//   AK: A[m][k] = a.p[k/nper] + m*lda + k%nper        (segmented along k)
//   BK_: B[k][n] = b.p[n/nper] + (n%nper)*ldb + k      (segmented along rows n)
template <bool VEC, bool SEG_ON_K>
__device__ __forceinline__ void load_kc(float4 (&r)[4], const Seg3& s, int64_t ld, int64_t nper,
                                        int64_t row0, int64_t rows, int64_t k0, int64_t kend,
                                        int tid) {
  const int c8 = tid & 7;
  const int64_t k = k0 + c8 * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = row0 + (tid >> 3) + 32 * i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < rows) {
      if (VEC) {
        if (k < kend) {
          int64_t loc;
          const float* base;
          if (SEG_ON_K) {
            base = seg_ptr(s, k, nper, loc);
            v = *reinterpret_cast<const float4*>(base + row * ld + loc);
          } else {
            base = seg_ptr(s, row, nper, loc);
            v = *reinterpret_cast<const float4*>(base + loc * ld + k);
          }
        }
      } else {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (k + e < kend) {
            int64_t loc;
            if (SEG_ON_K) {
              const float* base = seg_ptr(s, k + e, nper, loc);
              t[e] = base[row * ld + loc];
            } else {
              const float* base = seg_ptr(s, row, nper, loc);
              t[e] = base[loc * ld + k + e];
            }
          }
        }
        v = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
    r[i] = v;
  }
}

// "RC": tile = 32 k-rows x 128 contiguous free-dim columns.
//   AM: A[m][k] = a.p[m/nper] + k*lda + m%nper        (segmented along columns m)
//   BN_: B[k][n] = b.p[k/nper] + (k%nper)*ldb + n      (segmented along rows k)
template <bool VEC, bool SEG_ON_K>
__device__ __forceinline__ void load_rc(float4 (&r)[4], const Seg3& s, int64_t ld, int64_t nper,
                                        int64_t col0, int64_t cols, int64_t k0, int64_t kend,
                                        int tid) {
  const int c32 = tid & 31;
  const int64_t col = col0 + c32 * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t k = k0 + (tid >> 5) + 8 * i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < kend) {
      if (VEC) {
        if (col < cols) {
          int64_t loc;
          if (SEG_ON_K) {
            const float* base = seg_ptr(s, k, nper, loc);
            v = *reinterpret_cast<const float4*>(base + loc * ld + col);
          } else {
            const float* base = seg_ptr(s, col, nper, loc);
            v = *reinterpret_cast<const float4*>(base + k * ld + loc);
          }
        }
      } else {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (col + e < cols) {
            int64_t loc;
            if (SEG_ON_K) {
              const float* base = seg_ptr(s, k, nper, loc);
              t[e] = base[loc * ld + col + e];
            } else {
              const float* base = seg_ptr(s, col + e, nper, loc);
              t[e] = base[k * ld + loc];
            }
          }
        }
        v = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
    r[i] = v;
  }
}

// ---- register -> LDS ------------------------------------------------------------------
__device__ __forceinline__ void store_kc(float* lds, const float4 (&r)[4], int tid) {
  const int c8 = tid & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (tid >> 3) + 32 * i;
    const int chunk = c8 ^ ((row >> 1) & 7);
    *reinterpret_cast<float4*>(lds + row * BK + chunk * 4) = r[i];
  }
}
__device__ __forceinline__ void store_rc(float* lds, const float4 (&r)[4], int tid) {
  const int c32 = tid & 31;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = (tid >> 5) + 8 * i;
    *reinterpret_cast<float4*>(lds + k * BM + c32 * 4) = r[i];
  }
}

// ---- LDS -> fragments, one QUARTER (4 k-values) at a time: f[t][e] holds k = 16*h + 4*c + e of
// free-dim index base+32t+(lane&31).  KC: one ds_read_b128 per t; RC: four ds_read_b32 per t.
__device__ __forceinline__ void fragq_kc(float (&f)[2][4], const float* lds, int base, int lane,
                                         int c) {
  const int h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int row = base + t * 32 + (lane & 31);
    const int sw = (row >> 1) & 7;
    const float4 v = *reinterpret_cast<const float4*>(lds + row * BK + (((h * 4 + c) ^ sw) * 4));
    f[t][0] = v.x; f[t][1] = v.y; f[t][2] = v.z; f[t][3] = v.w;
  }
}
__device__ __forceinline__ void fragq_rc(float (&f)[2][4], const float* lds, int base, int lane,
                                         int c) {
  const int h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int col = base + t * 32 + (lane & 31);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[t][e] = lds[(h * 16 + c * 4 + e) * BM + col];
  }
}

// A_KC: A is [M][K] K-contiguous (fwd, dgrad); else [K][M] (wgrad).
// B_KC: B is weights [N][K] (fwd); else [K][N] (dgrad, wgrad).
template <bool A_KC, bool B_KC, bool VEC>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[4 * TILE_FLOATS];  // A0 B0 A1 B1 : 64 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  const unsigned tiles_n = (unsigned)((g.N + BN - 1) / BN);
  const unsigned tiles_m = (unsigned)((g.M + BM - 1) / BM);
  const unsigned per_split = tiles_m * tiles_n;
  const unsigned lid = gct_xcd_remap(blockIdx.x, gridDim.x);
  const unsigned z = lid / per_split, rest = lid - z * per_split;
  const int64_t m0 = (int64_t)(rest / tiles_n) * BM, n0 = (int64_t)(rest % tiles_n) * BN;
  const int64_t kbeg = (int64_t)z * g.ksplit;
  const int64_t kend = (kbeg + g.ksplit < g.K) ? kbeg + g.ksplit : g.K;

  const Seg3 sa = g.a, sb = g.b;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[4], rb[4];
  auto gload = [&](int64_t k0) {
    if (A_KC)
      load_kc<VEC, true>(ra, sa, g.lda, g.a_nper, m0, g.M, k0, kend, tid);
    else
      load_rc<VEC, false>(ra, sa, g.lda, g.a_nper, m0, g.M, k0, kend, tid);
    if (B_KC)
      load_kc<VEC, false>(rb, sb, g.ldb, g.b_nper, n0, g.N, k0, kend, tid);
    else
      load_rc<VEC, true>(rb, sb, g.ldb, g.b_nper, n0, g.N, k0, kend, tid);
  };
  auto lstore = [&](int buf) {
    float* la = lds + buf * 2 * TILE_FLOATS;
    float* lb = la + TILE_FLOATS;
    if (A_KC) store_kc(la, ra, tid); else store_rc(la, ra, tid);
    if (B_KC) store_kc(lb, rb, tid); else store_rc(lb, rb, tid);
  };

  const int64_t nkt = (kend - kbeg + BK - 1) / BK;
#ifdef GCT_STAMPS
  unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory");
#endif
  if (nkt > 0) {
    gload(kbeg);
    lstore(0);
  }
  __syncthreads();
  STAMP(0);  // prologue
  for (int64_t kt = 0; kt < nkt; ++kt) {
    const int cur = (int)(kt & 1);
    if (kt + 1 < nkt) gload(kbeg + (kt + 1) * BK);  // in flight during the MFMAs below
    STAMP(1);  // global load issue
    const float* la = lds + cur * 2 * TILE_FLOATS;
    const float* lb = la + TILE_FLOATS;
    // fragments are prefetched ONE QUARTER (16 MFMAs = 1024 cycles) ahead of their use, so the
    // LDS latency is always covered by a full MFMA group instead of two instructions
    float fa[2][2][4], fb[2][2][4];
    auto fragq = [&](int set, int c) {
      if (A_KC) fragq_kc(fa[set], la, wm, lane, c); else fragq_rc(fa[set], la, wm, lane, c);
      if (B_KC) fragq_kc(fb[set], lb, wn, lane, c); else fragq_rc(fb[set], lb, wn, lane, c);
    };
    fragq(0, 0);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int set = c & 1;
      if (c < 3) fragq(set ^ 1, c + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][e], fb[set][j][e], acc[i][j],
                                                             0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    STAMP(2);  // frag reads + 64 MFMAs
#ifdef GCT_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(3);  // wait for the prefetched tile
#endif
    if (kt + 1 < nkt) lstore(cur ^ 1);
    STAMP(4);  // LDS stores
    __syncthreads();
    STAMP(5);  // barrier
  }

  // ---- epilogue: acc[i][j][r] -> C[row][col], col = lane&31, row = (r&3)+8*(r>>2)+4*(lane>>5)
  const int h = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t col = n0 + wn + j * 32 + (lane & 31);
      if (col >= g.N) continue;
      int64_t cloc;
      float* cbase;
      float bias = 0.f;
      if (g.epi == EPI_SLAB) {
        cbase = g.c0 + (int64_t)z * g.slab_stride;
        cloc = col;
      } else {
        const bool g1 = col >= g.c_nper, g2 = col >= 2 * g.c_nper;
        cloc = col - (g2 ? 2 * g.c_nper : (g1 ? g.c_nper : 0));
        cbase = g.c0 + (g2 ? g.c_d2 : (g1 ? g.c_d1 : 0));
        if (g.epi < EPI_D0 && g.bias0)
          bias = g.bias0[(g2 ? g.bias_d2 : (g1 ? g.bias_d1 : 0)) + cloc];
      }
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const int64_t row_base = m0 + wm + i * 32 + 8 * q4 + 4 * h;  // multiple of 4
        uint4 bits = make_uint4(~0u, ~0u, ~0u, ~0u);
        const bool need_rng = g.thr != 0u && (g.epi == GCT_EPI_GELU_DROP ||
                                              g.epi == GCT_EPI_GELU_DROP_SAVE ||
                                              g.epi == GCT_EPI_DROP_RESID ||
                                              g.epi == EPI_D0 + GCT_DEPI_GELU_BWD);
        if (need_rng) bits = gct_drop_bits(g.rng, drop_quad(g, row_base), (uint32_t)col);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int64_t row = row_base + e;
          if (row >= g.M) continue;
          float v = acc[i][j][q4 * 4 + e];
          const int64_t off = row * g.ldc + cloc;
          const bool keep = gct_drop_keep(bits, e, (uint32_t)col, g.thr);
          switch (g.epi) {
            case GCT_EPI_BIAS:
              v += bias;
              break;
            case GCT_EPI_GELU_DROP: {
              v += bias;
              g.pre[off] = v;
              v = gct_gelu(v);
              v = keep ? v * g.keep_scale : 0.f;
            } break;
            case GCT_EPI_GELU_DROP_SAVE: {
              float gd;
              const float y = gct_gelu_with_grad(v + bias, gd);
              g.pre[off] = keep ? gd : 0.f;
              v = keep ? y * g.keep_scale : 0.f;
            } break;
            case GCT_EPI_DROP_RESID: {
              v += bias;
              v = keep ? v * g.keep_scale : 0.f;
              v += g.resid[off];
            } break;
            case EPI_D0 + GCT_DEPI_ACCUM:
              v += cbase[off];
              break;
            case EPI_D0 + GCT_DEPI_GELU_BWD: {
              float u = 0.f;
              if (g.pre_rows > 0) {
                const int64_t er0 = pre_row0(g, row_base);
                if (er0 >= 0 && er0 + e < g.pre_rows) u = g.pre_in[(er0 + e) * g.ldc + cloc];
              } else {
                u = g.pre_in[off];
              }
              v = keep ? v * gct_gelu_grad(u) * g.keep_scale : 0.f;
            } break;
            case EPI_D0 + GCT_DEPI_MUL_SAVED: {
              float d = 0.f;
              if (g.pre_rows > 0) {
                const int64_t er0 = pre_row0(g, row_base);
                if (er0 >= 0 && er0 + e < g.pre_rows) d = g.pre_in[(er0 + e) * g.ldc + cloc];
              } else {
                d = g.pre_in[off];
              }
              v = d == 0.f ? 0.f : v * d * g.keep_scale;
            } break;
            default:
              break;  // STORE / SLAB
          }
          cbase[off] = v;
        }
      }
    }
  }
#ifdef GCT_STAMPS
  STAMP(6);  // epilogue
  if (g.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 64) {
    for (int i = 0; i < 8; ++i) g.stamps[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + i] = seg[i];
  }
#endif
}


// =====================================================================================
// FAST PATH kernel: same tiling/pipeline as gemm_f32_kernel, for the shapes that matter
// (K % 32 == 0, 16-B aligned operands, segment boundaries aligned to the tile) with the two
// costs the s_memtime stamps exposed removed:
//   * tile loads: a wave-uniform 64-bit base (SGPRs, advanced per K-tile) + per-thread 32-bit
//     offsets computed ONCE; edge rows/columns are clamped to valid memory instead of being
//     predicated (they only feed accumulator rows/columns that are never stored) -- the loop
//     issues 8 global_load_dwordx4 back to back with no address arithmetic or branches;
//   * epilogue: each wave transposes its 64x64 accumulator block through LDS and every lane
//     finishes a 4-row x 4-column patch: float4 bias/resid/pre accesses, one Philox call per
//     column (4 rows each), float4 stores of 256 contiguous bytes per 16 lanes (was: 64 scalar
//     stores per lane behind a per-element switch, 42k cycles per tile).
// =====================================================================================
// epilogue stores: 16 B per lane, non-temporal -- the outputs (84-336 MB) are far larger than the L2
// and are not re-read by this kernel, so they should not evict the operand panels (A/B: +3-7 % on the
// K = 512 shapes, +1 % on the step, against ordinary stores)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void epi_store4(float* p, const float (&x)[4]) {
#ifdef GCT_LAB_NO_EPI_STORE   // tools/gemm_lab.hip: arithmetic kept alive, (almost) nothing stored
  if (x[0] != 123456.789f) return;
#endif
  __builtin_nontemporal_store(f32x4_t{x[0], x[1], x[2], x[3]}, reinterpret_cast<f32x4_t*>(p));
}

// SIDE: the epilogues a kernel can be launched with -- 0 any, 1 forward (GCT_EPI_*), 2 dgrad (GCT_DEPI_*), 3 none
// (slabs only); the others are compiled out of it
template <int SIDE>
struct FastEpiT {
  static constexpr bool FWD = SIDE == 0 || SIDE == 1, BWD = SIDE == 0 || SIDE == 2;
  const GemmArgs& g;
  // number of extra float4 reads per patch row this epilogue needs (resid / accumulate / pre_in)
  __device__ __forceinline__ bool needs_extra() const {
#ifdef GCT_LAB_NO_EPI_MATH
    return false;
#endif
    return (FWD && g.epi == GCT_EPI_DROP_RESID) || (BWD && g.epi == EPI_D0 + GCT_DEPI_ACCUM) || reads_pre();
  }
  // the dgrad epilogues that read pre_in (the forward's row space when pre_rows > 0)
  __device__ __forceinline__ bool reads_pre() const {
    return BWD && (g.epi == EPI_D0 + GCT_DEPI_GELU_BWD || g.epi == EPI_D0 + GCT_DEPI_MUL_SAVED);
  }
  __device__ __forceinline__ const float* extra_base(const float* cbase) const {
    return (FWD && g.epi == GCT_EPI_DROP_RESID) ? g.resid : (reads_pre() ? g.pre_in : cbase);
  }
  // issue the extra reads of one 4x4 patch (latency overlaps the other patches' work)
  __device__ __forceinline__ void prefetch(float4 (&x)[4], int64_t row0, const float* cbase,
                                           int64_t cloc) const {
    const float* eb = extra_base(cbase);
    int64_t er0 = row0, elim = g.M;
    if (reads_pre() && g.pre_rows > 0) {
      er0 = pre_row0(g, row0);
      elim = er0 < 0 ? -1 : g.pre_rows;
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      x[rr] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + rr < g.M && er0 + rr < elim) x[rr] = *reinterpret_cast<const float4*>(eb + (er0 + rr) * g.ldc + cloc);
    }
  }
  __device__ __forceinline__ void apply(float4 (&v)[4], int64_t row0, int64_t col0,
                                        float* cbase, int64_t cloc, float4 bias) const {
    float4 x[4];
    if (needs_extra()) prefetch(x, row0, cbase, cloc);
    apply(v, x, row0, col0, cbase, cloc, bias);
  }
  __device__ __forceinline__ void apply(float4 (&v)[4], const float4 (&ex)[4], int64_t row0,
                                        int64_t col0, float* cbase, int64_t cloc, float4 bias) const {
    // v[rr] = 4 consecutive columns (col0..col0+3) of row row0+rr; row0 % 4 == 0
#ifdef GCT_LAB_NO_EPI_MATH    // tools/gemm_lab.hip: raw accumulators
    const int epi = EPI_D0 + GCT_DEPI_STORE;
#else
    const int epi = g.epi;
#endif
    uint4 bits[2];   // one Philox call per 4 rows x 2 columns (col0 % 4 == 0)
    const bool rng = g.thr != 0u && ((FWD && (epi == GCT_EPI_GELU_DROP || epi == GCT_EPI_GELU_DROP_SAVE ||
                                              epi == GCT_EPI_DROP_RESID)) ||
                                     (BWD && epi == EPI_D0 + GCT_DEPI_GELU_BWD));
    if (rng) {
#pragma unroll
      for (int cp = 0; cp < 2; ++cp)
        bits[cp] = gct_drop_bits(g.rng, drop_quad(g, row0), (uint32_t)(col0 + 2 * cp));
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int64_t row = row0 + rr;
      if (row >= g.M) break;
      const int64_t off = row * g.ldc + cloc;
      float x[4] = {v[rr].x, v[rr].y, v[rr].z, v[rr].w};
      const float bs[4] = {bias.x, bias.y, bias.z, bias.w};
      bool keep[4] = {true, true, true, true};
      if (rng) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) keep[cc] = gct_drop_keep(bits[cc >> 1], rr, (uint32_t)cc, g.thr);
      }
      if (FWD && epi == GCT_EPI_BIAS) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) x[cc] += bs[cc];
      } else if (FWD && epi == GCT_EPI_GELU_DROP) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) x[cc] += bs[cc];
        epi_store4(g.pre + off, x);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) x[cc] = keep[cc] ? gct_gelu(x[cc]) * g.keep_scale : 0.f;
      } else if (FWD && epi == GCT_EPI_GELU_DROP_SAVE) {
        // the saved factor is the backward's whole elementwise work: gelu'(v) where the element is kept, 0 where it
        // is dropped (one erf serves both)
        float d[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          float gd;
          const float y = gct_gelu_with_grad(x[cc] + bs[cc], gd);
          d[cc] = keep[cc] ? gd : 0.f;
          x[cc] = keep[cc] ? y * g.keep_scale : 0.f;
        }
        epi_store4(g.pre + off, d);
      } else if (FWD && epi == GCT_EPI_DROP_RESID) {
        const float4 r = ex[rr];
        const float rs[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          x[cc] = (keep[cc] ? (x[cc] + bs[cc]) * g.keep_scale : 0.f) + rs[cc];
      } else if (BWD && epi == EPI_D0 + GCT_DEPI_ACCUM) {
        const float4 r = ex[rr];
        x[0] += r.x; x[1] += r.y; x[2] += r.z; x[3] += r.w;
      } else if (BWD && epi == EPI_D0 + GCT_DEPI_GELU_BWD) {
        const float4 u = ex[rr];
        const float us[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          x[cc] = keep[cc] ? x[cc] * gct_gelu_grad(us[cc]) * g.keep_scale : 0.f;
      } else if (BWD && epi == EPI_D0 + GCT_DEPI_MUL_SAVED) {
        const float4 u = ex[rr];
        const float ds[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) x[cc] = ds[cc] == 0.f ? 0.f : x[cc] * ds[cc] * g.keep_scale;
      }
      epi_store4(cbase + off, x);
    }
  }
};
using FastEpi = FastEpiT<0>;


// Per-wave epilogue shared by the 128x128 fp32-MFMA kernel and the bf16x6 kernels (both leave a
// 64x64 block per wave in the 32x32 MFMA accumulator layout): transpose through LDS (stg: 64x64
// floats private to the wave), then every lane finishes 4 patches of 4 rows x 4 columns.
template <int SIDE>
__device__ __forceinline__ void wave_epilogue_tail(const GemmArgs& g, float* stg, int lane, int64_t mw,
                                                   int64_t nw, unsigned z);
template <int SIDE>
__device__ __forceinline__ void wave_epilogue(const GemmArgs& g, const f32x16 (&acc)[2][2], float* stg,
                                              int lane, int64_t mw, int64_t nw, unsigned z) {
  {
    const int h = lane >> 5, c32 = lane & 31;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          stg[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 64 + j * 32 + c32] = acc[i][j][r];
  }
  wave_epilogue_tail<SIDE>(g, stg, lane, mw, nw, z);
}

// What the four patches of a lane share (its 4-column chunk): destination, segment select and bias.  Depends only on
// the wave's block origin and the lane, so a kernel may resolve it before its main loop.
struct EpiLane {
  bool live;        // col0 < N
  int64_t col0, cloc;
  float* cbase;
  float4 bias;
};
__device__ __forceinline__ EpiLane epi_lane(const GemmArgs& g, int lane, int64_t nw, unsigned z) {
  EpiLane el;
  el.col0 = nw + (lane & 15) * 4;
  el.live = el.col0 < g.N;
  el.cloc = 0;
  el.cbase = g.c0;
  el.bias = make_float4(0.f, 0.f, 0.f, 0.f);
  if (el.live) {
    if (g.epi == EPI_SLAB) {
      el.cbase = g.c0 + (int64_t)z * g.slab_stride;
      el.cloc = el.col0;
    } else {
      const bool g1 = el.col0 >= g.c_nper, g2 = el.col0 >= 2 * g.c_nper;
      el.cloc = el.col0 - (g2 ? 2 * g.c_nper : (g1 ? g.c_nper : 0));
      el.cbase = g.c0 + (g2 ? g.c_d2 : (g1 ? g.c_d1 : 0));
      if (g.epi < EPI_D0 && g.bias0)
        el.bias = *reinterpret_cast<const float4*>(g.bias0 + (g2 ? g.bias_d2 : (g1 ? g.bias_d1 : 0)) + el.cloc);
    }
  }
  return el;
}

// Branch-free request of the extra epilogue operands (needs_extra()) of a lane's four patches, for issue between the
// MFMAs of a kernel's last K-tile: p[it] is row 0 of patch it's operand rows, `have` bit it says that all four rows
// exist (inside M, and -- through a quad map -- inside pre_rows and not padding).  The other patches (the ragged last
// rows of a matrix, padding quads, lanes past N) point at rows 0..3 of the operand, which always exist (epi_ahead_ok
// asks for that); what is read there is dropped and wave_epilogue_finish loads those patches the ordinary way.
struct EpiAhead {
  const float* p[4];
  unsigned have;
};
template <int SIDE>
__device__ __forceinline__ bool epi_ahead_ok(const GemmArgs& g) {
  const FastEpiT<SIDE> ep{g};
  return ep.needs_extra() && g.M >= 4 && !(ep.reads_pre() && g.pre_rows > 0 && g.pre_rows < 4);
}
// quad-map entries of the lane's four patches (pre_rows > 0: pre_in is read through the map), fetched before the main
// loop so that the plan below does not wait for them; -1: padding, or no such patch
template <int SIDE>
__device__ __forceinline__ void epi_ahead_quads(const GemmArgs& g, int lane, int64_t mw, int64_t nw, int (&qv)[4]) {
  const FastEpiT<SIDE> ep{g};
  const bool mapped = ep.reads_pre() && g.pre_rows > 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t row0 = mw + (it * 4 + (lane >> 4)) * 4;
    qv[it] = (int)(row0 >> 2);
    if (mapped && g.quad_map) qv[it] = (nw + (lane & 15) * 4 < g.N && row0 + 3 < g.M) ? g.quad_map[(row0 + g.row_base) >> 2] : -1;
  }
}
template <int SIDE>
__device__ __forceinline__ EpiAhead epi_ahead_plan(const GemmArgs& g, const EpiLane& el, int lane, int64_t mw,
                                                   const int (&qv)[4]) {
  const FastEpiT<SIDE> ep{g};
  const float* eb = ep.extra_base(el.cbase) + el.cloc;
  const bool mapped = ep.reads_pre() && g.pre_rows > 0;
  const int64_t elim = mapped ? g.pre_rows : g.M;
  EpiAhead ah;
  ah.have = 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int64_t row0 = mw + (it * 4 + (lane >> 4)) * 4;
    const int64_t er0 = mapped ? (int64_t)qv[it] * 4 : row0;        // as pre_row0()
    const bool ok = el.live && row0 + 3 < g.M && er0 >= 0 && er0 + 3 < elim;
    ah.p[it] = eb + (ok ? er0 * g.ldc : 0);
    ah.have |= ok ? 1u << it : 0u;
  }
  return ah;
}
template <int IT0, int IT1>   // patches IT0 .. IT1 - 1
__device__ __forceinline__ void epi_ahead_issue(const GemmArgs& g, const EpiAhead& ah, float4 (&ex)[4][4]) {
#pragma unroll
  for (int it = IT0; it < IT1; ++it)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) ex[it][rr] = *reinterpret_cast<const float4*>(ah.p[it] + rr * g.ldc);
}

// second part of the per-wave epilogue: the 64x64 block is in `stg` (row-major, this wave's own LDS writes); ex[it]
// already holds the extra operands of the patches whose bit is set in `have`
template <int SIDE>
__device__ __forceinline__ void wave_epilogue_finish(const GemmArgs& g, float* stg, int lane, int64_t mw,
                                                     const EpiLane& el, float4 (&ex)[4][4], unsigned have) {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's own LDS writes are visible to it
  __builtin_amdgcn_wave_barrier();
  const FastEpiT<SIDE> ep{g};
  // the lane's column chunk is the same for its 4 patches: destination, bias and the
  // segment select are resolved once; the residual / accumulate / pre-activation rows of
  // all 4 patches are requested up front so their latency overlaps
  const int c4 = lane & 15;
  if (el.live) {
    if (ep.needs_extra()) {
#pragma unroll
      for (int it = 0; it < 4; ++it)
        if (!((have >> it) & 1u)) ep.prefetch(ex[it], mw + (it * 4 + (lane >> 4)) * 4, el.cbase, el.cloc);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int rg = it * 4 + (lane >> 4);
      const int64_t row0 = mw + rg * 4;
      if (row0 >= g.M) continue;
      float4 v[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        v[rr] = *reinterpret_cast<const float4*>(stg + (rg * 4 + rr) * 64 + c4 * 4);
      ep.apply(v, ex[it], row0, el.col0, el.cbase, el.cloc, el.bias);
    }
  }
}
// ... for the kernels that request nothing ahead
template <int SIDE>
__device__ __forceinline__ void wave_epilogue_tail(const GemmArgs& g, float* stg, int lane, int64_t mw,
                                                   int64_t nw, unsigned z) {
  float4 ex[4][4];
  wave_epilogue_finish<SIDE>(g, stg, lane, mw, epi_lane(g, lane, nw, z), ex, 0u);
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void
gemm_f32_fast_kernel(const GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[4 * TILE_FLOATS];  // A0 B0 A1 B1 : 64 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

  const unsigned tiles_n = (unsigned)((g.N + BN - 1) / BN);
  const unsigned tiles_m = (unsigned)((g.M + BM - 1) / BM);
  const unsigned per_split = tiles_m * tiles_n;
  const unsigned lid = gct_xcd_remap(blockIdx.x, gridDim.x);
  const unsigned z = lid / per_split, rest = lid - z * per_split;
  const int64_t m0 = (int64_t)(rest / tiles_n) * BM, n0 = (int64_t)(rest % tiles_n) * BN;
  const int64_t kbeg = (int64_t)z * g.ksplit;
  const int64_t kend = (kbeg + g.ksplit < g.K) ? kbeg + g.ksplit : g.K;

  // ---- per-thread invariant 32-bit offsets (floats), edges clamped into valid memory
  uint32_t offa[4], offb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (A_KC) {
      int64_t r = (tid >> 3) + 32 * i;
      if (m0 + r > g.M - 1) r = g.M - 1 - m0;
      offa[i] = (uint32_t)(r * g.lda + (tid & 7) * 4);
    } else {
      int64_t c = (tid & 31) * 4;
      if (m0 + c > g.M - 4) c = g.M - 4 - m0;
      offa[i] = (uint32_t)(((tid >> 5) + 8 * i) * g.lda + c);
    }
    if (B_KC) {
      int64_t r = (tid >> 3) + 32 * i;
      if (n0 + r > g.N - 1) r = g.N - 1 - n0;
      offb[i] = (uint32_t)(r * g.ldb + (tid & 7) * 4);
    } else {
      int64_t c = (tid & 31) * 4;
      if (n0 + c > g.N - 4) c = g.N - 4 - n0;
      offb[i] = (uint32_t)(((tid >> 5) + 8 * i) * g.ldb + c);
    }
  }
  // ---- wave-uniform tile bases; a K-tile (resp. the row/column tile) lies in ONE segment
  auto useg = [](const Seg3& s, int64_t idx, int64_t nper, int64_t& local) -> const float* {
    const bool g1 = idx >= nper, g2 = idx >= 2 * nper;
    local = idx - (g2 ? 2 * nper : (g1 ? nper : 0));
    return s.p0 + (g2 ? s.d2 : (g1 ? s.d1 : 0));
  };
  int64_t aloc_m, bloc_n;
  const float* a_mbase = nullptr;
  const float* b_nbase = nullptr;
  if (!A_KC) a_mbase = useg(g.a, m0, g.a_nper, aloc_m) + aloc_m;                     // + k*lda
  if (B_KC) b_nbase = useg(g.b, n0, g.b_nper, bloc_n) + bloc_n * g.ldb;             // + k
  auto abase = [&](int64_t k0) -> const float* {
    if (A_KC) {
      int64_t loc;
      const float* p = useg(g.a, k0, g.a_nper, loc);
      return p + m0 * g.lda + loc;
    }
    return a_mbase + k0 * g.lda;
  };
  auto bbase = [&](int64_t k0) -> const float* {
    if (B_KC) return b_nbase + k0;
    int64_t loc;
    const float* p = useg(g.b, k0, g.b_nper, loc);
    return p + loc * g.ldb + n0;
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[4], rb[4];
#define GCT_GLOAD(k0_)                                                                     \
  do {                                                                                     \
    const float* ab__ = abase(k0_);                                                        \
    const float* bb__ = bbase(k0_);                                                        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                          \
        ra[i] = *reinterpret_cast<const float4*>(ab__ + offa[i]);                          \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                          \
        rb[i] = *reinterpret_cast<const float4*>(bb__ + offb[i]);                          \
  } while (0)
#define GCT_LSTORE(buf_)                                                                   \
  do {                                                                                     \
    float* la__ = lds + (buf_) * 2 * TILE_FLOATS;                                          \
    float* lb__ = la__ + TILE_FLOATS;                                                      \
    if (A_KC) store_kc(la__, ra, tid); else store_rc(la__, ra, tid);                       \
    if (B_KC) store_kc(lb__, rb, tid); else store_rc(lb__, rb, tid);                       \
  } while (0)
// the prefetched tile must stay in VGPRs until the MFMA block is done: an opaque use right
// before the LDS stores stops hipcc from sinking the stores (and their vmcnt waits, and
// scratch spills) to just behind the loads
#define GCT_PIN(v_) asm volatile("" : "+v"(v_.x), "+v"(v_.y), "+v"(v_.z), "+v"(v_.w))

  const int64_t nkt = (kend - kbeg) / BK;
#ifdef GCT_STAMPS
  unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tprev)::"memory");
#endif
  // wgrad only: db[n] = sum_m dY[m][n] falls out of the A tiles already in registers.  Weights
  // (0/1) instead of branches keep the loop a single basic block; only the tile_n == 0 column of
  // workgroups contributes, and the duplicated final prefetch is masked out.
  float4 bsum = make_float4(0.f, 0.f, 0.f, 0.f);
  const float bw0 = (!A_KC && !B_KC && g.bias_slab && n0 == 0) ? 1.f : 0.f;
#define GCT_BSUM(w_)                                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                           \
    bsum.x = fmaf(w_, ra[i].x, bsum.x); bsum.y = fmaf(w_, ra[i].y, bsum.y);                 \
    bsum.z = fmaf(w_, ra[i].z, bsum.z); bsum.w = fmaf(w_, ra[i].w, bsum.w);                 \
  }
  if (nkt > 0) {
    GCT_GLOAD(kbeg);
    if (!A_KC && !B_KC) { GCT_BSUM(bw0) }
    GCT_LSTORE(0);
  }
  __syncthreads();
  STAMP(0);
  // The loop body is ONE basic block (no branches: the last iteration re-loads the final tile
  // and stores it to the idle LDS buffer, which nobody reads) so that the scheduler can
  // interleave memory instructions with the MFMA stream:
  //   quarter 0: the 8 global loads of tile t+1 trickle out, one per two MFMAs (issued as a
  //              burst right after the barrier the 4 waves block ~750 cycles on the CU's
  //              vector-memory issue path -- s_memtime stamps, tools/gemm_stamps.hip);
  //   quarter 3: the 8 ds_write_b128 of tile t+1 (other LDS buffer), one per two MFMAs.
  // Exposed per K-tile: the barrier and the first fragment read.
  float fa[2][2][4], fb[2][2][4];
#define GCT_FRAGQ(set_, c_, la_, lb_)                                                        \
  do {                                                                                       \
    if (A_KC) fragq_kc(fa[set_], la_, wm, lane, c_); else fragq_rc(fa[set_], la_, wm, lane, c_); \
    if (B_KC) fragq_kc(fb[set_], lb_, wn, lane, c_); else fragq_rc(fb[set_], lb_, wn, lane, c_); \
  } while (0)
#define GCT_MFMA16(set_)                                                                     \
  _Pragma("unroll") for (int e = 0; e < 4; ++e)                                              \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                              \
  _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set_][i][e], fb[set_][j][e], acc[i][j], 0, 0, 0)
  if (nkt > 0) GCT_FRAGQ(0, 0, lds, lds + TILE_FLOATS);
  for (int64_t kt = 0; kt < nkt; ++kt) {
    const int cur = (int)(kt & 1);
    const float* la = lds + cur * 2 * TILE_FLOATS;
    const float* lb = la + TILE_FLOATS;
    const int64_t knext = (kt + 1 < nkt) ? kbeg + (kt + 1) * BK : kbeg + kt * BK;
    __builtin_amdgcn_sched_barrier(0);
    // ---- quarter 0
    GCT_FRAGQ(1, 1, la, lb);
    GCT_GLOAD(knext);
    GCT_MFMA16(0);
    __builtin_amdgcn_sched_group_barrier(0x100, 16, 0);  // fragment reads first
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMA
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // 1 global load
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(1);
    // ---- quarter 1, 2
    GCT_FRAGQ(0, 2, la, lb);
    __builtin_amdgcn_sched_barrier(0);
    GCT_MFMA16(1);
    __builtin_amdgcn_sched_barrier(0);
    GCT_FRAGQ(1, 3, la, lb);
    __builtin_amdgcn_sched_barrier(0);
    GCT_MFMA16(0);
    __builtin_amdgcn_sched_barrier(0);
    STAMP(2);
    // ---- quarter 3 + LDS stores of the next tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      GCT_PIN(ra[i]);
      GCT_PIN(rb[i]);
    }
    if (!A_KC && !B_KC) {
      const float bw = (kt + 1 < nkt) ? bw0 : 0.f;
      GCT_BSUM(bw)
    }
    GCT_LSTORE(cur ^ 1);
    GCT_MFMA16(1);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // 2 MFMA
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // 1 LDS store
    }
    __builtin_amdgcn_sched_barrier(0);
    STAMP(3);
    __syncthreads();
    STAMP(4);
    GCT_FRAGQ(0, 0, lds + (cur ^ 1) * 2 * TILE_FLOATS, lds + (cur ^ 1) * 2 * TILE_FLOATS + TILE_FLOATS);
  }
  __syncthreads();  // the speculative fragment read above must finish before LDS is reused
#undef GCT_FRAGQ
#undef GCT_MFMA16
#undef GCT_BSUM
  if (!A_KC && !B_KC) {
    if (g.bias_slab && n0 == 0) {            // block-uniform: combine the 8 row groups, fixed order
      float4* red = reinterpret_cast<float4*>(lds);
      red[tid] = bsum;
      __syncthreads();
      if (tid < 32) {
        float4 t4 = red[tid];
        for (int r = 1; r < 8; ++r) {
          const float4 u = red[r * 32 + tid];
          t4.x += u.x; t4.y += u.y; t4.z += u.z; t4.w += u.w;
        }
        const int64_t col = m0 + tid * 4;
        if (col + 3 < g.M) *reinterpret_cast<float4*>(g.bias_slab + (int64_t)z * g.M + col) = t4;
      }
      __syncthreads();
    }
  }
#undef GCT_GLOAD
#undef GCT_LSTORE
#undef GCT_PIN

  // ---- epilogue: per-wave 64x64 transpose through LDS (the tile buffers are free now)
  wave_epilogue<A_KC && B_KC ? 1 : (A_KC ? 2 : 3)>(g, acc, lds + wave * 4096, lane, m0 + wm, n0 + wn, z);
#ifdef GCT_STAMPS
  STAMP(6);  // epilogue
  if (g.stamps && (threadIdx.x & 63) == 0 && blockIdx.x < 64) {
    for (int i = 0; i < 8; ++i) g.stamps[((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + i] = seg[i];
  }
#endif
}


int64_t g_x6_kernel_launches = 0;   // gemm_x6_kernel / gemm_x6s_kernel launches, 3 pieces (a tail-balanced call makes two)
int64_t g_x3_kernel_launches = 0;   // the same kernels with 2 pieces (bf16x3 mode)
#include "gemm_x6.inc"

// =====================================================================================
// SKINNY-M forward kernel (KV-cached decode: M = batch rows per step = 512): 64x64 tiles, 4 waves
// of one 32x32 MFMA tile each, 32 KB LDS => 4-5 workgroups per CU and 4x as many tiles as the
// 128x128 kernel, which fills only 16-64 of the 256 CUs at M = 512.  Same operand layout
// (x [M][K], w [N][K]), same epilogue (FastEpi), simple two-buffer pipeline.
// =====================================================================================
__global__ __launch_bounds__(256) void gemm_f32_small_kernel(const GemmArgs g) {
  constexpr int SB = 64, STILE = SB * BK;  // 2048 floats per operand tile
  __shared__ __attribute__((aligned(16))) float lds[4 * STILE];  // A0 B0 A1 B1 : 32 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const unsigned tiles_n = (unsigned)((g.N + SB - 1) / SB);
  const unsigned tiles_m = (unsigned)((g.M + SB - 1) / SB);
  const unsigned lid0 = gct_xcd_remap(blockIdx.x, gridDim.x);
  const unsigned z = lid0 / (tiles_m * tiles_n), lid = lid0 - z * (tiles_m * tiles_n);
  const int64_t m0 = (int64_t)(lid / tiles_n) * SB, n0 = (int64_t)(lid % tiles_n) * SB;
  const int64_t kbeg = (int64_t)z * g.ksplit;
  const int64_t kend = (kbeg + g.ksplit < g.K) ? kbeg + g.ksplit : g.K;

  uint32_t offa[2], offb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int64_t r = (tid >> 3) + 32 * i;
    int64_t ra_ = r, rb_ = r;
    if (m0 + ra_ > g.M - 1) ra_ = g.M - 1 - m0;
    if (n0 + rb_ > g.N - 1) rb_ = g.N - 1 - n0;
    offa[i] = (uint32_t)(ra_ * g.lda + (tid & 7) * 4);
    offb[i] = (uint32_t)(rb_ * g.ldb + (tid & 7) * 4);
  }
  const bool g1 = n0 >= g.b_nper, g2 = n0 >= 2 * g.b_nper;   // the 64-row weight tile lies in one segment
  const float* bbase0 = g.b.p0 + (g2 ? g.b.d2 : (g1 ? g.b.d1 : 0)) +
                        (n0 - (g2 ? 2 * g.b_nper : (g1 ? g.b_nper : 0))) * g.ldb;
  const float* abase0 = g.a.p0 + m0 * g.lda;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float4 ra[2], rb[2];
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ra[i] = *reinterpret_cast<const float4*>(abase0 + k0 + offa[i]);
      rb[i] = *reinterpret_cast<const float4*>(bbase0 + k0 + offb[i]);
    }
  };
  auto lstore = [&](int buf) {
    float* la = lds + buf * 2 * STILE;
    float* lb = la + STILE;
    const int c8 = tid & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (tid >> 3) + 32 * i;
      const int chunk = c8 ^ ((row >> 1) & 7);
      *reinterpret_cast<float4*>(la + row * BK + chunk * 4) = ra[i];
      *reinterpret_cast<float4*>(lb + row * BK + chunk * 4) = rb[i];
    }
  };
  const int64_t nkt = (kend - kbeg) / BK;
  gload(kbeg);
  lstore(0);
  __syncthreads();
  const int h = lane >> 5;
  for (int64_t kt = 0; kt < nkt; ++kt) {
    const int cur = (int)(kt & 1);
    if (kt + 1 < nkt) gload(kbeg + (kt + 1) * BK);
    const float* la = lds + cur * 2 * STILE;
    const float* lb = la + STILE;
    const int rowa = wm + (lane & 31), rowb = wn + (lane & 31);
    const int swa = (rowa >> 1) & 7, swb = (rowb >> 1) & 7;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 a4 = *reinterpret_cast<const float4*>(la + rowa * BK + (((h * 4 + c) ^ swa) * 4));
      const float4 b4 = *reinterpret_cast<const float4*>(lb + rowb * BK + (((h * 4 + c) ^ swb) * 4));
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
    }
    if (kt + 1 < nkt) lstore(cur ^ 1);
    __syncthreads();
  }
  // epilogue: per-wave 32x32 transpose through LDS, 4x4 patch per lane
  float* stg = lds + wave * 1024;
  {
    const int c32 = lane & 31;
#pragma unroll
    for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * h) * 32 + c32] = acc[r];
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  const FastEpi ep{g};
  const int rg = lane >> 3, c4 = lane & 7;           // 8 row groups x 8 column chunks
  const int64_t row0 = m0 + wm + rg * 4, col0 = n0 + wn + c4 * 4;
  if (row0 < g.M && col0 < g.N) {
    float4 v[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) v[rr] = *reinterpret_cast<const float4*>(stg + (rg * 4 + rr) * 32 + c4 * 4);
    if (g.epi == EPI_SLAB) {                 // split-K partial: raw sums, dense [M][N] slab z
      float* sl = g.c0 + (int64_t)z * g.slab_stride;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        if (row0 + rr < g.M) *reinterpret_cast<float4*>(sl + (row0 + rr) * g.N + col0) = v[rr];
      return;
    }
    const bool q1 = col0 >= g.c_nper, q2 = col0 >= 2 * g.c_nper;
    const int64_t cloc = col0 - (q2 ? 2 * g.c_nper : (q1 ? g.c_nper : 0));
    float* cbase = g.c0 + (q2 ? g.c_d2 : (q1 ? g.c_d1 : 0));
    float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
    if (g.bias0) bias = *reinterpret_cast<const float4*>(g.bias0 + (q2 ? g.bias_d2 : (q1 ? g.bias_d1 : 0)) + cloc);
    ep.apply(v, row0, col0, cbase, cloc, bias);
  }
}


// =====================================================================================
// PANEL kernel for the smallest skinny problems (a 512-row decode step: M x N / (32 x TN) <= ~512 tiles): one
// workgroup per 32 x TN output tile runs the WHOLE reduction -- no split-K slabs, no fix-up launch -- on K chunks of
// 256: the chunk's operand panels (A 32 x 256, B TN x 256 fp32) are requested in one burst (8 + TN/4 float4 per
// thread in flight), written to LDS once and multiplied from there (v_mfma_f32_16x16x4_f32, four waves = 2 x 2 or
// 2 x 4 sub-tiles); the next chunk's burst is in flight during the MFMAs.  A step of the KV-cached decode is ~37
// dependent GEMMs, each far too small to fill the chip: what counts is the latency of one launch (was: 64 x 64
// tiles with K split 4-12 ways, 17 us, + a 9 us fix-up launch).
// =====================================================================================
// RAGGED (TN = 32 only): N <= 32 output columns of any count and leading dimension (the vocabulary head: 28-31
// columns) -- weight rows beyond N are clamped to the last one (they feed columns that are never stored), the
// epilogue is the plain bias one with scalar guarded stores.  One column of workgroups, M / 32 of them.
template <int TN, bool RAGGED = false>
__global__ __launch_bounds__(256) void gemm_f32_panel_kernel(const GemmArgs g) {
  constexpr int TM = 32, KC = 256, SD = KC + 4, NBL = TN / 4;   // NBL float4 of the B panel per thread and chunk
  extern __shared__ __attribute__((aligned(16))) float plds[];
  float* As = plds;                    // [TM][SD]
  float* Bs = plds + TM * SD;          // [TN][SD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, c16 = lane & 15;
  const unsigned tiles_m = (unsigned)((g.M + TM - 1) / TM);
  const unsigned lid = gct_xcd_remap(blockIdx.x, gridDim.x);
  // consecutive logical ids (= one XCD) share a weight panel
  const int64_t m0 = (int64_t)(lid % tiles_m) * TM, n0 = (int64_t)(lid / tiles_m) * TN;
  const bool s1 = n0 >= g.b_nper, s2 = n0 >= 2 * g.b_nper;     // the TN weight rows lie in one segment
  const float* bbase = g.b.p0 + (s2 ? g.b.d2 : (s1 ? g.b.d1 : 0)) + (n0 - (s2 ? 2 * g.b_nper : (s1 ? g.b_nper : 0))) * g.ldb;
  const float* abase = g.a.p0;
  uint32_t offa[8], offb[NBL];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int idx = tid + 256 * i, row = idx >> 6, c4 = idx & 63;
    int64_t r = m0 + row;
    if (r > g.M - 1) r = g.M - 1;
    offa[i] = (uint32_t)(r * g.lda + c4 * 4);
  }
#pragma unroll
  for (int i = 0; i < NBL; ++i) {
    const int idx = tid + 256 * i, c4 = idx & 63;
    int64_t row = idx >> 6;
    if (RAGGED && n0 + row > g.N - 1) row = g.N - 1 - n0;
    offb[i] = (uint32_t)(row * g.ldb + c4 * 4);
  }
  f32x4_t ra[8], rb[NBL];           // native vectors: HIP's float4 struct copies kept these arrays in scratch
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ra[i] = *reinterpret_cast<const f32x4_t*>(abase + k0 + offa[i]);
#pragma unroll
    for (int i = 0; i < NBL; ++i) rb[i] = *reinterpret_cast<const f32x4_t*>(bbase + k0 + offb[i]);
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<f32x4_t*>(As + (idx >> 6) * SD + (idx & 63) * 4) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<f32x4_t*>(Bs + (idx >> 6) * SD + (idx & 63) * 4) = rb[i];
    }
  };
  constexpr int NS = TN / 32;          // 16 x 16 sub-tiles per wave (they share the A fragment)
  const int wm = (wave >> 1) * 16, wn = (wave & 1) * (TN / 2);
  f32x4_t acc[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int64_t nch = g.K / KC;
  gload(0);
  lstore();
  __syncthreads();
  for (int64_t c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload((c + 1) * KC);
    // lane group g4 owns k = 64 g4 .. 64 g4 + 63 of the chunk for BOTH operands (any k permutation is legal)
    const float* ap = As + (wm + c16) * SD + g4 * 64;
#pragma unroll 4
    for (int j = 0; j < 16; ++j) {
      const float4 a4 = *reinterpret_cast<const float4*>(ap + 4 * j);
#pragma unroll
      for (int u = 0; u < NS; ++u) {
        const float4 b4 = *reinterpret_cast<const float4*>(Bs + (wn + 16 * u + c16) * SD + g4 * 64 + 4 * j);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b4.x, acc[u], 0, 0, 0);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b4.y, acc[u], 0, 0, 0);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b4.z, acc[u], 0, 0, 0);
        acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b4.w, acc[u], 0, 0, 0);
      }
    }
    __syncthreads();                   // every wave is done with this chunk's panels
    if (c + 1 < nch) {
      lstore();
      __syncthreads();
    }
  }
  // epilogue: per-wave 16 x 16 transpose through LDS (the panels are free), one 4 x 4 patch per lane 0..15
  float* stg = plds + wave * (16 * 20);
  const FastEpi ep{g};
#pragma unroll
  for (int u = 0; u < NS; ++u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) stg[(4 * g4 + i) * 20 + c16] = acc[u][i];   // C[m = 4 g4 + i][n = c16]
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) {
      const int pr = lane >> 2, pc = lane & 3;
      const int64_t row0 = m0 + wm + 4 * pr, col0 = n0 + wn + 16 * u + 4 * pc;
      if (RAGGED) {
        for (int rr = 0; rr < 4; ++rr)
          for (int cc = 0; cc < 4; ++cc)
            if (row0 + rr < g.M && col0 + cc < g.N)
              g.c0[(row0 + rr) * g.ldc + col0 + cc] = stg[(4 * pr + rr) * 20 + 4 * pc + cc] + (g.bias0 ? g.bias0[col0 + cc] : 0.f);
      } else if (row0 < g.M && col0 < g.N) {
        float4 v[4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) v[rr] = *reinterpret_cast<const float4*>(stg + (4 * pr + rr) * 20 + 4 * pc);
        const bool q1 = col0 >= g.c_nper, q2 = col0 >= 2 * g.c_nper;
        const int64_t cloc = col0 - (q2 ? 2 * g.c_nper : (q1 ? g.c_nper : 0));
        float* cbase = g.c0 + (q2 ? g.c_d2 : (q1 ? g.c_d1 : 0));
        float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g.bias0) bias = *reinterpret_cast<const float4*>(g.bias0 + (q2 ? g.bias_d2 : (q1 ? g.bias_d1 : 0)) + cloc);
        ep.apply(v, row0, col0, cbase, cloc, bias);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
  }
}

template <int TN, bool RAGGED = false>
int launch_panel(const GemmArgs& g, hipStream_t st) {
  constexpr size_t LDS = (size_t)(32 + TN) * 260 * sizeof(float);
  static bool attr_set = false;        // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)gemm_f32_panel_kernel<TN, RAGGED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) {
      gct_set_error("gemm_f32_panel: cannot reserve %zu bytes of LDS: %s", LDS, hipGetErrorString(e));
      return GCT_ERR_HIP;
    }
    attr_set = true;
  }
  const int64_t tiles = ((g.M + 31) / 32) * (RAGGED ? 1 : g.N / TN);
  hipLaunchKernelGGL((gemm_f32_panel_kernel<TN, RAGGED>), dim3((unsigned)tiles), dim3(256), LDS, st, g);
  GCT_LAUNCH_CHECK("gemm_f32_panel");
  return GCT_OK;
}

// split-K tail of the skinny-M path: out = epilogue(sum_s slab[s] + bias ...), one 4x4 patch per
// thread, float4 everywhere, same FastEpi as the GEMM kernels.
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const GemmArgs g, const float* slabs,
                                                              int nslab, int64_t slab_stride) {
  const int64_t pc = g.N / 4, pr = (g.M + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= pc * pr) return;
  const int64_t row0 = (idx / pc) * 4, col0 = (idx % pc) * 4;
  float4 v[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    v[rr] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + rr < g.M) {
      const float* p = slabs + (row0 + rr) * g.N + col0;
      for (int s = 0; s < nslab; ++s) {
        const float4 t = *reinterpret_cast<const float4*>(p + (int64_t)s * slab_stride);
        v[rr].x += t.x; v[rr].y += t.y; v[rr].z += t.z; v[rr].w += t.w;
      }
    }
  }
  const bool q1 = col0 >= g.c_nper, q2 = col0 >= 2 * g.c_nper;
  const int64_t cloc = col0 - (q2 ? 2 * g.c_nper : (q1 ? g.c_nper : 0));
  float* cbase = g.c0 + (q2 ? g.c_d2 : (q1 ? g.c_d1 : 0));
  float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
  if (g.bias0) bias = *reinterpret_cast<const float4*>(g.bias0 + (q2 ? g.bias_d2 : (q1 ? g.bias_d1 : 0)) + cloc);
  const FastEpi ep{g};
  ep.apply(v, row0, col0, cbase, cloc, bias);
}

// GEMM arithmetic: GCT_GEMM_F32 = v_mfma_f32_32x32x2_f32 everywhere; GCT_GEMM_BF16X6 = exact 3-way bf16
// split with six partial products (gemm_x6.inc) wherever a launch qualifies; GCT_GEMM_BF16X3 (opt-in, set only
// through gct_gemm_set_mode) = the same routes and kernels with two pieces and three products.  Process-wide; the
// default comes from GCT_GEMM_MODE=f32|x6 (x6 when unset).
int g_gemm_mode = -1;
int64_t g_gemm_launches[2] = {0, 0};   // GEMM calls served by [fp32-MFMA kernels, bf16x6 kernels] (tests / diagnostics;
                                       // bf16x3 calls count in g_x3_kernel_launches only)
inline int gemm_mode() {
  if (g_gemm_mode < 0) {
    const char* e = getenv("GCT_GEMM_MODE");
    g_gemm_mode = (e && (e[0] == 'f' || e[0] == '0')) ? GCT_GEMM_F32 : GCT_GEMM_BF16X6;
  }
  return g_gemm_mode;
}

// single source of truth for "this launch takes gemm_f32_fast_kernel"
template <bool A_KC, bool B_KC>
bool fast_ok(const GemmArgs& g, bool vec) {
  auto seg_ok = [](int64_t nper, int64_t extent, int64_t gran) { return nper >= extent || nper % gran == 0; };
  return vec && g.K % BK == 0 && g.ksplit % BK == 0 && g.M >= 4 && g.N >= 4 &&
         (A_KC ? seg_ok(g.a_nper, g.K, BK) : (seg_ok(g.a_nper, g.M, BM) && g.M % 4 == 0)) &&
         (B_KC ? seg_ok(g.b_nper, g.N, BN) : (seg_ok(g.b_nper, g.K, BK) && g.N % 4 == 0)) &&
         g.N % 4 == 0 && g.ldc % 4 == 0 && gct_aligned16(g.c0) && g.c_d1 % 4 == 0 && g.c_d2 % 4 == 0 &&
         (g.c_nper >= g.N || g.c_nper % 4 == 0) && g.slab_stride % 4 == 0 &&
         (!g.bias0 || (gct_aligned16(g.bias0) && g.bias_d1 % 4 == 0 && g.bias_d2 % 4 == 0)) &&
         (!g.resid || gct_aligned16(g.resid)) && (!g.pre || gct_aligned16(g.pre)) &&
         (!g.pre_in || gct_aligned16(g.pre_in)) && 130 * g.lda < (1ll << 31) && 130 * g.ldb < (1ll << 31);
}

// ---- split rules: each slab count is computed here once, for the launch and for the workspace queries alike

// bytes of s fp32 slabs of [rows][cols]; 0 when s <= 1 (no split, no slabs)
inline int64_t slab_bytes(int64_t s, int64_t rows, int64_t cols) {
  return s > 1 ? s * rows * cols * (int64_t)sizeof(float) : 0;
}

// skinny M (decode steps): 64x64 tiles when the 128x128 grid would leave most CUs idle
// (192: with more tiles the bf16x6 kernel wins even on half the CUs -- decode at n >= 6144 lost 5-8 % with 384)
inline bool skinny_m(int64_t M, int64_t N) { return ((M + BM - 1) / BM) * ((N + BN - 1) / BN) < 192; }

// K-splits of the skinny fp32 route (gemm_f32_small_kernel; 1 = none): ~768 workgroups, >= 4 K-tiles per split
int skinny_splits(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = ((M + 63) / 64) * ((N + 63) / 64);
  if (tiles <= 0) return 1;
  int64_t ns = 768 / tiles;
  if (ns > K / BK / 4) ns = K / BK / 4;
  return ns < 1 ? 1 : (int)ns;
}

// Tail balancing for the bf16x6 forward / dgrad launches (one 128x256 workgroup per CU, 256 CUs): when the
// tile count leaves a partial last round, the rows of that round are computed as a second launch with K
// split s ways (s * rem workgroups of 1/s duration) into fp32 slabs, and a small fix-up kernel sums the slabs
// and applies the epilogue.  E.g. 640 tiles (N = 512 at 40 960 rows): 3 rounds -> 2.5; 2 592 tiles (N = 2 048
// at 41 472 rows): 11 rounds -> 10.25.  Deterministic (fixed summation order, no atomics).
// decides whether (and how) a [M][N] x K bf16x6 forward / dgrad launch is tail-split: returns the number of
// K-splits (1 = no) and the first tail row
int x6_tail_plan(int64_t M, int64_t N, int64_t K, int64_t* m1_out) {
  constexpr int64_t CUS = 256;
  const int64_t tm = (M + XBM - 1) / XBM, tn = (N + XBN - 1) / XBN, tiles = tm * tn;
  const int64_t rem = tiles % CUS;
  if (tiles <= CUS || rem == 0 || rem % tn != 0 || K % XBK != 0) return 1;
  const int64_t nkt = K / XBK;
  int best = 1;
  double cost = 1.0;                                   // duration of the last round, in rounds
  // a workgroup costs (o + K-tiles) with o ~ 3.3 K-tile times of prologue + epilogue (s_memtime stamps),
  // so a 1/s share of K costs (o + nkt / s) / (o + nkt) of a full tile, not 1/s
  const double o = 3.3;
  for (int s2 = 2; s2 <= 8 && nkt / s2 >= 2; ++s2) {
    const double c = (double)((rem * s2 + CUS - 1) / CUS) * (o + (double)nkt / s2) / (o + nkt) + 0.05;  // + fix-up pass
    if (c < cost - 1e-9) { cost = c; best = s2; }
  }
  if (best == 1 || cost > 0.75) return 1;
  *m1_out = (tiles - rem) / tn * XBM;
  return best;
}

// Few 128x256 tiles but a long reduction (FFN-2 of a 1 024 .. 8 192-row decode step: 32-64 tiles, K = 2 048): the bf16x6
// kernel with K split s ways into fp32 slabs + the fix-up kernel fills the chip where the plain launch would use a
// quarter of it and the skinny fp32 kernel would run at the fp32 pipe's rate.
// number of K-splits of that route (1 = not taken)
int x6_splitk_all_plan(int64_t M, int64_t N, int64_t K) {
  constexpr int64_t CUS = 256;
  const int64_t tiles = ((M + XBM - 1) / XBM) * ((N + XBN - 1) / XBN), nkt = K / XBK;
  // K = 1024 (the folded cross-attention output projection of a decode step) pays only from 2 048 rows on: with fewer
  // the panel kernel is faster (+7 % per step at n = 1 024, measured both ways at 1 024 ... 8 192)
  if (tiles > CUS / 2 || K % XBK != 0 || nkt < 32 || M < 1024 || (nkt < 64 && M < 2048)) return 1;
  int64_t sp = CUS / tiles;
  if (sp > nkt / 8) sp = nkt / 8;                      // >= 8 K-tiles per split
  if (sp > 8) sp = 8;
  return sp < 2 ? 1 : (int)sp;
}

// ---- route thresholds (measured; each one moves launches between kernels)

// 64 x 128 tiles of the bf16x6 small-tile kernel
inline int64_t x6s_tiles(int64_t M, int64_t N) { return ((M + SBM - 1) / SBM) * ((N + SBN - 1) / SBN); }

// few 128 x 256 tiles but enough 64 x 128 ones: the small-tile bf16x6 kernel (forward and dgrad; decode steps of
// 2 000-4 000 rows, training at small batches).  Measured (tools/kernel_bench.py --suite decgemm, rows 1 024 ... 5 184):
// a 64 x 128 tile takes 0.75 us per K-tile alone on its CU and 1.45 us when two share it, a 128 x 256 tile 2.8 us;
// from K = 2 048 on the large kernel's K-split routes fill the chip and win, at K = 1 024 only while every small tile
// has a CU to itself
inline bool x6s_shape(const GemmArgs& g) {
  const int64_t big = ((g.M + XBM - 1) / XBM) * ((g.N + XBN - 1) / XBN), small = x6s_tiles(g.M, g.N), nkt = g.K / XBK;
  return big <= 160 && small >= 96 && small <= (nkt <= 16 ? 512 : 256) && nkt <= 32;
}

// K <= 1 024 and a short tail: the tail rows of a tail-balanced bf16x6 launch on 64 x 128 tiles (gemm_x6s_kernel, up
// to two per CU) finish with their own epilogue -- no slabs, no fix-up launch (48.6 -> 48.2 ms per step with the
// forward launches alone) -- while they are at most this many tiles
constexpr int64_t X6_TAIL_SMALL_MAX = 512;

// skinny fp32 forwards: the panel kernel while it has at most this many 32 x 32 tiles; 4096: +9 % / +3 % per decode step
// at n = 1024 / 4096 over 384
constexpr int64_t PANEL32_MAX_TILES = 4096;

// ---- slab routes: K split into fp32 slabs at ws, then splitk_epilogue_kernel applies g's epilogue to their sum

// the split-K form of g: raw partial sums of `splits` K ranges (whole 32-wide K-tiles) into dense [M][N] slabs at ws
static_assert(BK == XBK, "the fp32 and bf16x6 kernels split K at the same granularity");
// K range of one slab when K is split `splits` ways, and the slabs that makes (fewer than `splits` when the ranges,
// whole K-tiles each, cover K sooner)
inline int64_t slab_krange(int64_t K, int splits) { return ((K / BK + splits - 1) / splits) * BK; }
inline int slab_count(int64_t K, int splits) {
  const int64_t ks = slab_krange(K, splits);
  return (int)((K + ks - 1) / ks);
}

GemmArgs slab_args(const GemmArgs& g, int splits, float* ws) {
  GemmArgs p = g;
  p.ksplit = slab_krange(g.K, splits);
  p.nsplit = slab_count(g.K, splits);
  p.epi = EPI_SLAB; p.c0 = ws; p.ldc = g.N; p.slab_stride = g.M * g.N;
  p.c_d1 = p.c_d2 = 0; p.c_nper = INT64_MAX / 4; p.bias0 = nullptr; p.resid = nullptr; p.pre = nullptr; p.pre_in = nullptr;
  return p;
}

// bytes of ws the slab launch p writes
inline int64_t slabs_written(const GemmArgs& p) { return (int64_t)p.nsplit * p.slab_stride * (int64_t)sizeof(float); }

int launch_fixup(const GemmArgs& g, const GemmArgs& slabs, hipStream_t st, const char* name) {
  const int64_t patches = ((g.M + 3) / 4) * (g.N / 4);
  hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((patches + 255) / 256)), dim3(256), 0, st, g,
                     (const float*)slabs.c0, slabs.nsplit, slabs.slab_stride);
  GCT_LAUNCH_CHECK(name);
  return GCT_OK;
}

// ---- what a fwd / dgrad call executed, for gct_gemm_last_route (diagnostics: a few stores per call, written where the
// kernels are launched).  Layout: out8 of gct_linear_fwd_route.
thread_local int64_t t_last_route[8] = {-1, 1, 0, 0, 1, 0, 0, 0};
inline void note_route(int kind, int splits, int launches, int64_t ws_written) {
  const int64_t r[8] = {kind, splits, 0, 0, 1, launches, ws_written, 0};
  for (int i = 0; i < 8; ++i) t_last_route[i] = r[i];
}

// the tail of a bf16 tile launch (GemmRoute::X6, forward / dgrad)
struct X6Tail {
  enum Kind { NONE = 0, SMALL_TILES = 1, SLABS = 2 } kind;
  int splits;        // SLABS: K-splits asked of slab_args (it may make fewer slabs: slab_count); 1 otherwise
  int64_t m1;        // first tail row (a multiple of 128)
};

// the tail rows [m1, M) of g as their own problem: the dropout coordinates continue through row_base
GemmArgs x6_tail_args(const GemmArgs& g, int64_t m1) {
  GemmArgs e = g;
  e.M = g.M - m1; e.row_base = g.row_base + m1;
  e.a.p0 += m1 * g.lda;                                // FWD / DGRAD: A is [M][K]
  e.c0 += m1 * g.ldc;
  if (e.resid) e.resid += m1 * g.ldc;
  if (e.pre) e.pre += m1 * g.ldc;
  // pre_in read through the quad map keeps the forward's row space: the tail finds its rows through row_base
  if (e.pre_in && !(g.pre_rows > 0 && g.quad_map)) e.pre_in += m1 * g.ldc;
  return e;
}

// Pure: whether (and how) the launch of g on the bf16 tile route is tail-balanced (x6_tail_plan): the tail rows on the
// small-tile kernel, or K-split into slabs at ws + a fix-up.  Only the capture check is left to the executor.
template <int MODE>
X6Tail plan_x6_tail(const GemmArgs& g, const float* ws, int64_t ws_bytes) {
  const X6Tail none = {X6Tail::NONE, 1, 0};
  if (MODE == X6_WGRAD || g.nsplit != 1 || !ws || !gct_aligned16(ws)) return none;
  int64_t m1 = 0;
  const int best = x6_tail_plan(g.M, g.N, g.K, &m1);
  const int64_t m2 = g.M - m1, nkt = g.K / XBK;
  if (best == 1 || slab_bytes(best, m2, g.N) > ws_bytes) return none;
  if (nkt <= 32 && x6s_tiles(m2, g.N) <= X6_TAIL_SMALL_MAX) {
    const GemmArgs e = x6_tail_args(g, m1);
    if (MODE == X6_FWD ? x6s_ok(e, true) : x6s_dgrad_ok(e, true)) return {X6Tail::SMALL_TILES, 1, m1};
  }
  return {X6Tail::SLABS, best, m1};
}

// executor of the bf16x6 route: plain, or tail-balanced as plan_x6_tail says.  A stream that is being captured gets
// the plain launch: one kernel per GEMM in a captured graph.  NP: pieces (3: bf16x6, 2: bf16x3).
template <int MODE, int NP>
int launch_x6_tail_split(const GemmArgs& g, hipStream_t st, float* ws, int64_t ws_bytes) {
  X6Tail t = plan_x6_tail<MODE>(g, ws, ws_bytes);
  if (t.kind != X6Tail::NONE) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // keep captured graphs to one kernel per GEMM
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) t.kind = X6Tail::NONE;
  }
  if (t.kind == X6Tail::NONE) return launch_x6<MODE, NP>(g, st);
  GemmArgs head = g;
  head.M = t.m1;
  int rc = launch_x6<MODE, NP>(head, st);
  if (rc) return rc;
  const GemmArgs e = x6_tail_args(g, t.m1);
  t_last_route[2] = t.kind; t_last_route[3] = t.m1;
  if (t.kind == X6Tail::SMALL_TILES) {
    t_last_route[5] = 2;
    return launch_x6s<MODE == X6_DGRAD ? X6_DGRAD : X6_FWD, NP>(e, st);   // never X6_WGRAD: plan_x6_tail
  }
  const GemmArgs p = slab_args(e, t.splits, ws);
  t_last_route[4] = p.nsplit; t_last_route[5] = 3; t_last_route[6] = slabs_written(p);
  rc = launch_x6<MODE, NP>(p, st);
  if (rc) return rc;
  return launch_fixup(e, p, st, "x6 tail fix-up");
}

// ---- the route of one GEMM call: plan_gemm decides, launch() executes
struct GemmRoute {
  enum Kind {
    X6S,            // gemm_x6s_kernel: 64 x 128 bf16x6 tiles over the whole problem
    X6_SPLITK_ALL,  // gemm_x6_kernel with K split `splits` ways into slabs + fix-up
    PANEL_THIN,     // gemm_f32_panel_kernel<32, RAGGED>: N <= 32
    PANEL32,        // gemm_f32_panel_kernel<32>: the whole reduction in one workgroup per 32 x 32 tile
    F32_SMALL,      // gemm_f32_small_kernel: 64 x 64 fp32 tiles, K split `splits` ways into slabs + fix-up when > 1
    X6,             // gemm_x6_kernel: 128 x 256 bf16x6 tiles, tail-balanced by launch_x6_tail_split
    F32_FAST,       // gemm_f32_fast_kernel
    F32_VEC,        // gemm_f32_kernel<VEC = true>
    F32,            // gemm_f32_kernel<VEC = false>
  } kind;
  int splits;
};
static_assert(GemmRoute::X6S == GCT_GEMM_ROUTE_X6S && GemmRoute::X6_SPLITK_ALL == GCT_GEMM_ROUTE_X6_SPLITK_ALL &&
                  GemmRoute::PANEL_THIN == GCT_GEMM_ROUTE_PANEL_THIN && GemmRoute::PANEL32 == GCT_GEMM_ROUTE_PANEL32 &&
                  GemmRoute::F32_SMALL == GCT_GEMM_ROUTE_F32_SMALL && GemmRoute::X6 == GCT_GEMM_ROUTE_X6 &&
                  GemmRoute::F32_FAST == GCT_GEMM_ROUTE_F32_FAST && GemmRoute::F32_VEC == GCT_GEMM_ROUTE_F32_VEC &&
                  GemmRoute::F32 == GCT_GEMM_ROUTE_F32, "GCT_GEMM_ROUTE_* are the kinds of GemmRoute");

// The first row whose shape condition holds wins.  Pure: no launches, no environment; `mode` is the arithmetic mode
// (bf16x6 and bf16x3 plan alike: the X6* routes then run the 3- resp. 2-piece kernels), ws / ws_bytes the caller's
// workspace (a slab route is taken only where its slabs fit).
template <bool A_KC, bool B_KC>
GemmRoute plan_gemm(const GemmArgs& g, bool vec, int mode, const float* ws, int64_t ws_bytes) {
  constexpr bool FWD = A_KC && B_KC, DGRAD = A_KC && !B_KC;
  constexpr int MODE = A_KC ? (B_KC ? X6_FWD : X6_DGRAD) : X6_WGRAD;
  const bool x6 = mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3;
  const bool x6_fwd = x6 && FWD && g.epi < EPI_D0, x6_dgrad = x6 && DGRAD && g.epi >= EPI_D0 && g.epi < EPI_SLAB;
  const bool ws_ok = ws && gct_aligned16(ws);
  if (x6_fwd || x6_dgrad) {
    const bool x6s = x6_fwd ? x6s_ok(g, vec) : x6s_dgrad_ok(g, vec);
    if (x6s && x6s_shape(g)) return {GemmRoute::X6S, 1};
    // weight segments of 128 rows (the sampler's mu | log_var, N = 2 x 128): not a whole number of 256-row tiles per
    // segment, so the large kernel cannot take them -- the small-tile kernel for the whole problem instead of fp32 MFMA
    if (x6_fwd && x6s && !x6_ok<X6_FWD>(g, vec) && x6s_tiles(g.M, g.N) >= 96) return {GemmRoute::X6S, 1};
    // few tiles, long reduction (decode FFN-2; dgrad with K' = 1 536 / 2 048 at batch 64): K split over the whole problem
    const int sp = x6_splitk_all_plan(g.M, g.N, g.K);
    if (x6_ok<MODE>(g, vec) && g.nsplit == 1 && ws_ok && sp > 1 && slab_bytes(sp, g.M, g.N) <= ws_bytes)
      return {GemmRoute::X6_SPLITK_ALL, sp};
  }
  // narrow outputs (the vocabulary head, N = 28-31): the ragged panel kernel, exact fp32 MFMA, M / 32 workgroups
  if (FWD && vec && g.N <= 32 && g.K % 256 == 0 && g.epi == GCT_EPI_BIAS && g.nsplit == 1 && g.b_nper >= g.N &&
      g.c_nper >= g.N && g.M >= 1 && g.lda * 4 * 33 < (1ll << 31) && g.ldb * 4 * 33 < (1ll << 31) && g.M < (1ll << 36))
    return {GemmRoute::PANEL_THIN, 1};
  const bool fast = fast_ok<A_KC, B_KC>(g, vec);
  if (FWD && fast && g.nsplit == 1 && skinny_m(g.M, g.N) && g.epi < EPI_D0 && (g.b_nper >= g.N || g.b_nper % 64 == 0)) {
    // ... the panel kernel (whole reduction in one workgroup, one launch) when even 64 x 64 tiles are few
    if (g.K % 256 == 0 && g.lda * 4 * 33 < (1ll << 31) && g.ldb * 4 * 65 < (1ll << 31) &&
        (g.c_nper >= g.N || g.c_nper % 64 == 0)) {
      const int64_t tm32 = (g.M + 31) / 32;
      if (g.N % 32 == 0 && (g.b_nper >= g.N || g.b_nper % 32 == 0) && tm32 * (g.N / 32) <= PANEL32_MAX_TILES)
        return {GemmRoute::PANEL32, 1};
    }
    int64_t ns = 1;
    if (ws_ok) {
      // never more slabs than the caller's workspace holds (fewer splits, same result up to summation order)
      const int64_t slab = g.M * g.N * (int64_t)sizeof(float);
      ns = skinny_splits(g.M, g.N, g.K);
      if (ns * slab > ws_bytes) ns = ws_bytes / slab;
      if (ns < 1) ns = 1;
    }
    return {GemmRoute::F32_SMALL, (int)ns};
  }
  if (x6 && (A_KC || !B_KC) && x6_ok<MODE>(g, vec)) return {GemmRoute::X6, 1};
  return {fast ? GemmRoute::F32_FAST : (vec ? GemmRoute::F32_VEC : GemmRoute::F32), 1};
}

template <bool A_KC, bool B_KC>
int launch(const GemmArgs& g, bool vec, hipStream_t st, float* ws = nullptr, int64_t ws_bytes = 0) {
  constexpr int MODE = A_KC ? (B_KC ? X6_FWD : X6_DGRAD) : X6_WGRAD;
  const int64_t tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN) * g.nsplit;
  if (tiles <= 0) {
    if (A_KC) note_route(GCT_GEMM_ROUTE_NONE, 1, 0, 0);
    return GCT_OK;
  }
  if (tiles > INT_MAX) {
    gct_set_error("gemm: grid too large");
    return GCT_ERR_ARG;
  }
  const int mode = gemm_mode();
  const bool x3 = mode == GCT_GEMM_BF16X3;
  const GemmRoute r = plan_gemm<A_KC, B_KC>(g, vec, mode, ws, ws_bytes);
  if (A_KC) note_route(r.kind, 1, 1, 0);               // forward / dgrad; the slab routes and the tail add theirs below
  switch (r.kind) {
    case GemmRoute::X6S:
      if (x3) return launch_x6s<B_KC ? X6_FWD : X6_DGRAD, 2>(g, st);
      ++g_gemm_launches[1];
      return launch_x6s<B_KC ? X6_FWD : X6_DGRAD, 3>(g, st);
    case GemmRoute::X6_SPLITK_ALL: {
      const GemmArgs p = slab_args(g, r.splits, ws);
      if (A_KC) note_route(r.kind, p.nsplit, 2, slabs_written(p));
      int rc = x3 ? launch_x6<MODE, 2>(p, st) : launch_x6<MODE, 3>(p, st);
      if (!rc) rc = launch_fixup(g, p, st, "x6 split-K fix-up");
      if (!rc && !x3) ++g_gemm_launches[1];
      return rc;
    }
    case GemmRoute::PANEL_THIN:
      ++g_gemm_launches[0];
      return launch_panel<32, true>(g, st);
    case GemmRoute::PANEL32:
      return launch_panel<32>(g, st);
    case GemmRoute::F32_SMALL: {
      const int64_t tiles64 = ((g.M + 63) / 64) * ((g.N + 63) / 64);
      if (r.splits == 1) {
        hipLaunchKernelGGL(gemm_f32_small_kernel, dim3((unsigned)tiles64), dim3(256), 0, st, g);
        GCT_LAUNCH_CHECK("gemm_f32_small");
        return GCT_OK;
      }
      const GemmArgs p = slab_args(g, r.splits, ws);
      if (A_KC) note_route(r.kind, p.nsplit, 2, slabs_written(p));
      hipLaunchKernelGGL(gemm_f32_small_kernel, dim3((unsigned)(tiles64 * p.nsplit)), dim3(256), 0, st, p);
      GCT_LAUNCH_CHECK("gemm_f32_small(split-K)");
      return launch_fixup(g, p, st, "splitk_epilogue");
    }
    case GemmRoute::X6:
      if (x3) return launch_x6_tail_split<MODE, 2>(g, st, ws, ws_bytes);
      ++g_gemm_launches[1];
      return launch_x6_tail_split<MODE, 3>(g, st, ws, ws_bytes);
    default:
      break;
  }
  ++g_gemm_launches[0];
  const dim3 grid((unsigned)tiles), block(256);
  if (r.kind == GemmRoute::F32_FAST)
    hipLaunchKernelGGL((gemm_f32_fast_kernel<A_KC, B_KC>), grid, block, 0, st, g);
  else if (r.kind == GemmRoute::F32_VEC)
    hipLaunchKernelGGL((gemm_f32_kernel<A_KC, B_KC, true>), grid, block, 0, st, g);
  else
    hipLaunchKernelGGL((gemm_f32_kernel<A_KC, B_KC, false>), grid, block, 0, st, g);
  GCT_LAUNCH_CHECK("gemm_f32");
  return GCT_OK;
}

// gemm_x6_bwd_pair_kernel: the wgrad workgroups of gw (slab form, nsplit row ranges) and the dgrad tiles of gd as one grid
template <int NP>
int launch_x6_pair(const GemmArgs& gw, const GemmArgs& gd, hipStream_t st) {
  const int64_t nw = ((gw.M + XBM - 1) / XBM) * ((gw.N + XBN - 1) / XBN) * gw.nsplit;
  const int64_t nd = ((gd.M + XBM - 1) / XBM) * ((gd.N + XBN - 1) / XBN);
  if (nw <= 0 || nd <= 0 || nw + nd > INT_MAX) {
    gct_set_error("gemm_x6 pair: bad grid (%lld + %lld blocks)", (long long)nw, (long long)nd);
    return GCT_ERR_ARG;
  }
  static bool attr_set = false;   // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)gemm_x6_bwd_pair_kernel<NP>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, X_LDS_BYTES);
    if (e != hipSuccess) {
      gct_set_error("gemm_x6 pair: cannot reserve %d bytes of LDS: %s", X_LDS_BYTES, hipGetErrorString(e));
      return GCT_ERR_HIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL((gemm_x6_bwd_pair_kernel<NP>), dim3((unsigned)(nw + nd)), dim3(512), X_LDS_BYTES, st, gw, gd,
                     (unsigned)nw);
  ++(NP == 3 ? g_x6_kernel_launches : g_x3_kernel_launches);
  GCT_LAUNCH_CHECK("gemm_x6 pair");
  return GCT_OK;
}

inline bool al16(const void* p) { return p == nullptr || gct_aligned16(p); }

inline Seg3 mkseg(const float* p0, const float* p1, const float* p2) {
  Seg3 r;
  r.p0 = p0;
  r.d1 = p1 ? (int64_t)(p1 - p0) : 0;
  r.d2 = p2 ? (int64_t)(p2 - p0) : 0;
  return r;
}

// deterministic slab reduction + bias-gradient helpers live in reduce.hip
}  // namespace

int gct_reduce_slabs_seg(const float* slabs, int nslab, int64_t stride, float* d0, float* d1,
                         float* d2, int64_t nper_elems, int64_t n, hipStream_t st);
int gct_reduce_slabs_seg2(const float* sa, int nslab, int64_t stride_a, float* a0, float* a1, float* a2,
                          int64_t nper_a, int64_t na, const float* sb, int64_t stride_b, float* b0, float* b1,
                          float* b2, int64_t nper_b, int64_t nb, hipStream_t st);
int gct_colsum(const float* y0, const float* y1, const float* y2, int64_t ld, int64_t M, int nseg,
               int nper, float* d0, float* d1, float* d2, float* ws, hipStream_t st);
int64_t gct_colsum_ws_floats(int64_t M, int64_t N);

static int wgrad_splits(int64_t M, int64_t Ntot, int64_t K, bool x6 = false) {
  const int64_t tiles = x6 ? ((Ntot + XBM - 1) / XBM) * ((K + XBN - 1) / XBN)
                           : ((Ntot + BM - 1) / BM) * ((K + BN - 1) / BN);
  // exactly one resident round: 256 CUs x 2 blocks (64 KB LDS each) = 512 blocks, never 513
  // (bf16x6: one 144 KB workgroup per CU = 256 blocks)
  int64_t want = (x6 ? 256 : 512) / tiles;
  const int64_t maxs = (M + 4 * BK - 1) / (4 * BK);
  if (want > maxs) want = maxs;
  if (want < 1) want = 1;
  if (want > 64) want = 64;
  return (int)want;
}

// ---- the route of one gct_linear_wgrad call: the one statement of its vector test, kernel, split and bias rules
// (gct_linear_wgrad executes it, gct_wgrad_route reports it)
struct WgradRoute {
  GemmRoute::Kind kind;   // X6 (bf16 tiles), F32_FAST, F32_VEC or F32
  bool bias_fused;        // bias slabs written by the GEMM kernel; else gct_colsum (which borrows ws first)
};

static bool wgrad_vec_shape(int64_t lddy, int64_t ldx, int nper, int K) {
  return (lddy % 4 == 0) && (ldx % 4 == 0) && (nper % 4 == 0) && (K % 4 == 0);
}

// the shape half of a wgrad launch: dW[n][k] = sum_m dY[m][n] X[m][k] as slabs at ws (only its alignment is read)
static GemmArgs wgrad_args(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldx, float* ws) {
  const int64_t Ntot = (int64_t)nseg * nper;
  GemmArgs g = {};
  g.M = Ntot; g.N = K; g.K = M;
  g.lda = lddy; g.a_nper = nper;
  g.ldb = ldx; g.b_nper = INT64_MAX / 4;
  g.c0 = ws; g.ldc = K; g.c_nper = INT64_MAX / 4;
  g.slab_stride = Ntot * K;
  g.ksplit = BK; g.nsplit = 1; g.epi = EPI_SLAB;
  return g;
}

// Pure: no launch, no device access, no environment.  Sets g.ksplit / g.nsplit: the rows split into `wgrad_splits`
// ranges of whole 32-row tiles (fewer when they do not all get a tile).
static WgradRoute plan_wgrad(GemmArgs& g, bool vec, bool want_bias, int mode) {
  const int64_t M = g.K;
  g.ksplit = BK; g.nsplit = 1;
  // bf16x6 or bf16x3: same route.  The kernel choice does not depend on the split (every split is whole K-tiles)
  const bool use_x6 = plan_gemm<false, false>(g, vec, mode, nullptr, 0).kind == GemmRoute::X6;
  const int splits = wgrad_splits(M, g.M, g.N, use_x6);
  int64_t ks = (M + splits - 1) / splits;
  ks = (ks + BK - 1) / BK * BK;
  g.ksplit = ks > 0 ? ks : BK;
  g.nsplit = (int)((M + g.ksplit - 1) / g.ksplit);
  if (g.nsplit < 1) g.nsplit = 1;
  const GemmRoute::Kind kind = plan_gemm<false, false>(g, vec, mode, nullptr, 0).kind;   // what launch() will take
  return {kind, want_bias && (kind == GemmRoute::X6 || kind == GemmRoute::F32_FAST)};
}

extern "C" int64_t gct_wgrad_ws_bytes(int64_t M, int64_t Ntot, int64_t K) {
  const int s1 = wgrad_splits(M, Ntot, K), s2 = wgrad_splits(M, Ntot, K, true);
  const int s = s1 > s2 ? s1 : s2;
  const int64_t slab = (int64_t)s * Ntot * K;
  const int64_t cs = gct_colsum_ws_floats(M, Ntot);
  const int64_t need = slab + 4 + (int64_t)s * Ntot;   // weight slabs + fused bias slabs
  return (need > cs ? need : cs) * (int64_t)sizeof(float) + 256;
}

// the shape half of a forward / dgrad launch (the calls add their addresses, the route queries stand-ins that carry the
// alignment and which buffers there are), and the calls' vector tests
static GemmArgs fwd_args(int64_t M, int K, int nseg, int nper, int64_t ldx, int64_t ldw, int64_t ldy, int epi) {
  GemmArgs g = {};
  g.M = M; g.N = (int64_t)nseg * nper; g.K = K;
  g.lda = ldx; g.a_nper = INT64_MAX / 4;
  g.ldb = ldw; g.b_nper = nper;
  g.ldc = ldy; g.c_nper = nper;
  g.ksplit = K; g.nsplit = 1; g.epi = epi;
  return g;
}
static bool fwd_vec_shape(int K, int64_t ldx, int64_t ldw) { return (ldx % 4 == 0) && (ldw % 4 == 0) && (K % 4 == 0); }

static GemmArgs dgrad_args(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldw, int64_t lddx, int depi) {
  GemmArgs g = {};
  g.M = M; g.N = K; g.K = (int64_t)nseg * nper;  // reduce over the layer's output features
  g.lda = lddy; g.a_nper = nper;
  g.ldb = ldw; g.b_nper = nper;
  g.ldc = lddx; g.c_nper = INT64_MAX / 4;
  g.ksplit = g.K; g.nsplit = 1; g.epi = EPI_D0 + depi;
  return g;
}
static bool dgrad_vec_shape(int nper, int K, int64_t lddy, int64_t ldw) {
  return (lddy % 4 == 0) && (ldw % 4 == 0) && (nper % 4 == 0) && (K % 4 == 0);
}

extern "C" int gct_linear_fwd(const float* x, int64_t ldx, int64_t M, int K, const float* w0,
                              const float* w1, const float* w2, int64_t ldw, const uint16_t* wp0,
                              int64_t plane_stride, const float* b0, const float* b1,
                              const float* b2, int nseg, int nper, float* y0, float* y1, float* y2,
                              int64_t ldy, int epi, const float* resid, float* pre, float p,
                              uint64_t seed, uint32_t site, float* ws, int64_t ws_bytes,
                              const int32_t* quad_map, void* stream) {
  GCT_CHECK_ARG(x && w0 && y0 && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0,
                "linear_fwd: bad args");
  GCT_CHECK_ARG(!quad_map || M % 4 == 0, "linear_fwd: compacted rows come in quads");
  GCT_CHECK_ARG(ws_bytes >= 0, "linear_fwd: negative workspace size");
  GCT_CHECK_ARG(nseg < 2 || (w1 && y1), "linear_fwd: missing segment 1");
  GCT_CHECK_ARG(nseg < 3 || (w2 && y2), "linear_fwd: missing segment 2");
  GCT_CHECK_ARG(epi == GCT_EPI_BIAS || nseg == 1, "linear_fwd: fused epilogues need nseg == 1");
  GCT_CHECK_ARG(epi >= GCT_EPI_BIAS && epi <= GCT_EPI_GELU_DROP_SAVE, "linear_fwd: unknown epilogue %d", epi);
  GCT_CHECK_ARG((epi != GCT_EPI_GELU_DROP && epi != GCT_EPI_GELU_DROP_SAVE) || pre, "linear_fwd: GELU epilogue needs pre");
  GCT_CHECK_ARG(epi != GCT_EPI_DROP_RESID || resid, "linear_fwd: residual epilogue needs resid");
  GCT_CHECK_ARG(p >= 0.f && p < 1.f, "linear_fwd: dropout p out of range");
  GCT_CHECK_ARG(!b0 || nseg < 2 || b1, "linear_fwd: bias of segment 1 missing");
  GCT_CHECK_ARG(!b0 || nseg < 3 || b2, "linear_fwd: bias of segment 2 missing");
  GemmArgs g = fwd_args(M, K, nseg, nper, ldx, ldw, ldy, epi);
  g.a = mkseg(x, nullptr, nullptr);
  g.b = mkseg(w0, w1, w2);
  g.c0 = y0; g.c_d1 = y1 ? y1 - y0 : 0; g.c_d2 = y2 ? y2 - y0 : 0;
  g.bias0 = b0; g.bias_d1 = (b0 && b1) ? b1 - b0 : 0; g.bias_d2 = (b0 && b2) ? b2 - b0 : 0;
  g.resid = resid; g.pre = pre;
  g.thr = gct_drop_threshold(p); g.keep_scale = 1.0f / (1.0f - p); g.rng = gct_rng_make(seed, site);
  g.bp0 = wp0; g.bp_stride = plane_stride;
  g.quad_map = quad_map;          // rows are a quad compaction: the dropout coordinates of the epilogues follow the map
  const bool vec = al16(x) && al16(w0) && al16(w1) && al16(w2) && fwd_vec_shape(K, ldx, ldw);
  return launch<true, true>(g, vec, (hipStream_t)stream, ws, ws ? ws_bytes : 0);   // every slab route checks its need against ws_bytes
}

extern "C" int gct_gemm_set_mode(int mode) {
  GCT_CHECK_ARG(mode == GCT_GEMM_F32 || mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3,
                "gemm_set_mode: unknown mode %d", mode);
  g_gemm_mode = mode;
  return GCT_OK;
}
extern "C" int gct_gemm_get_mode(void) { return gemm_mode(); }
extern "C" int64_t gct_gemm_x6_kernel_launches(void) { return g_x6_kernel_launches; }
extern "C" int64_t gct_gemm_x3_launches(void) { return g_x3_kernel_launches; }
extern "C" int gct_gemm_launch_counts(int64_t* out2) {
  GCT_CHECK_ARG(out2, "gemm_launch_counts: null");
  out2[0] = g_gemm_launches[0]; out2[1] = g_gemm_launches[1];
  return GCT_OK;
}

extern "C" int gct_split_planes(const float* src, int64_t numel, uint16_t* planes, int64_t plane_stride,
                                void* stream) {
  GCT_CHECK_ARG(src && planes && numel >= 0 && numel % 4 == 0 && plane_stride >= numel && plane_stride % 4 == 0 &&
                    gct_aligned16(src) && ((((uintptr_t)planes) & 7u) == 0),
                "split_planes: bad args (numel and plane_stride must be multiples of 4, src 16-B aligned)");
  if (numel == 0) return GCT_OK;
  const int64_t n4 = numel / 4;
  hipLaunchKernelGGL(split_planes_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     src, planes, n4, plane_stride);
  GCT_LAUNCH_CHECK("split_planes");
  return GCT_OK;
}

// Workspace queries: the slabs of every route a call of this shape can take, from the routes' own split rules (an upper
// bound: alignment and the epilogue are not known here).
extern "C" int64_t gct_linear_fwd_ws_bytes(int64_t M, int K, int Ntot) {
  int64_t need = 0, m1 = 0;
  if (skinny_m(M, Ntot)) {
    need = slab_bytes(skinny_splits(M, Ntot, K), M, Ntot);
  } else {
    const int s = x6_tail_plan(M, Ntot, K, &m1);      // bf16x6 tail balancing: s slabs of the tail rows
    need = slab_bytes(s, M - m1, Ntot);
  }
  const int64_t all = slab_bytes(x6_splitk_all_plan(M, Ntot, K), M, Ntot);
  return (need > all ? need : all) + 256;
}

extern "C" int64_t gct_linear_dgrad_ws_bytes(int64_t M, int Ntot, int K) {
  int64_t m1 = 0;
  const int s = x6_tail_plan(M, K, Ntot, &m1);       // dx is [M][K], reduced over Ntot
  const int64_t tail = slab_bytes(s, M - m1, K);
  const int64_t all = slab_bytes(x6_splitk_all_plan(M, K, Ntot), M, K);
  return (tail > all ? tail : all) + 256;
}

extern "C" int gct_linear_dgrad(const float* dy0, const float* dy1, const float* dy2, int64_t lddy,
                                int64_t M, int nseg, int nper, const float* w0, const float* w1,
                                const float* w2, int64_t ldw, const uint16_t* wp0,
                                int64_t plane_stride, int K, float* dx, int64_t lddx, int depi,
                                const float* pre, float p, uint64_t seed, uint32_t site,
                                float* ws, int64_t ws_bytes, const int32_t* quad_map, int64_t pre_rows,
                                void* stream) {
  GCT_CHECK_ARG(ws_bytes >= 0, "linear_dgrad: negative workspace size");
  GCT_CHECK_ARG(dy0 && w0 && dx && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0,
                "linear_dgrad: bad args");
  GCT_CHECK_ARG(!quad_map || M % 4 == 0, "linear_dgrad: compacted rows come in quads");
  GCT_CHECK_ARG(nseg < 2 || (w1 && dy1), "linear_dgrad: missing segment 1");
  GCT_CHECK_ARG(nseg < 3 || (w2 && dy2), "linear_dgrad: missing segment 2");
  GCT_CHECK_ARG(depi >= GCT_DEPI_STORE && depi <= GCT_DEPI_MUL_SAVED, "linear_dgrad: unknown epilogue %d", depi);
  GCT_CHECK_ARG(depi != GCT_DEPI_GELU_BWD || pre, "linear_dgrad: GELU bwd needs pre");
  GCT_CHECK_ARG(depi != GCT_DEPI_MUL_SAVED || pre, "linear_dgrad: saved-factor epilogue needs pre");
  GCT_CHECK_ARG(p >= 0.f && p < 1.f, "linear_dgrad: dropout p out of range");
  GemmArgs g = dgrad_args(M, nseg, nper, K, lddy, ldw, lddx, depi);
  g.a = mkseg(dy0, dy1, dy2);
  g.b = mkseg(w0, w1, w2);
  g.c0 = dx;
  g.pre_in = pre;
  g.thr = gct_drop_threshold(p); g.keep_scale = 1.0f / (1.0f - p); g.rng = gct_rng_make(seed, site);
  g.bp0 = wp0; g.bp_stride = plane_stride;
  g.quad_map = quad_map;
  g.pre_rows = quad_map ? pre_rows : 0;
  const bool vec = al16(dy0) && al16(dy1) && al16(dy2) && al16(w0) && al16(w1) && al16(w2) &&
                   dgrad_vec_shape(nper, K, lddy, ldw);
  return launch<true, false>(g, vec, (hipStream_t)stream, ws, ws ? ws_bytes : 0);
}

// ---- route queries of the forward / dgrad calls: the calls' own GemmArgs helpers, plan_gemm and plan_x6_tail on
// stand-in addresses (only alignment and presence are read); launch() writes the same eight numbers as it launches
template <bool B_KC>
static void report_route(const GemmArgs& g, bool vec, int mode, const float* ws, int64_t ws_bytes, int64_t* out8) {
  constexpr int MODE = B_KC ? X6_FWD : X6_DGRAD;
  int64_t r8[8] = {GCT_GEMM_ROUTE_NONE, 1, 0, 0, 1, 0, 0, 0};
  if (g.M > 0) {
    const GemmRoute r = plan_gemm<true, B_KC>(g, vec, mode, ws, ws_bytes);
    r8[0] = r.kind; r8[5] = 1;
    if (r.kind == GemmRoute::X6_SPLITK_ALL || (r.kind == GemmRoute::F32_SMALL && r.splits > 1)) {
      const GemmArgs p = slab_args(g, r.splits, nullptr);
      r8[1] = p.nsplit; r8[5] = 2; r8[6] = slabs_written(p);
    } else if (r.kind == GemmRoute::X6) {
      const X6Tail t = plan_x6_tail<MODE>(g, ws, ws_bytes);
      if (t.kind != X6Tail::NONE) { r8[2] = t.kind; r8[3] = t.m1; r8[5] = 2; }
      if (t.kind == X6Tail::SLABS) {
        const GemmArgs p = slab_args(x6_tail_args(g, t.m1), t.splits, nullptr);
        r8[4] = p.nsplit; r8[5] = 3; r8[6] = slabs_written(p);
      }
    }
  }
  for (int i = 0; i < 8; ++i) out8[i] = r8[i];
}

static const float* standin(bool present, bool aligned16) {
  return present ? reinterpret_cast<const float*>((uintptr_t)(aligned16 ? 16 : 4)) : nullptr;
}

extern "C" int gct_linear_fwd_route(int64_t M, int K, int nseg, int nper, int64_t ldx, int64_t ldw, int64_t ldy, int epi,
                                    int aligned16, int have_planes, int have_bias, int mode, int64_t ws_bytes,
                                    int64_t* out8) {
  GCT_CHECK_ARG(out8 && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0 && ldx >= 0 && ldw >= 0 && ldy >= 0 &&
                    ws_bytes >= 0, "linear_fwd_route: bad args");
  GCT_CHECK_ARG(epi >= GCT_EPI_BIAS && epi <= GCT_EPI_GELU_DROP_SAVE, "linear_fwd_route: unknown epilogue %d", epi);
  GCT_CHECK_ARG(epi == GCT_EPI_BIAS || nseg == 1, "linear_fwd_route: fused epilogues need nseg == 1");
  GCT_CHECK_ARG(mode == GCT_GEMM_F32 || mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3,
                "linear_fwd_route: unknown mode %d", mode);
  const bool al = aligned16 != 0;
  GemmArgs g = fwd_args(M, K, nseg, nper, ldx, ldw, ldy, epi);
  g.a.p0 = standin(true, al);
  g.b.p0 = standin(true, al);
  g.b.d1 = nseg > 1 ? (int64_t)nper * ldw : 0; g.b.d2 = nseg > 2 ? 2 * (int64_t)nper * ldw : 0;
  g.c0 = const_cast<float*>(standin(true, al));
  g.c_d1 = nseg > 1 ? nper : 0; g.c_d2 = nseg > 2 ? 2 * (int64_t)nper : 0;
  g.bias0 = standin(have_bias != 0, al); g.bias_d1 = have_bias ? g.c_d1 : 0; g.bias_d2 = have_bias ? g.c_d2 : 0;
  g.resid = standin(epi == GCT_EPI_DROP_RESID, al);
  g.pre = const_cast<float*>(standin(epi == GCT_EPI_GELU_DROP || epi == GCT_EPI_GELU_DROP_SAVE, al));
  g.bp0 = reinterpret_cast<const uint16_t*>(standin(have_planes != 0, true));
  g.bp_stride = g.N * g.K;
  report_route<true>(g, al && fwd_vec_shape(K, ldx, ldw), mode, standin(ws_bytes > 0, al), ws_bytes, out8);
  return GCT_OK;
}

extern "C" int gct_linear_dgrad_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldw, int64_t lddx,
                                      int depi, int aligned16, int have_planes, int mode, int64_t ws_bytes,
                                      int64_t* out8) {
  GCT_CHECK_ARG(out8 && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0 && lddy >= 0 && ldw >= 0 && lddx >= 0 &&
                    ws_bytes >= 0, "linear_dgrad_route: bad args");
  GCT_CHECK_ARG(depi >= GCT_DEPI_STORE && depi <= GCT_DEPI_MUL_SAVED, "linear_dgrad_route: unknown epilogue %d", depi);
  GCT_CHECK_ARG(mode == GCT_GEMM_F32 || mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3,
                "linear_dgrad_route: unknown mode %d", mode);
  const bool al = aligned16 != 0;
  GemmArgs g = dgrad_args(M, nseg, nper, K, lddy, ldw, lddx, depi);
  g.a.p0 = standin(true, al);
  g.a.d1 = nseg > 1 ? nper : 0; g.a.d2 = nseg > 2 ? 2 * (int64_t)nper : 0;
  g.b.p0 = standin(true, al);
  g.b.d1 = nseg > 1 ? (int64_t)nper * ldw : 0; g.b.d2 = nseg > 2 ? 2 * (int64_t)nper * ldw : 0;
  g.c0 = const_cast<float*>(standin(true, al));
  g.pre_in = standin(depi == GCT_DEPI_GELU_BWD || depi == GCT_DEPI_MUL_SAVED, al);
  g.bp0 = reinterpret_cast<const uint16_t*>(standin(have_planes != 0, true));
  g.bp_stride = g.N * g.K;
  report_route<false>(g, al && dgrad_vec_shape(nper, K, lddy, ldw), mode, standin(ws_bytes > 0, al), ws_bytes, out8);
  return GCT_OK;
}

extern "C" int gct_gemm_last_route(int64_t* out8) {
  GCT_CHECK_ARG(out8, "gemm_last_route: null");
  for (int i = 0; i < 8; ++i) out8[i] = t_last_route[i];
  return GCT_OK;
}

extern "C" int gct_linear_wgrad(const float* dy0, const float* dy1, const float* dy2, int64_t lddy,
                                int64_t M, int nseg, int nper, const float* x, int64_t ldx, int K,
                                float* dw0, float* dw1, float* dw2, int64_t lddw, float* db0,
                                float* db1, float* db2, float* ws, const int32_t* tile_list,
                                const int32_t* tile_count, void* stream) {
  GCT_CHECK_ARG(dy0 && x && dw0 && ws && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0,
                "linear_wgrad: bad args");
  GCT_CHECK_ARG(nseg < 2 || (dy1 && dw1), "linear_wgrad: missing segment 1");
  GCT_CHECK_ARG(nseg < 3 || (dy2 && dw2), "linear_wgrad: missing segment 2");
  GCT_CHECK_ARG(lddw == K, "linear_wgrad: dW must be dense [nper][K]");
  hipStream_t st = (hipStream_t)stream;
  const int64_t Ntot = (int64_t)nseg * nper;
  const bool vec = al16(dy0) && al16(dy1) && al16(dy2) && al16(x) && wgrad_vec_shape(lddy, ldx, nper, K);
  GemmArgs g = wgrad_args(M, nseg, nper, K, lddy, ldx, ws);
  g.a = mkseg(dy0, dy1, dy2);
  g.b = mkseg(x, nullptr, nullptr);
  const WgradRoute r = plan_wgrad(g, vec, db0 != nullptr, gemm_mode());   // sets g.ksplit / g.nsplit
  if (r.kind == GemmRoute::X6 && tile_list && tile_count) { g.kt_list = tile_list; g.kt_count = tile_count; }   // other kernels reduce over every row
  // bias gradients: fused into the GEMM on the fast path (column sums of the A tiles), else a
  // separate column-sum pass that borrows ws before the slabs are written (stream-ordered)
  float* bslab = nullptr;
  if (db0) {
    if (r.bias_fused) {
      int64_t off = (int64_t)g.nsplit * g.slab_stride;
      off = (off + 3) / 4 * 4;
      bslab = ws + off;                     // [nsplit][Ntot] right behind the weight slabs
      g.bias_slab = bslab;
    } else {
      int rc = gct_colsum(dy0, dy1, dy2, lddy, M, nseg, nper, db0, db1, db2, ws, st);
      if (rc) return rc;
    }
  }
  int rc = launch<false, false>(g, vec, st);
  if (rc) return rc;
  if (bslab)     // weight and bias slabs in one launch
    return gct_reduce_slabs_seg2(ws, g.nsplit, g.slab_stride, dw0, dw1, dw2, (int64_t)nper * K, Ntot * K, bslab, Ntot,
                                 db0, db1, db2, nper, Ntot, st);
  return gct_reduce_slabs_seg(ws, g.nsplit, g.slab_stride, dw0, dw1, dw2, (int64_t)nper * K, Ntot * K, st);
}

extern "C" int gct_wgrad_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldx, int aligned16,
                               int want_bias, int mode, int64_t* out4) {
  GCT_CHECK_ARG(out4 && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0 && lddy >= 0 && ldx >= 0,
                "wgrad_route: bad args");
  GCT_CHECK_ARG(mode == GCT_GEMM_F32 || mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3,
                "wgrad_route: unknown mode %d", mode);
  // only the alignment of the workspace is read: a stand-in address with the alignment asked about
  float* const ws = reinterpret_cast<float*>((uintptr_t)(aligned16 ? 16 : 4));
  GemmArgs g = wgrad_args(M, nseg, nper, K, lddy, ldx, ws);
  const WgradRoute r = plan_wgrad(g, aligned16 && wgrad_vec_shape(lddy, ldx, nper, K), want_bias != 0, mode);
  out4[0] = r.kind == GemmRoute::X6 ? GCT_WGRAD_BF16_TILES
            : r.kind == GemmRoute::F32_FAST ? GCT_WGRAD_F32_FAST
            : r.kind == GemmRoute::F32_VEC ? GCT_WGRAD_F32_VEC : GCT_WGRAD_F32_SCALAR;
  out4[1] = g.nsplit;
  out4[2] = g.ksplit;
  out4[3] = r.bias_fused ? 1 : 0;
  return GCT_OK;
}

// =====================================================================================
// One Linear's backward as ONE launch (gemm_x6_bwd_pair_kernel): the dgrad tiles and the weight-gradient workgroups of
// the same dY share a grid, so neither has to be a whole number of rounds on the 256 CUs alone -- the dgrad needs no
// tail launch / fix-up and the weight gradient need not be cut into exactly 256 workgroups.
//
// The split count comes from a list-scheduling model of that grid (one 144 KB workgroup per CU, blocks dispatched in
// order: the wgrad workgroups first, each dgrad tile on the CU that frees first).  Unit: the time of one dgrad K-tile
// (128 x 256 x 32) on its CU.
//   dgrad tile       o + K'/32 + e(epilogue)         o = 3.3 (x6_tail_plan's prologue + epilogue, s_memtime stamps)
//   wgrad workgroup  o_w + c_w * rows/(32 s) + st    both operands are split on the fly: a longer K-tile (c_w)
//   later reduction  r * s * Ntot * K                the slabs are read once more by the deferred reduction
// =====================================================================================
namespace {
constexpr double PAIR_O = 3.3, PAIR_E_RMW = 0.4;          // dgrad: fixed part; epilogues that read a second [M][N] operand
constexpr double PAIR_OW = 3.3, PAIR_CW = 1.12, PAIR_ST = 0.5;   // wgrad: fixed part, K-tile ratio, 128 KB slab store
constexpr double PAIR_RED = 1.0 / 2.8e6;                  // K-tile times per slab element reduced later (4 B at ~4 TB/s,
                                                          // 2.8 us per K-tile)
constexpr double PAIR_LAUNCH = 1.0;                       // ramp + drain of one more launch on the stream
// Lab (tools/kernel_bench.py --suite bwdpair, profiles/r08_bwd_pair_lab_every_shape_paired.log and, with the rule
// below in place, r08_bwd_pair_lab.log; the Linear shapes of a layer at 40 960,
// 18 016 and 10 432 rows, paired and separate calls alternated): one unit is 2.0-2.3 us both ways, i.e. the model ranks
// the two ways as the clock does, with one exception.  Where the model finds no partial round to fill -- the dgrad alone
// is a whole number of rounds (FFN-2 at 40 960 rows: 2 560 tiles) or fits into one round behind a weight gradient that
// already is one (10 432 rows: 164 tiles) -- all it predicts is the launch saved, and the clock gives that back: the two
// problems then only share the L2 (measured 0.98-1.03 of the separate calls).  So a pair must save at least this much
// beyond nothing, i.e. fill a round, not just drop a launch:
constexpr double PAIR_MIN_GAIN = 2.0;

struct BwdPairPlan {
  bool paired;
  int nsplit;          // wgrad row ranges (slabs) of the call, paired or not
  int64_t ksplit;      // rows per range, a multiple of 32
  bool bias_fused;
  int64_t wblocks, dblocks;   // blocks of the pair grid (0 when not paired)
  double makespan;     // modelled K-tile times of the paired launch (+ its share of the reduction); 0 when not modelled
  double separate;     // the same model for the two separate calls
};

// end of the last block when nw blocks of tw and then nd blocks of td are dispatched in order to 256 CUs
double pair_makespan(int64_t nw, double tw, int64_t nd, double td) {
  constexpr int64_t CUS = 256;
  const int64_t q = nw / CUS, nb = nw % CUS, na = CUS - nb;   // nb CUs run q + 1 wgrad blocks, na run q
  const double fa = (double)q * tw, fb = (double)(q + 1) * tw;
  double end = nw > 0 ? (nb ? fb : fa) : 0.0;
  int64_t ka = 0, kb = 0;
  for (int64_t left = nd; left > 0;) {
    const double sa = fa + (double)ka * td, sb = fb + (double)kb * td;
    const bool a = nb == 0 || sa <= sb;
    const double fin = (a ? sa : sb) + td;
    if (fin > end) end = fin;
    left -= a ? na : nb;
    ++(a ? ka : kb);
  }
  return end;
}

// last round of a dgrad launched alone, in rounds: what x6_tail_plan decides (1.0: an ordinary round)
double x6_tail_cost(int64_t M, int64_t N, int64_t K, int* launches) {
  int64_t m1 = 0;
  const int s = x6_tail_plan(M, N, K, &m1);
  *launches = 1;
  if (s == 1) return 1.0;
  const int64_t tn = (N + XBN - 1) / XBN, rem = (((M + XBM - 1) / XBM) * tn) % 256, nkt = K / XBK;
  *launches = (nkt <= 32 && x6s_tiles(M - m1, N) <= X6_TAIL_SMALL_MAX) ? 2 : 3;
  return (double)((rem * s + 255) / 256) * (PAIR_O + (double)nkt / s) / (PAIR_O + nkt) + 0.05;
}

// Pure (shape only): the wgrad split of the paired launch and the modelled times of both ways.  M rows, dW [Ntot][K],
// dX [M][K] reduced over Ntot; ws_bytes: the weight-gradient workspace (slabs + bias slabs must fit).
BwdPairPlan plan_bwd_pair_shape(int64_t M, int64_t Ntot, int64_t K, int depi, bool want_bias, int64_t ws_bytes) {
  BwdPairPlan r = {false, 1, BK, false, 0, 0, 0.0, 0.0};
  const int64_t nktm = M / XBK;
  if (M <= 0 || M % XBK != 0 || Ntot % XBK != 0) return r;
  const int64_t tw_tiles = ((Ntot + XBM - 1) / XBM) * ((K + XBN - 1) / XBN);
  const int64_t td_tiles = ((M + XBM - 1) / XBM) * ((K + XBN - 1) / XBN);
  const double td = PAIR_O + (double)(Ntot / XBK) + (depi == GCT_DEPI_STORE ? 0.0 : PAIR_E_RMW);
  auto wcost = [&](int64_t ks) { return PAIR_OW + PAIR_CW * (double)(ks / XBK) + PAIR_ST; };
  auto red = [&](int ns) { return PAIR_RED * (double)ns * (double)Ntot * (double)K; };
  double best = 0.0;
  for (int64_t s = 1; s <= 64 && nktm / s >= 4; ++s) {
    const int64_t ks = (nktm + s - 1) / s * XBK, ns = (M + ks - 1) / ks;
    if (ns != s) continue;                               // the same ranges as a smaller s
    const int64_t need = (ns * Ntot * K + 4 + (want_bias ? ns * Ntot : 0)) * (int64_t)sizeof(float);
    if (need > ws_bytes) break;
    const double c = pair_makespan(tw_tiles * ns, wcost(ks), td_tiles, td) + red((int)ns) + PAIR_LAUNCH;
    if (r.makespan == 0.0 || c < best - 1e-9) { best = c; r.makespan = c; r.nsplit = (int)ns; r.ksplit = ks; }
  }
  if (r.makespan == 0.0) return r;
  // the two separate calls: the wgrad in rounds of its own split, the dgrad in rounds with its balanced tail
  const int ss = wgrad_splits(M, Ntot, K, true);
  const int64_t kss = ((M + ss - 1) / ss + BK - 1) / BK * BK, nss = (M + kss - 1) / kss;
  int dl = 1;
  const double tail = x6_tail_cost(M, K, Ntot, &dl);
  const double rounds_d = td_tiles <= 256 ? 1.0 : (double)(td_tiles / 256) + (td_tiles % 256 ? tail : 0.0);
  r.separate = (double)((tw_tiles * nss + 255) / 256) * wcost(kss) + red((int)nss) + rounds_d * td + PAIR_LAUNCH * (1 + dl);
  r.wblocks = tw_tiles * r.nsplit;
  r.dblocks = td_tiles;
  r.paired = r.separate - r.makespan >= PAIR_MIN_GAIN;
  return r;
}

struct BwdShape {           // what the routes of a gct_linear_bwd call depend on
  int64_t M; int nseg, nper, K; int64_t lddy, ldx, ldw, lddx;
  int depi; bool aligned16, planes, want_bias; int mode;
};

GemmArgs dgrad_shape_args(const BwdShape& b, float* dx, const uint16_t* wp0, int64_t plane_stride) {
  GemmArgs g = dgrad_args(b.M, b.nseg, b.nper, b.K, b.lddy, b.ldw, b.lddx, b.depi);
  g.c0 = dx;
  g.bp0 = wp0; g.bp_stride = plane_stride;
  return g;
}

// Pure: the plan of a gct_linear_bwd call.  Paired only when BOTH problems would take GemmRoute::X6 on their own and
// the model says that the pair is the shorter way; gw gets the split of the call either way (plan_wgrad's when not paired).
BwdPairPlan plan_bwd_pair(const BwdShape& b, GemmArgs& gw, const GemmArgs& gd, int64_t wws_bytes, const float* dws,
                          int64_t dws_bytes) {
  const bool vec_w = b.aligned16 && wgrad_vec_shape(b.lddy, b.ldx, b.nper, b.K);
  const bool vec_d = b.aligned16 && dgrad_vec_shape(b.nper, b.K, b.lddy, b.ldw);
  const WgradRoute wr = plan_wgrad(gw, vec_w, b.want_bias, b.mode);          // sets gw.ksplit / gw.nsplit
  BwdPairPlan r = {false, gw.nsplit, gw.ksplit, wr.bias_fused, 0, 0, 0.0, 0.0};
  if (wr.kind != GemmRoute::X6) return r;
  if (plan_gemm<true, false>(gd, vec_d, b.mode, dws, dws_bytes).kind != GemmRoute::X6) return r;
  const BwdPairPlan m = plan_bwd_pair_shape(b.M, (int64_t)b.nseg * b.nper, b.K, b.depi, b.want_bias, wws_bytes);
  r.makespan = m.makespan; r.separate = m.separate;
  if (!m.paired) return r;
  GemmArgs t = gw;
  t.ksplit = m.ksplit; t.nsplit = m.nsplit;
  if (plan_gemm<false, false>(t, vec_w, b.mode, nullptr, 0).kind != GemmRoute::X6) return r;
  gw.ksplit = m.ksplit; gw.nsplit = m.nsplit;
  r.paired = true; r.nsplit = m.nsplit; r.ksplit = m.ksplit; r.bias_fused = b.want_bias;
  r.wblocks = m.wblocks; r.dblocks = m.dblocks;
  return r;
}

// [lo, hi) of a strided matrix of `rows` x `cols` floats
inline bool ranges_overlap(const float* a, int64_t arows, int64_t lda, int64_t acols, const float* b, int64_t brows,
                           int64_t ldb, int64_t bcols) {
  if (!a || !b || arows <= 0 || brows <= 0) return false;
  const float* ae = a + (arows - 1) * lda + acols;
  const float* be = b + (brows - 1) * ldb + bcols;
  return (uintptr_t)a < (uintptr_t)be && (uintptr_t)b < (uintptr_t)ae;
}
}  // namespace

extern "C" int64_t gct_linear_bwd_ws_bytes(int64_t M, int64_t Ntot, int64_t K) { return gct_wgrad_ws_bytes(M, Ntot, K); }

extern "C" int gct_linear_bwd_route(int64_t M, int nseg, int nper, int K, int64_t lddy, int64_t ldx, int64_t ldw,
                                    int64_t lddx, int depi, int aligned16, int have_planes, int want_bias, int mode,
                                    int64_t ws_bytes, int64_t* out8) {
  GCT_CHECK_ARG(out8 && M >= 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0 && lddy >= 0 && ldx >= 0 && ldw >= 0 &&
                    lddx >= 0 && ws_bytes >= 0, "linear_bwd_route: bad args");
  GCT_CHECK_ARG(depi >= GCT_DEPI_STORE && depi <= GCT_DEPI_MUL_SAVED, "linear_bwd_route: unknown epilogue %d", depi);
  GCT_CHECK_ARG(mode == GCT_GEMM_F32 || mode == GCT_GEMM_BF16X6 || mode == GCT_GEMM_BF16X3,
                "linear_bwd_route: unknown mode %d", mode);
  // only the alignment of the buffers is read: stand-in addresses with the alignment asked about
  const uintptr_t al = aligned16 ? 16 : 4;
  const BwdShape b = {M, nseg, nper, K, lddy, ldx, ldw, lddx, depi, aligned16 != 0, have_planes != 0, want_bias != 0, mode};
  GemmArgs gw = wgrad_args(M, nseg, nper, K, lddy, ldx, reinterpret_cast<float*>(al));
  const GemmArgs gd = dgrad_shape_args(b, reinterpret_cast<float*>(al),
                                       have_planes ? reinterpret_cast<const uint16_t*>((uintptr_t)16) : nullptr, K * (int64_t)nseg * nper);
  const int64_t dws_bytes = gct_linear_dgrad_ws_bytes(M, nseg * nper, K);
  const BwdPairPlan r = plan_bwd_pair(b, gw, gd, ws_bytes, reinterpret_cast<const float*>(al), dws_bytes);
  out8[0] = r.paired ? 1 : 0;
  out8[1] = r.nsplit;
  out8[2] = r.ksplit;
  out8[3] = r.bias_fused ? 1 : 0;
  out8[4] = r.wblocks;
  out8[5] = r.dblocks;
  out8[6] = (int64_t)(r.makespan * 1000.0 + 0.5);
  out8[7] = (int64_t)(r.separate * 1000.0 + 0.5);
  return GCT_OK;
}

extern "C" int gct_linear_bwd(const float* dy0, const float* dy1, const float* dy2, int64_t lddy, int64_t M, int nseg,
                              int nper, const float* x, int64_t ldx, int K, float* dw0, float* dw1, float* dw2,
                              int64_t lddw, float* db0, float* db1, float* db2, float* wws, int64_t wws_bytes,
                              const int32_t* tile_list, const int32_t* tile_count, const float* w0, const float* w1,
                              const float* w2, int64_t ldw, const uint16_t* wp0, int64_t plane_stride, float* dx,
                              int64_t lddx, int depi, const float* pre, float p, uint64_t seed, uint32_t site,
                              float* dws, int64_t dws_bytes, const int32_t* quad_map, int64_t pre_rows, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  bool pair_ok = dy0 && x && dw0 && wws && w0 && dx && M > 0 && K > 0 && nseg >= 1 && nseg <= 3 && nper > 0 &&
                 lddw == K && wws_bytes > 0 && dws_bytes >= 0 && (nseg < 2 || (dy1 && dw1 && w1)) &&
                 (nseg < 3 || (dy2 && dw2 && w2)) && depi >= GCT_DEPI_STORE && depi <= GCT_DEPI_MUL_SAVED &&
                 (!quad_map || M % 4 == 0) && ((depi != GCT_DEPI_GELU_BWD && depi != GCT_DEPI_MUL_SAVED) || pre) &&
                 p >= 0.f && p < 1.f;
  if (pair_ok) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;   // a captured graph keeps today's kernels
    pair_ok = hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
  }
  if (pair_ok) {       // the pair runs both problems at once: dX must not overwrite what the weight gradient reads
    const float* dys[3] = {dy0, dy1, dy2};
    for (int sgi = 0; sgi < nseg; ++sgi) pair_ok = pair_ok && !ranges_overlap(dx, M, lddx, K, dys[sgi], M, lddy, nper);
    pair_ok = pair_ok && !ranges_overlap(dx, M, lddx, K, x, M, ldx, K);
  }
  if (pair_ok) {
    const int mode = gemm_mode();
    const bool al = al16(dy0) && al16(dy1) && al16(dy2) && al16(x) && al16(w0) && al16(w1) && al16(w2);
    const BwdShape b = {M, nseg, nper, K, lddy, ldx, ldw, lddx, depi, al, wp0 != nullptr, db0 != nullptr, mode};
    GemmArgs gw = wgrad_args(M, nseg, nper, K, lddy, ldx, wws);
    gw.a = mkseg(dy0, dy1, dy2);
    gw.b = mkseg(x, nullptr, nullptr);
    GemmArgs gd = dgrad_shape_args(b, dx, wp0, plane_stride);
    gd.a = mkseg(dy0, dy1, dy2);
    gd.b = mkseg(w0, w1, w2);
    gd.pre_in = pre;
    gd.thr = gct_drop_threshold(p); gd.keep_scale = 1.0f / (1.0f - p); gd.rng = gct_rng_make(seed, site);
    gd.quad_map = quad_map;
    gd.pre_rows = quad_map ? pre_rows : 0;
    const BwdPairPlan r = plan_bwd_pair(b, gw, gd, wws_bytes, dws, dws ? dws_bytes : 0);
    if (r.paired) {
      if (tile_list && tile_count) { gw.kt_list = tile_list; gw.kt_count = tile_count; }
      float* bslab = nullptr;
      if (db0) {
        int64_t off = (int64_t)gw.nsplit * gw.slab_stride;
        off = (off + 3) / 4 * 4;
        bslab = wws + off;                  // [nsplit][Ntot] right behind the weight slabs, as in gct_linear_wgrad
        gw.bias_slab = bslab;
      }
      const bool x3 = mode == GCT_GEMM_BF16X3;
      const int rc = x3 ? launch_x6_pair<2>(gw, gd, st) : launch_x6_pair<3>(gw, gd, st);
      if (rc) return rc;
      if (!x3) g_gemm_launches[1] += 2;     // two GEMM problems, one kernel launch
      const int64_t Ntot = (int64_t)nseg * nper;
      if (bslab)
        return gct_reduce_slabs_seg2(wws, gw.nsplit, gw.slab_stride, dw0, dw1, dw2, (int64_t)nper * K, Ntot * K, bslab,
                                     Ntot, db0, db1, db2, nper, Ntot, st);
      return gct_reduce_slabs_seg(wws, gw.nsplit, gw.slab_stride, dw0, dw1, dw2, (int64_t)nper * K, Ntot * K, st);
    }
  }
  // not paired: today's two calls, unchanged (they check their own arguments)
  int rc = gct_linear_wgrad(dy0, dy1, dy2, lddy, M, nseg, nper, x, ldx, K, dw0, dw1, dw2, lddw, db0, db1, db2, wws,
                            tile_list, tile_count, stream);
  if (rc) return rc;
  return gct_linear_dgrad(dy0, dy1, dy2, lddy, M, nseg, nper, w0, w1, w2, ldw, wp0, plane_stride, K, dx, lddx, depi,
                          pre, p, seed, site, dws, dws_bytes, quad_map, pre_rows, stream);
}

// ---- cross-attention K | V straight from the latent (ABI 32) ------------------------------------------------------
// The decoder memory is e = z W_z^T + b_z and, without cond2lat rows, feeds nothing but the k_linear | v_linear
// projections of the decoder layers: kvb_l = e W_kv,l^T + b_kv,l = z A_l^T + c_l with A_l = W_kv,l W_z and
// c_l = W_kv,l b_z + b_kv,l.  The row-sized GEMMs then reduce over the latent width instead of d_model, and the
// weight-sized products below carry the gradients back to W_kv,l, W_z and b_z.
namespace {

struct KvFoldTab {
  const float* w[2 * GCT_KV_FOLD_MAX_LAYERS];      // segment 2 l: k_linear.weight of layer l, 2 l + 1: v_linear.weight
  const float* b[2 * GCT_KV_FOLD_MAX_LAYERS];
};

// one wave per weight row r of the stack (4 rows per workgroup, all of one segment: d % 4 == 0):
// wstack[r][:] = W_seg[r % d][:], c[r] = W_seg[r % d][:] . bz + b_seg[r % d]
__global__ __launch_bounds__(256) void kv_fold_stack_kernel(const KvFoldTab t, int d, int dm, const float* __restrict__ bz,
                                                            float* __restrict__ wstack, float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int64_t r0 = (int64_t)blockIdx.x * 4;
  const int seg = (int)(r0 / d);                     // uniform over the workgroup: the table entry is a scalar load
  const int64_t i = r0 % d + (threadIdx.x >> 6);
  const float* src = t.w[seg] + i * dm;
  float* dst = wstack + (r0 + (threadIdx.x >> 6)) * dm;
  float acc = 0.f;
  for (int k = lane * 4; k < dm; k += 256) {
    const float4 v = *reinterpret_cast<const float4*>(src + k);
    const float4 z = *reinterpret_cast<const float4*>(bz + k);
    *reinterpret_cast<float4*>(dst + k) = v;
    acc = fmaf(v.x, z.x, acc); acc = fmaf(v.y, z.y, acc); acc = fmaf(v.z, z.z, acc); acc = fmaf(v.w, z.w, acc);
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  const float* b = t.b[seg];
  if (lane == 0) c[r0 + (threadIdx.x >> 6)] = acc + (b ? b[i] : 0.f);
}

// dW[m][n] = sum_k P[m][k] W_z[n][k] + s[m] b_z[n] for the 2 d rows m of one layer (rows < d to dw0, the others to
// dw1), db = s: fp32 fma chains over the latent width, 64 x 64 outputs per workgroup, 4 x 4 per thread
constexpr int KVF_T = 64, KVF_K = 32, KVF_LD = KVF_T + 4;
__global__ __launch_bounds__(256) void kv_fold_wgrad_kernel(const float* __restrict__ p, const float* __restrict__ s, int d,
                                                            int lat, const float* __restrict__ wz,
                                                            const float* __restrict__ bz, int dm, float* __restrict__ dw0,
                                                            float* __restrict__ dw1, float* __restrict__ db0,
                                                            float* __restrict__ db1) {
  __shared__ float as[KVF_K][KVF_LD], bs[KVF_K][KVF_LD];
  const int tid = threadIdx.x, tm = tid >> 4, tn = tid & 15;
  const int m0 = blockIdx.x * KVF_T, n0 = blockIdx.y * KVF_T, M = 2 * d;
  float acc[4][4] = {};
  // 64 rows x 8 float4 of each operand per K-chunk, two per thread: the next chunk is in flight while this one is used
  float4 ra[2], rb[2];
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + i * 256, row = e >> 3, k = (e & 7) * 4;       // lat % 4 == 0: a float4 is inside or outside
    ra[i] = (k < lat && m0 + row < M) ? *reinterpret_cast<const float4*>(p + (int64_t)(m0 + row) * lat + k) : zero4;
    rb[i] = (k < lat && n0 + row < dm) ? *reinterpret_cast<const float4*>(wz + (int64_t)(n0 + row) * lat + k) : zero4;
  }
  for (int k0 = 0; k0 < lat; k0 += KVF_K) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {                              // k-major in LDS
      const int e = tid + i * 256, row = e >> 3, kk = (e & 7) * 4;
      as[kk][row] = ra[i].x; as[kk + 1][row] = ra[i].y; as[kk + 2][row] = ra[i].z; as[kk + 3][row] = ra[i].w;
      bs[kk][row] = rb[i].x; bs[kk + 1][row] = rb[i].y; bs[kk + 2][row] = rb[i].z; bs[kk + 3][row] = rb[i].w;
    }
    __syncthreads();
    if (k0 + KVF_K < lat) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = tid + i * 256, row = e >> 3, k = k0 + KVF_K + (e & 7) * 4;
        ra[i] = (k < lat && m0 + row < M) ? *reinterpret_cast<const float4*>(p + (int64_t)(m0 + row) * lat + k) : zero4;
        rb[i] = (k < lat && n0 + row < dm) ? *reinterpret_cast<const float4*>(wz + (int64_t)(n0 + row) * lat + k) : zero4;
      }
    }
#pragma unroll 8
    for (int k = 0; k < KVF_K; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(&as[k][tm * 4]);
      const float4 b = *reinterpret_cast<const float4*>(&bs[k][tn * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  const int n = n0 + tn * 4;
  if (n >= dm) return;                                        // dm % 4 == 0: the four columns are inside together
  const float4 z = *reinterpret_cast<const float4*>(bz + n);
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tm * 4 + i;
    if (m >= M) break;
    const float sm = s[m];
    float* dst = (m < d ? dw0 + (int64_t)m * dm : dw1 + (int64_t)(m - d) * dm) + n;
    const float4 o = {fmaf(sm, z.x, acc[i][0]), fmaf(sm, z.y, acc[i][1]), fmaf(sm, z.z, acc[i][2]),
                      fmaf(sm, z.w, acc[i][3])};
    *reinterpret_cast<float4*>(dst) = o;
    if (blockIdx.y == 0 && tn == 0) (m < d ? db0 + m : db1 + (m - d))[0] = sm;
  }
}

// db_z[n] = sum_r wstack[r][n] s[r] in two deterministic stages: partial sums of 32 rows, then their sum in a fixed order
constexpr int KVF_ROWS = 32;
__global__ __launch_bounds__(256) void kv_fold_dbz_part_kernel(const float* __restrict__ wstack, const float* __restrict__ s,
                                                               int64_t rows, int dm, float* __restrict__ part) {
  const int n = blockIdx.y * 256 + threadIdx.x;
  if (n >= dm) return;
  const int64_t r0 = (int64_t)blockIdx.x * KVF_ROWS, r1 = r0 + KVF_ROWS < rows ? r0 + KVF_ROWS : rows;
  float acc = 0.f;
#pragma unroll 8
  for (int64_t r = r0; r < r1; ++r) acc = fmaf(wstack[r * dm + n], s[r], acc);
  part[(int64_t)blockIdx.x * dm + n] = acc;
}
__global__ __launch_bounds__(256) void kv_fold_dbz_sum_kernel(const float* __restrict__ part, int nparts, int dm,
                                                              float* __restrict__ dbz) {
  __shared__ float sh[8][32];                          // 32 columns per workgroup, the parts dealt to 8 lanes each
  const int c = threadIdx.x & 31, lane = threadIdx.x >> 5, n = blockIdx.x * 32 + c;
  float acc = 0.f;
  if (n < dm)
    for (int i = lane; i < nparts; i += 8) acc += part[(int64_t)i * dm + n];
  sh[lane][c] = acc;
  __syncthreads();
  if (lane == 0 && n < dm) {
    float t = sh[0][c];
    for (int j = 1; j < 8; ++j) t += sh[j][c];
    dbz[n] = t;
  }
}

}  // namespace

extern "C" int64_t gct_kv_fold_ws_bytes(int layers, int d, int dm, int lat) {
  const int64_t rows = (int64_t)layers * 2 * d;
  const int64_t g = gct_linear_dgrad_ws_bytes(rows, dm, lat);
  const int64_t parts = ((rows + KVF_ROWS - 1) / KVF_ROWS) * dm * (int64_t)sizeof(float) + 256;
  return g > parts ? g : parts;
}

extern "C" int gct_kv_fold_fwd(int layers, const int64_t* w_addrs, const int64_t* b_addrs, int d, int dm,
                               const float* wz, const uint16_t* wzp, int64_t wz_plane_stride, const float* bz, int lat,
                               float* wstack, float* a, float* c, uint16_t* a_planes, int64_t a_plane_stride,
                               float* ws, int64_t ws_bytes, void* stream) {
  GCT_CHECK_ARG(layers >= 1 && layers <= GCT_KV_FOLD_MAX_LAYERS && w_addrs && wz && bz && wstack && a && c,
                "kv_fold_fwd: bad args (1 .. %d layers)", GCT_KV_FOLD_MAX_LAYERS);
  GCT_CHECK_ARG(d > 0 && d % 4 == 0 && dm > 0 && dm % 4 == 0 && lat > 0 && lat % 4 == 0,
                "kv_fold_fwd: d, d_model and the latent width must be multiples of 4");
  GCT_CHECK_ARG(gct_aligned16(wz) && gct_aligned16(bz) && gct_aligned16(wstack) && gct_aligned16(a),
                "kv_fold_fwd: buffers must be 16-byte aligned");
  KvFoldTab t = {};
  for (int i = 0; i < 2 * layers; ++i) {
    t.w[i] = reinterpret_cast<const float*>((uintptr_t)w_addrs[i]);
    t.b[i] = b_addrs ? reinterpret_cast<const float*>((uintptr_t)b_addrs[i]) : nullptr;
    GCT_CHECK_ARG(t.w[i] && gct_aligned16(t.w[i]), "kv_fold_fwd: weight %d missing or not 16-byte aligned", i);
  }
  const int64_t rows = (int64_t)layers * 2 * d;
  hipLaunchKernelGGL(kv_fold_stack_kernel, dim3((unsigned)(rows / 4)), dim3(256), 0, (hipStream_t)stream, t, d, dm, bz,
                     wstack, c);
  GCT_LAUNCH_CHECK("kv_fold_stack");
  // A = wstack W_z: the dgrad form (rows of wstack against the natural [d_model][latent] weight and its planes)
  int rc = gct_linear_dgrad(wstack, nullptr, nullptr, dm, rows, 1, dm, wz, nullptr, nullptr, lat, wzp, wz_plane_stride,
                            lat, a, lat, GCT_DEPI_STORE, nullptr, 0.f, 0, 0, ws, ws ? ws_bytes : 0, nullptr, 0, stream);
  if (rc || !a_planes) return rc;
  return gct_split_planes(a, rows * lat, a_planes, a_plane_stride, stream);
}

extern "C" int gct_kv_fold_wgrad(const float* p, const float* s, int d, int lat, const float* wz, const float* bz,
                                 int dm, float* dw0, float* dw1, float* db0, float* db1, void* stream) {
  GCT_CHECK_ARG(p && s && wz && bz && dw0 && dw1 && db0 && db1 && d > 0 && lat > 0 && lat % 4 == 0 && dm > 0 &&
                    dm % 4 == 0,
                "kv_fold_wgrad: bad args (latent width and d_model must be multiples of 4)");
  GCT_CHECK_ARG(gct_aligned16(p) && gct_aligned16(wz) && gct_aligned16(bz) && gct_aligned16(dw0) && gct_aligned16(dw1),
                "kv_fold_wgrad: buffers must be 16-byte aligned");
  const dim3 grid((unsigned)((2 * d + KVF_T - 1) / KVF_T), (unsigned)((dm + KVF_T - 1) / KVF_T));
  hipLaunchKernelGGL(kv_fold_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, s, d, lat, wz, bz, dm, dw0, dw1,
                     db0, db1);
  GCT_LAUNCH_CHECK("kv_fold_wgrad");
  return GCT_OK;
}

extern "C" int gct_kv_fold_dbz(const float* wstack, const float* s, int64_t rows, int dm, float* dbz, float* ws,
                               int64_t ws_bytes, void* stream) {
  GCT_CHECK_ARG(wstack && s && dbz && ws && rows > 0 && dm > 0, "kv_fold_dbz: bad args");
  const int64_t parts = (rows + KVF_ROWS - 1) / KVF_ROWS;
  GCT_CHECK_ARG(parts * dm * (int64_t)sizeof(float) <= ws_bytes && parts <= INT_MAX,
                "kv_fold_dbz: workspace of %lld B < %lld B", (long long)ws_bytes,
                (long long)(parts * dm * (int64_t)sizeof(float)));
  hipLaunchKernelGGL(kv_fold_dbz_part_kernel, dim3((unsigned)parts, (unsigned)((dm + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, wstack, s, rows, dm, ws);
  GCT_LAUNCH_CHECK("kv_fold_dbz_part");
  hipLaunchKernelGGL(kv_fold_dbz_sum_kernel, dim3((unsigned)((dm + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, (int)parts, dm, dbz);
  GCT_LAUNCH_CHECK("kv_fold_dbz_sum");
  return GCT_OK;
}
