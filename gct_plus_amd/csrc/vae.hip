// K6: VAE reparameterisation and KL term.
// Reference: Model/sublayers.py:14-20, Model/cvaetf.py:63-69 (z = eps*exp(0.5*log_var) + mu);
// Train/trainer1.py:23 (KLD = -0.5*sum(1 + lv - mu^2 - exp(lv)) over ALL elements, padded
// source positions included).  HBM-bound elementwise kernels; sums are two-stage, fixed order.
//
// Per-dimension KL (gct_kld_dims_fwd / gct_kld_dims_bwd / gct_latent_moments; the rule: include/gctplus_hip.h).
// mu and log_var are [R][D] rows.  L = D / 4 lanes read one row as float4, so a 256-thread workgroup covers
// RPP = 256 / L whole rows per pass (threads past RPP * L idle) and there are P = ceil(R / RPP) passes.
// Grid rule: G = min(GCT_KLD_DIMS_MAX_GRID, ceil(P / 4)) workgroups, a function of (R, D) alone; workgroup b takes the
// passes b, b + G, b + 2G, ... -- so a thread meets its rows in ascending order -- and keeps fp64 sums per dimension.
// The RPP row groups of a workgroup are added through LDS in ascending order, one fp64 partial per (quantity,
// workgroup, dimension) goes to ws [Q][G][D], and a single-workgroup launch adds the G partials of a dimension in a
// fixed order (dims_reduce_partials).  No atomics: the same bytes give the same result.
#include <math.h>

#include "common.h"

namespace {

__device__ __forceinline__ float u01(uint32_t x) {  // (0,1]
  return ((float)(x >> 8) + 1.0f) * (1.0f / 16777216.0f);
}

__global__ __launch_bounds__(256) void reparam_fwd_kernel(const float* mu, const float* lv,
                                                          const float* eps_in, float* eps_out,
                                                          float* z, int64_t n, GctRng rng) {
  const int64_t n4 = (n + 3) / 4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    float e[4];
    if (eps_in) {
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = (i * 4 + j < n) ? eps_in[i * 4 + j] : 0.f;
    } else {
      const uint4 r = gct_philox(rng, (uint32_t)i, (uint32_t)(i >> 32), 0x13198A2Eu, 0x03707344u);
      const float r0 = sqrtf(-2.0f * logf(u01(r.x))), r1 = sqrtf(-2.0f * logf(u01(r.z)));
      float s0, c0, s1, c1;
      sincosf(6.283185307179586f * u01(r.y), &s0, &c0);
      sincosf(6.283185307179586f * u01(r.w), &s1, &c1);
      e[0] = r0 * c0; e[1] = r0 * s0; e[2] = r1 * c1; e[3] = r1 * s1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t k = i * 4 + j;
      if (k < n) {
        eps_out[k] = e[j];
        z[k] = e[j] * expf(0.5f * lv[k]) + mu[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void reparam_bwd_kernel(const float* dz, const float* lv,
                                                          const float* eps, const float* dmu_ext,
                                                          const float* dlv_ext, float* dmu,
                                                          float* dlv, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const float g = dz[i];
    float a = g, b = 0.5f * g * eps[i] * expf(0.5f * lv[i]);
    if (dmu_ext) a += dmu_ext[i];
    if (dlv_ext) b += dlv_ext[i];
    dmu[i] = a;
    dlv[i] = b;
  }
}

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
  v = gct_wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// The two expressions of the KL term, each written once: every kernel that sums or differentiates it calls these.
__device__ __forceinline__ float kld_term(float m, float l) { return 1.0f + l - m * m - expf(l); }
__device__ __forceinline__ float kld_dmu(float g, float m) { return g * m; }
__device__ __forceinline__ float kld_dlv(float g, float l) { return g * 0.5f * (expf(l) - 1.0f); }

__global__ __launch_bounds__(256) void kld_partial_kernel(const float* mu, const float* lv,
                                                          float* ws, int64_t n) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    acc += kld_term(mu[i], lv[i]);
  }
  const float t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void final_sum_kernel(const float* ws, int n, float scale,
                                                        float* out) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) acc += ws[i];
  const float t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) out[0] = t * scale;
}

__global__ __launch_bounds__(256) void kld_bwd_kernel(const float* mu, const float* lv,
                                                      const float* gout, float* dmu, float* dlv,
                                                      int64_t n) {
  const float g = gout[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    dmu[i] = kld_dmu(g, mu[i]);
    dlv[i] = kld_dlv(g, lv[i]);
  }
}

// ------------------------------------------------------------------------------------ per-dimension KL
#define GCT_KLD_DIMS_MAX_GRID 512
constexpr int kDimsFinishThreads = 1024;         // >= GCT_LATENT_MAX_DIM: one thread per dimension in the last launch

// Quantities per dimension.  Forward: sum of t, live rows.  Moments: sum mu, sum mu^2, sum exp(lv), sum lv, sum of t,
// live rows (acc's row order).  The row count is carried per dimension like the sums, so one code path serves all.
template <bool MOMENTS> struct DimsQ { static constexpr int n = MOMENTS ? 6 : 2, t = MOMENTS ? 4 : 0, rows = n - 1; };

template <bool MOMENTS>
__global__ __launch_bounds__(256) void kld_dims_partial_kernel(const float* __restrict__ mu,
                                                               const float* __restrict__ lv,
                                                               const uint8_t* __restrict__ live, int64_t R, int D,
                                                               double* __restrict__ ws) {
  constexpr int NQ = DimsQ<MOMENTS>::n, QT = DimsQ<MOMENTS>::t, QR = DimsQ<MOMENTS>::rows;
  __shared__ double sh[1024];                    // [RPP][D] with RPP * D <= 256 * 4
  const int L = D >> 2, rpp = 256 / L;
  const int tid = threadIdx.x, rg = tid / L, lane = tid - rg * L;
  const bool active = rg < rpp;
  double acc[NQ][4];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[q][c] = 0.0;
  if (active) {
    const int64_t step = (int64_t)gridDim.x * rpp;
    for (int64_t r = (int64_t)blockIdx.x * rpp + rg; r < R; r += step) {
      if (live && !live[r]) continue;
      const float4 m4 = reinterpret_cast<const float4*>(mu + r * D)[lane];
      const float4 l4 = reinterpret_cast<const float4*>(lv + r * D)[lane];
      const float m[4] = {m4.x, m4.y, m4.z, m4.w}, l[4] = {l4.x, l4.y, l4.z, l4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[QT][c] += (double)kld_term(m[c], l[c]);
        acc[QR][c] += 1.0;
        if constexpr (MOMENTS) {
          const double md = (double)m[c];
          acc[0][c] += md;
          acc[1][c] += md * md;                  // exact in fp64: a product of two fp32 values
          acc[2][c] += (double)expf(l[c]);
          acc[3][c] += (double)l[c];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (active) {
#pragma unroll
      for (int c = 0; c < 4; ++c) sh[tid * 4 + c] = acc[q][c];      // == sh[rg * D + lane * 4 + c]
    }
    __syncthreads();
    for (int j = tid; j < D; j += 256) {
      double s = sh[j];
      for (int g = 1; g < rpp; ++g) s += sh[g * D + j];
      ws[((int64_t)q * gridDim.x + blockIdx.x) * D + j] = s;
    }
    __syncthreads();
  }
}

// One workgroup of kDimsFinishThreads.  The G partials of quantity q are split into S = 1024 / D contiguous slices;
// thread (s, j) adds slice s of dimension j in ascending workgroup order, and the S slice sums of a dimension are
// added in ascending order.  The result is valid on the threads j < D (s == 0).  sh: kDimsFinishThreads doubles.
__device__ __forceinline__ double dims_reduce_partials(const double* __restrict__ ws, int q, int G, int D, double* sh) {
  const int tid = threadIdx.x, S = kDimsFinishThreads / D, per = (G + S - 1) / S;
  const int s = tid / D, j = tid - s * D;
  double a = 0.0;
  if (s < S) {
    const int g1 = min(G, (s + 1) * per);
    const double* p = ws + (int64_t)q * G * D + j;
    for (int g = s * per; g < g1; ++g) a += p[(int64_t)g * D];
  }
  __syncthreads();                               // sh may still be read by the previous call
  sh[tid] = a;
  __syncthreads();
  double t = 0.0;
  if (tid < D)
    for (int k = 0; k < S; ++k) t += sh[k * D + tid];
  return t;
}

// The kDimsFinishThreads lanes' values in a fixed order (butterfly inside a wave, waves 0..15 in turn), on every thread.
__device__ __forceinline__ double dims_block_sum(double v, double* sh16) {
  v = gct_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh16[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kDimsFinishThreads / 64; ++w) t += sh16[w];
  return t;
}

__global__ __launch_bounds__(kDimsFinishThreads) void kld_dims_finish_kernel(const double* __restrict__ ws, int G,
                                                                             int D, float free_bits, int n_mol,
                                                                             float* __restrict__ out,
                                                                             float* __restrict__ kl_dim,
                                                                             float* __restrict__ gate) {
  __shared__ double sh[kDimsFinishThreads];
  __shared__ double sh16[kDimsFinishThreads / 64];
  const int j = threadIdx.x;
  const double tsum = dims_reduce_partials(ws, DimsQ<false>::t, G, D, sh);
  const double rows = dims_reduce_partials(ws, DimsQ<false>::rows, G, D, sh);
  const double floor_ = (double)free_bits * (double)n_mol;
  double obj = 0.0, raw = 0.0, nfl = 0.0, nrow = 0.0;
  if (j < D) {
    const double K = 0.0 - 0.5 * tsum;           // (no rows: +0, not -0)
    const bool open = K > floor_;                // strict, in fp64, before any rounding
    kl_dim[j] = (float)K;
    gate[j] = open ? 1.0f : 0.0f;
    obj = open ? K : floor_;
    raw = K;
    nfl = open ? 0.0 : 1.0;
    if (j == 0) nrow = rows;
  }
  obj = dims_block_sum(obj, sh16);
  raw = dims_block_sum(raw, sh16);
  nfl = dims_block_sum(nfl, sh16);
  nrow = dims_block_sum(nrow, sh16);
  if (j == 0) {
    out[0] = (float)obj;
    out[1] = (float)raw;
    out[2] = (float)nfl;
    out[3] = (float)nrow;
  }
}

__global__ __launch_bounds__(kDimsFinishThreads) void latent_moments_finish_kernel(const double* __restrict__ ws, int G,
                                                                                   int D, double* __restrict__ acc) {
  __shared__ double sh[kDimsFinishThreads];
  for (int q = 0; q < DimsQ<true>::n; ++q) {
    const double t = dims_reduce_partials(ws, q, G, D, sh);
    if ((int)threadIdx.x < D) acc[q * D + threadIdx.x] += (q == DimsQ<true>::t) ? -0.5 * t : t;
  }
}

__global__ __launch_bounds__(256) void kld_dims_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                           const uint8_t* __restrict__ live,
                                                           const float* __restrict__ gate,
                                                           const float* __restrict__ gout, float* __restrict__ dmu,
                                                           float* __restrict__ dlv, int64_t n4, int L) {
  const float g = gout[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / L;
    const int q = (int)(i - r * L);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (!live || live[r]) {
      const float4 gt = reinterpret_cast<const float4*>(gate)[q];
      const float4 m = reinterpret_cast<const float4*>(mu)[i], l = reinterpret_cast<const float4*>(lv)[i];
      if (gt.x != 0.f) { a.x = kld_dmu(g, m.x); b.x = kld_dlv(g, l.x); }
      if (gt.y != 0.f) { a.y = kld_dmu(g, m.y); b.y = kld_dlv(g, l.y); }
      if (gt.z != 0.f) { a.z = kld_dmu(g, m.z); b.z = kld_dlv(g, l.z); }
      if (gt.w != 0.f) { a.w = kld_dmu(g, m.w); b.w = kld_dlv(g, l.w); }
    }
    reinterpret_cast<float4*>(dmu)[i] = a;
    reinterpret_cast<float4*>(dlv)[i] = b;
  }
}

// the grid rule of the header comment; 0 when there is no row
int kld_dims_grid(int64_t R, int D) {
  if (R <= 0) return 0;
  const int64_t rpp = 256 / (D / 4), passes = (R + rpp - 1) / rpp, g = (passes + 3) / 4;
  return (int)(g > GCT_KLD_DIMS_MAX_GRID ? GCT_KLD_DIMS_MAX_GRID : g);
}

bool kld_dims_dim_ok(int D) { return D >= 4 && D <= GCT_LATENT_MAX_DIM && D % 4 == 0; }

template <bool MOMENTS>
int kld_dims_partials(const float* mu, const float* lv, const uint8_t* live, int64_t R, int D, double* ws,
                      hipStream_t st) {
  const int G = kld_dims_grid(R, D);
  if (G > 0) {
    hipLaunchKernelGGL(kld_dims_partial_kernel<MOMENTS>, dim3((unsigned)G), dim3(256), 0, st, mu, lv, live, R, D, ws);
    GCT_LAUNCH_CHECK(MOMENTS ? "latent_moments" : "kld_dims_fwd");
  }
  return GCT_OK;
}

inline unsigned grid_for(int64_t n, int64_t cap) {
  int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

int gct_final_sum(const float* ws, int n, float scale, float* out, hipStream_t st) {
  hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(256), 0, st, ws, n, scale, out);
  GCT_LAUNCH_CHECK("final_sum");
  return GCT_OK;
}

extern "C" int gct_reparam_fwd(const float* mu, const float* log_var, const float* eps_in,
                               float* eps_out, float* z, int64_t n, uint64_t seed, uint32_t site,
                               void* stream) {
  GCT_CHECK_ARG(mu && log_var && eps_out && z && n >= 0, "reparam_fwd: bad args");
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3(grid_for((n + 3) / 4, 4096)), dim3(256), 0,
                     (hipStream_t)stream, mu, log_var, eps_in, eps_out, z, n,
                     gct_rng_make(seed, site));
  GCT_LAUNCH_CHECK("reparam_fwd");
  return GCT_OK;
}

extern "C" int gct_reparam_bwd(const float* dz, const float* log_var, const float* eps,
                               const float* dmu_ext, const float* dlv_ext, float* dmu, float* dlv,
                               int64_t n, void* stream) {
  GCT_CHECK_ARG(dz && log_var && eps && dmu && dlv && n >= 0, "reparam_bwd: bad args");
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(reparam_bwd_kernel, dim3(grid_for(n, 4096)), dim3(256), 0,
                     (hipStream_t)stream, dz, log_var, eps, dmu_ext, dlv_ext, dmu, dlv, n);
  GCT_LAUNCH_CHECK("reparam_bwd");
  return GCT_OK;
}

extern "C" int gct_kld_fwd(const float* mu, const float* log_var, float* out, float* ws, int64_t n,
                           void* stream) {
  GCT_CHECK_ARG(mu && log_var && out && ws && n >= 0, "kld_fwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = grid_for(n, 1024);
  hipLaunchKernelGGL(kld_partial_kernel, dim3(g), dim3(256), 0, st, mu, log_var, ws, n);
  GCT_LAUNCH_CHECK("kld_partial");
  return gct_final_sum(ws, (int)g, -0.5f, out, st);
}

extern "C" int gct_kld_bwd(const float* mu, const float* log_var, const float* gout, float* dmu,
                           float* dlv, int64_t n, void* stream) {
  GCT_CHECK_ARG(mu && log_var && gout && dmu && dlv && n >= 0, "kld_bwd: bad args");
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(kld_bwd_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, (hipStream_t)stream,
                     mu, log_var, gout, dmu, dlv, n);
  GCT_LAUNCH_CHECK("kld_bwd");
  return GCT_OK;
}

extern "C" int64_t gct_kld_dims_ws_bytes(int D) {
  if (!kld_dims_dim_ok(D)) return 0;
  return (int64_t)DimsQ<true>::n * GCT_KLD_DIMS_MAX_GRID * D * (int64_t)sizeof(double);
}

extern "C" int gct_kld_dims_fwd(const float* mu, const float* log_var, const uint8_t* live, int64_t R, int D,
                                float free_bits, int n_mol, float* out, float* kl_dim, float* gate, void* ws,
                                void* stream) {
  GCT_CHECK_ARG(kld_dims_dim_ok(D), "kld_dims_fwd: D must be a multiple of 4 in [4, %d]", GCT_LATENT_MAX_DIM);
  GCT_CHECK_ARG(R >= 0 && n_mol >= 1 && (R == 0 || (mu && log_var)) && out && kl_dim && gate && ws,
                "kld_dims_fwd: bad args");
  GCT_CHECK_ARG(isfinite(free_bits) && free_bits >= 0.0f, "kld_dims_fwd: free_bits must be a finite number >= 0");
  GCT_CHECK_ARG(gct_aligned16(mu) && gct_aligned16(log_var) && gct_aligned16(out) && gct_aligned16(kl_dim) &&
                    gct_aligned16(gate) && gct_aligned16(ws),
                "kld_dims_fwd: mu, log_var, out, kl_dim, gate and ws must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  const int rc = kld_dims_partials<false>(mu, log_var, live, R, D, (double*)ws, st);
  if (rc != GCT_OK) return rc;
  hipLaunchKernelGGL(kld_dims_finish_kernel, dim3(1), dim3(kDimsFinishThreads), 0, st, (const double*)ws,
                     kld_dims_grid(R, D), D, free_bits, n_mol, out, kl_dim, gate);
  GCT_LAUNCH_CHECK("kld_dims_fwd (finish)");
  return GCT_OK;
}

extern "C" int gct_kld_dims_bwd(const float* mu, const float* log_var, const uint8_t* live, const float* gate,
                                const float* gout, float* dmu, float* dlv, int64_t R, int D, void* stream) {
  GCT_CHECK_ARG(kld_dims_dim_ok(D), "kld_dims_bwd: D must be a multiple of 4 in [4, %d]", GCT_LATENT_MAX_DIM);
  GCT_CHECK_ARG(R >= 0 && gate && gout && (R == 0 || (mu && log_var && dmu && dlv)), "kld_dims_bwd: bad args");
  GCT_CHECK_ARG(gct_aligned16(mu) && gct_aligned16(log_var) && gct_aligned16(gate) && gct_aligned16(dmu) &&
                    gct_aligned16(dlv) && (((uintptr_t)gout) & 3u) == 0,
                "kld_dims_bwd: mu, log_var, gate, dmu and dlv must be 16-B aligned");
  if (R == 0) return GCT_OK;
  const int64_t n4 = R * (D / 4);
  hipLaunchKernelGGL(kld_dims_bwd_kernel, dim3(grid_for(n4, 4096)), dim3(256), 0, (hipStream_t)stream, mu, log_var,
                     live, gate, gout, dmu, dlv, n4, D / 4);
  GCT_LAUNCH_CHECK("kld_dims_bwd");
  return GCT_OK;
}

extern "C" int gct_latent_moments(const float* mu, const float* log_var, const uint8_t* live, int64_t R, int D,
                                  double* acc, void* ws, void* stream) {
  GCT_CHECK_ARG(kld_dims_dim_ok(D), "latent_moments: D must be a multiple of 4 in [4, %d]", GCT_LATENT_MAX_DIM);
  GCT_CHECK_ARG(R >= 0 && (R == 0 || (mu && log_var)) && acc && ws, "latent_moments: bad args");
  GCT_CHECK_ARG(gct_aligned16(mu) && gct_aligned16(log_var) && gct_aligned16(acc) && gct_aligned16(ws),
                "latent_moments: mu, log_var, acc and ws must be 16-B aligned");
  if (R == 0) return GCT_OK;                       // nothing to add
  hipStream_t st = (hipStream_t)stream;
  const int rc = kld_dims_partials<true>(mu, log_var, live, R, D, (double*)ws, st);
  if (rc != GCT_OK) return rc;
  hipLaunchKernelGGL(latent_moments_finish_kernel, dim3(1), dim3(kDimsFinishThreads), 0, st, (const double*)ws,
                     kld_dims_grid(R, D), D, acc);
  GCT_LAUNCH_CHECK("latent_moments (finish)");
  return GCT_OK;
}
