// K8: fused Adam over one flat fp32 buffer.
// Reference: torch.optim.Adam as configured in train1.py:116-119 (betas (0.9,0.98), eps 1e-9,
// no weight decay, no amsgrad); step arithmetic follows torch's single-tensor path:
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   denom = sqrt(v)/sqrt(1-b2^t) + eps ; p -= (lr/(1-b1^t)) * m/denom
// HBM-bound: 16 B read + 12 B written per parameter.  Grid: ceil(n / 4 / 256) workgroups, capped at 8192.
//
// Global gradient-norm clipping (torch.nn.utils.clip_grad_norm_'s rule, on the device):
//   gct_grad_norm         sum of squares of the flat gradient in fp64 -> norm, coef and running counters in an
//                         8-word device state (layout: include/gctplus_hip.h); 4 B read per parameter.
//                         Pass 1: ceil(n / 4 / 256) workgroups of 256, capped at GCT_GRAD_NORM_MAX_GRID = 2048, each
//                         lane 4 float4 loads in flight per trip of a grid-stride loop, one fp64 partial per workgroup
//                         into the caller's slab.  Pass 2: ONE workgroup sums the slab in a fixed order and one lane
//                         writes the state.  No atomics: the same buffer gives the same bits on every run and rank.
//                         The loads keep the default cache policy: the Adam launch behind the pass then finds g in
//                         the Infinity Cache (README: the pair costs the same with non-temporal loads).
//   gct_adam_step         given that state: the step above on (g * gscale) * coef, skipped when the state says
//                         "non-finite".
// Both Adam launches are instantiations of ONE kernel template, adam_kernel<ClipState...>: the update arithmetic has
// one source with every rounding written out.  The instantiation without a state (adam_kernel<>, launched when no
// state is given) has the argument list of the kernel before the clipped one existed and computes the same bits; with
// coef == 1 the clipped instantiation computes them too.
#include <math.h>

#include "common.h"

#define GCT_GRAD_NORM_MAX_GRID 2048

namespace {
// ClipState: empty (no clipping), or one `const float*`, the state gct_grad_norm wrote
template <typename... ClipState>
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v,
                                                   int64_t n4, int64_t n, float b1, float b2,
                                                   float eps, float step_size, float inv_bc2_sqrt,
                                                   float gscale, const int32_t* __restrict__ skip_if_nonzero,
                                                   ClipState... clip_state) {
  // Every rounding of the update is written out: with contraction left to the compiler, the two instantiations (and
  // two builds) fused different products of a sum.  The forms are those the kernel compiled to before the clipped
  // instantiation existed, so that an unclipped step stays what it was bit for bit -- which is why the scalar tail
  // (at most 3 elements of a call) rounds m and v differently from the float4 path.
#pragma clang fp contract(off)
  constexpr bool CLIP = sizeof...(ClipState) != 0;
  static_assert(sizeof...(ClipState) <= 1, "at most one clipping state");
  if (skip_if_nonzero && *skip_if_nonzero != 0) return;     // a gradient landed where none may (see the header)
  float coef = 1.0f;
  if constexpr (CLIP) {
    const float* state = (clip_state, ...);
    if (reinterpret_cast<const int32_t*>(state)[2] != 0) return;        // non-finite norm: p, m, v stay as they are
    coef = state[1];
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i * 4;
    if (e + 3 < n) {
      float4 pp = *reinterpret_cast<float4*>(p + e);
      float4 gg = *reinterpret_cast<const float4*>(g + e);
      float4 mm = *reinterpret_cast<float4*>(m + e);
      float4 vv = *reinterpret_cast<float4*>(v + e);
      float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gr = CLIP ? (G[j] * gscale) * coef : G[j] * gscale;
        M[j] = fmaf(b1, M[j], (1.0f - b1) * gr);
        V[j] = fmaf(gr, (1.0f - b2) * gr, b2 * V[j]);
        P[j] = fmaf(-step_size, M[j] / fmaf(sqrtf(V[j]), inv_bc2_sqrt, eps), P[j]);
      }
      *reinterpret_cast<float4*>(p + e) = pp;
      *reinterpret_cast<float4*>(m + e) = mm;
      *reinterpret_cast<float4*>(v + e) = vv;
    } else {
      for (int64_t k = e; k < n; ++k) {
        const float gr = CLIP ? (g[k] * gscale) * coef : g[k] * gscale;
        const float mk = fmaf(1.0f - b1, gr, b1 * m[k]);            // the tail's own roundings, see above
        const float vk = b2 * v[k] + ((1.0f - b2) * gr) * gr;
        m[k] = mk; v[k] = vk;
        p[k] = fmaf(-step_size, mk / fmaf(sqrtf(vk), inv_bc2_sqrt, eps), p[k]);
      }
    }
  }
}

// ---------------------------------------------------------------- gradient norm
__device__ __forceinline__ double sumsq4(double acc, float4 x) {
  acc = fma((double)x.x, (double)x.x, acc);
  acc = fma((double)x.y, (double)x.y, acc);
  acc = fma((double)x.z, (double)x.z, acc);
  return fma((double)x.w, (double)x.w, acc);
}

// the 256 lanes' values summed in a fixed order (butterfly inside a wave, waves 0..3 in turn); valid on thread 0
__device__ __forceinline__ double block_sum_256(double acc, double* lds) {
  acc = gct_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// partial[blockIdx.x] = sum of g[k]^2 over this workgroup's share of the nq whole float4s; workgroup 0 also takes the
// n - 4 * nq < 4 elements behind them.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t nq, int64_t n,
                                                         double* __restrict__ partial) {
  __shared__ double lds[4];
  const float4* g4 = reinterpret_cast<const float4*>(g);
  const int64_t stride = (int64_t)gridDim.x * 256;
  double acc = 0.0;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < nq; i += 4 * stride) {            // four independent 16-B loads in flight per lane
    const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    acc = sumsq4(sumsq4(sumsq4(sumsq4(acc, a), b), c), d);
  }
  for (; i < nq; i += stride) acc = sumsq4(acc, g4[i]);
  if (blockIdx.x == 0) {
    const int64_t k = nq * 4 + threadIdx.x;                 // scalar tail: n % 4 elements
    if (k < n) acc = fma((double)g[k], (double)g[k], acc);
  }
  acc = block_sum_256(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// One workgroup: the nblk partials in a fixed order, then the state (layout: include/gctplus_hip.h), from one lane.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ partial, int nblk,
                                                               float gscale, float max_norm, float* state) {
  __shared__ double lds[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
  acc = block_sum_256(acc, lds);
  if (threadIdx.x != 0) return;
  const double norm_d = fabs((double)gscale) * sqrt(acc);
  const float norm = (float)norm_d;                          // beyond fp32's range: inf, and the step is skipped
  const bool finite = isfinite(norm);
  const double coef_d = fmin(1.0, (double)max_norm / (norm_d + 1e-6));
  const float coef = finite ? (float)coef_d : 0.0f;
  int32_t* si = reinterpret_cast<int32_t*>(state);
  state[0] = norm;
  state[1] = coef;
  si[2] = finite ? 0 : 1;
  si[3] = si[3] + 1;
  si[4] = si[4] + ((finite && coef < 1.0f) ? 1 : 0);
  si[5] = si[5] + (finite ? 0 : 1);
  if (finite) state[6] = fmaxf(state[6], norm);
  si[7] = 0;
}

int grad_norm_grid(int64_t n) {
  if (n <= 0) return 0;
  const int64_t nq = n / 4;
  int64_t grid = (nq + 255) / 256;
  if (grid < 1) grid = 1;
  if (grid > GCT_GRAD_NORM_MAX_GRID) grid = GCT_GRAD_NORM_MAX_GRID;
  return (int)grid;
}
}  // namespace

extern "C" int gct_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                             float b1, float b2, float eps, int64_t step, float gscale,
                             const int32_t* skip_if_nonzero, const float* clip_state, void* stream) {
  GCT_CHECK_ARG(p && g && m && v && n >= 0 && step >= 1, "adam_step: bad args");
  GCT_CHECK_ARG(gct_aligned16(p) && gct_aligned16(g) && gct_aligned16(m) && gct_aligned16(v),
                "adam_step: buffers must be 16-B aligned");
  GCT_CHECK_ARG((((uintptr_t)clip_state) & 3u) == 0, "adam_step: clip_state must be 4-B aligned");
  if (n == 0) return GCT_OK;
  const double bc1 = 1.0 - pow((double)b1, (double)step);
  const double bc2 = 1.0 - pow((double)b2, (double)step);
  const float step_size = (float)((double)lr / bc1);
  const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
  const int64_t n4 = (n + 3) / 4;
  int64_t grid = (n4 + 255) / 256;
  if (grid > 8192) grid = 8192;
  if (clip_state)
    hipLaunchKernelGGL(adam_kernel<const float*>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m,
                       v, n4, n, b1, b2, eps, step_size, inv_bc2_sqrt, gscale, skip_if_nonzero, clip_state);
  else
    hipLaunchKernelGGL(adam_kernel<>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p, g, m,
                       v, n4, n, b1, b2, eps, step_size, inv_bc2_sqrt, gscale, skip_if_nonzero);
  GCT_LAUNCH_CHECK("adam_step");
  return GCT_OK;
}

extern "C" int64_t gct_grad_norm_ws_bytes(int64_t n) {
  const int64_t b = (int64_t)grad_norm_grid(n) * (int64_t)sizeof(double);
  return b < 16 ? 16 : (b + 15) / 16 * 16;
}

extern "C" int gct_grad_norm(const float* g, int64_t n, float gscale, float max_norm, float* state, void* ws,
                             void* stream) {
  GCT_CHECK_ARG(n >= 0 && (g || n == 0) && state && ws, "grad_norm: bad args");
  GCT_CHECK_ARG(gct_aligned16(g) && gct_aligned16(state) && gct_aligned16(ws),
                "grad_norm: g, state and ws must be 16-B aligned");
  GCT_CHECK_ARG(max_norm > 0.0f && isfinite(max_norm), "grad_norm: max_norm must be a finite number > 0");
  const int grid = grad_norm_grid(n);
  double* partial = (double*)ws;
  if (grid > 0) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, g, n / 4, n,
                       partial);
    GCT_LAUNCH_CHECK("grad_norm");
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, grid, gscale,
                     max_norm, state);
  GCT_LAUNCH_CHECK("grad_norm (finish)");
  return GCT_OK;
}
