// K12: latents for interpolation between molecules (Inference/mol_interpolation.py:124-141, 216-224 of the reference).
// gct_latent_stats: per-molecule, per-dimension mean and unbiased standard deviation of mu and log_var over the molecule's
// own latent rows (approximate_z's fit).  gct_latent_interp: one wave per (row, token) draws the two endpoints' latents
// from those fits, slerps them over the D dimensions and adds the retry ladder's noise.  include/gctplus_hip.h states
// the rules (random streams, guard, limits); nothing here depends on the grid, and there are no atomics.
// K13: importance-weighted marginal likelihoods.  gct_latent_iw: K posterior draws per molecule, each latent written
// once together with log p(z) - log q(z | x) of the draw; gct_iw_combine: the bound, the ELBO and the effective sample
// size of a molecule's K log-weights in fp64, one wave per molecule.
#include "common.h"

namespace {

__device__ __forceinline__ float u01(uint32_t x) {  // (0,1]: the u01 of vae.hip
  return ((float)(x >> 8) + 1.0f) * (1.0f / 16777216.0f);
}

// 4 standard normals of one Philox call: Box-Muller on (x, y) and (z, w), as reparam_fwd_kernel
__device__ __forceinline__ void normals4(uint4 r, float e[4]) {
  const float r0 = sqrtf(-2.0f * logf(u01(r.x))), r1 = sqrtf(-2.0f * logf(u01(r.z)));
  float s0, c0, s1, c1;
  sincosf(6.283185307179586f * u01(r.y), &s0, &c0);
  sincosf(6.283185307179586f * u01(r.w), &s1, &c1);
  e[0] = r0 * c0; e[1] = r0 * s0; e[2] = r1 * c1; e[3] = r1 * s1;
}

// thread = (molecule, which of mu / log_var, dimension): rows in ascending order, the mean first, then the squared
// deviations.  Lanes walk d, so every row is read coalesced.
__global__ __launch_bounds__(256) void latent_stats_kernel(const float* mu, const float* lv, const int32_t* rows,
                                                           int Le, int D, float* stats) {
  const int d = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y, which = blockIdx.z;
  if (d >= D) return;
  int nr = rows[i];
  nr = nr < 1 ? 1 : (nr > Le ? Le : nr);             // the wrapper checks 1 <= rows <= Le; never read outside the molecule
  const float* x = (which ? lv : mu) + (int64_t)i * Le * D + d;
  float s = 0.f;
  for (int l = 0; l < nr; ++l) s += x[(int64_t)l * D];
  const float mean = s / (float)nr;
  float q = 0.f;
  for (int l = 0; l < nr; ++l) {
    const float t = x[(int64_t)l * D] - mean;
    q += t * t;
  }
  float* o = stats + ((int64_t)i * 4 + 2 * which) * D + d;
  o[0] = mean;
  o[D] = nr > 1 ? sqrtf(q / (float)(nr - 1)) : 0.f;
}

constexpr int kMaxQ = GCT_LATENT_MAX_DIM / 4 / 64;   // quads of 4 dimensions per lane: 4

// slerp weights of (u, v) from their wave-wide dot products; false: the guard (lerp)
__device__ __forceinline__ bool slerp_weights(float uu, float vv, float uv, float alpha, float& wu, float& wv) {
  if (uu == 0.f || vv == 0.f) return false;
  const float c = uv / (sqrtf(uu) * sqrtf(vv));
  if (!(fabsf(c) <= GCT_LATENT_SLERP_MAX_COS)) return false;
  const float w = acosf(c), sw = sinf(w);
  wu = sinf((1.0f - alpha) * w) / sw;
  wv = sinf(alpha * w) / sw;
  return true;
}

// fit[k]: the 4 dimensions of quad j of statistic k of molecule m
__device__ __forceinline__ void load_fit(const float* stats, int m, int D, int j, float fit[4][4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d = 4 * j + e;
      fit[k][e] = d < D ? stats[((int64_t)m * 4 + k) * D + d] : 0.f;
    }
}

__global__ __launch_bounds__(256) void latent_interp_kernel(const float* stats, int n, int D, const int32_t* a,
                                                            const int32_t* b, const float* alpha,
                                                            const float* noise_std, const int32_t* len,
                                                            const int32_t* item, int64_t R, int T, float* z,
                                                            GctRng rng) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // wave = (r, t)
  if (w >= R * (int64_t)T) return;
  const int64_t r = w / T;
  const int t = (int)(w - r * T);
  float* zr = z + w * D;
  const int nq = (D + 3) >> 2;
  const int ma = a[r], mb = b[r], lr = len[r];
  // rows outside the limits the wrapper checks are written as zeros: nothing is read through a bad index
  if (t >= lr || ma < 0 || ma >= n || mb < 0 || mb >= n) {
    for (int d = lane; d < D; d += 64) zr[d] = 0.f;
    return;
  }
  const float al = alpha[r], ns = noise_std[r];
  const uint32_t c0 = (uint32_t)item[r], c1 = 8u * (uint32_t)t;
  const bool noisy = ns != 0.f;                       // wave-uniform: the noise-free rungs skip the log_var half

  float u[kMaxQ][4], v[kMaxQ][4], p[kMaxQ][4], q[kMaxQ][4], g[kMaxQ][4];
  float uu = 0.f, vv = 0.f, uv = 0.f, pp = 0.f, qq = 0.f, pq = 0.f;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int j = k * 64 + lane;
    if (j < nq) {
      float fa[4][4], fb[4][4], e[4];
      load_fit(stats, ma, D, j, fa);
      load_fit(stats, mb, D, j, fb);
      normals4(gct_philox(rng, c0, c1 + 0, (uint32_t)j, GCT_LATENT_C3), e);
#pragma unroll
      for (int x = 0; x < 4; ++x) u[k][x] = 4 * j + x < D ? fa[0][x] + fa[1][x] * e[x] : 0.f;
      normals4(gct_philox(rng, c0, c1 + 1, (uint32_t)j, GCT_LATENT_C3), e);
#pragma unroll
      for (int x = 0; x < 4; ++x) v[k][x] = 4 * j + x < D ? fb[0][x] + fb[1][x] * e[x] : 0.f;
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        uu += u[k][x] * u[k][x];
        vv += v[k][x] * v[k][x];
        uv += u[k][x] * v[k][x];
      }
      if (noisy) {
        normals4(gct_philox(rng, c0, c1 + 2, (uint32_t)j, GCT_LATENT_C3), e);
#pragma unroll
        for (int x = 0; x < 4; ++x) p[k][x] = 4 * j + x < D ? fa[2][x] + fa[3][x] * e[x] : 0.f;
        normals4(gct_philox(rng, c0, c1 + 3, (uint32_t)j, GCT_LATENT_C3), e);
#pragma unroll
        for (int x = 0; x < 4; ++x) q[k][x] = 4 * j + x < D ? fb[2][x] + fb[3][x] * e[x] : 0.f;
        normals4(gct_philox(rng, c0, c1 + 4, (uint32_t)j, GCT_LATENT_C3), g[k]);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          pp += p[k][x] * p[k][x];
          qq += q[k][x] * q[k][x];
          pq += p[k][x] * q[k][x];
        }
      }
    }
  }
  uu = gct_wave_sum(uu); vv = gct_wave_sum(vv); uv = gct_wave_sum(uv);
  float mu_u = 0.f, mu_v = 0.f, lv_p = 0.f, lv_q = 0.f;
  const bool m_slerp = slerp_weights(uu, vv, uv, al, mu_u, mu_v);
  bool l_slerp = false;
  if (noisy) {
    pp = gct_wave_sum(pp); qq = gct_wave_sum(qq); pq = gct_wave_sum(pq);
    l_slerp = slerp_weights(pp, qq, pq, al, lv_p, lv_q);
  }
  const bool vec = (D & 3) == 0 && (((uintptr_t)z) & 15u) == 0;
#pragma unroll
  for (int k = 0; k < kMaxQ; ++k) {
    const int j = k * 64 + lane;
    if (j < nq) {
      float o[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        // the guard's lerp as u + alpha (v - u): u == v gives u exactly
        const float m = m_slerp ? mu_u * u[k][x] + mu_v * v[k][x] : u[k][x] + al * (v[k][x] - u[k][x]);
        if (noisy) {
          const float l = l_slerp ? lv_p * p[k][x] + lv_q * q[k][x] : p[k][x] + al * (q[k][x] - p[k][x]);
          o[x] = m + ns * g[k][x] * expf(0.5f * l);
        } else {
          o[x] = m;
        }
      }
      if (vec) {
        *reinterpret_cast<float4*>(zr + 4 * j) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (4 * j + x < D) zr[4 * j + x] = o[x];
      }
    }
  }
}

// K13: one workgroup per output row r = (molecule i, draw k), walking the row's quads q = t * nq + j in steps of 256:
// consecutive work-items take consecutive quads, so every load and store of a wave is one contiguous run.  A quad
// costs one Philox call and one Box-Muller; z (and eps) are written once and nothing is read back.  The terms go into a
// per-work-item fp64 sum in ascending q, then the butterfly and the four waves: the order the header states.
__global__ __launch_bounds__(256) void latent_iw_kernel(const float* mu, const float* lv, const int32_t* rows,
                                                        const int32_t* item, int Le, int D, int k0, int Kc,
                                                        int64_t R, float* z, float* logw, float* eps_out, GctRng rng) {
  __shared__ double sh[4];
  const int tid = threadIdx.x, nq = (D + 3) >> 2;
  const int dt = 256 / nq, dj = 256 % nq;             // one step of 256 quads in (t, j)
  const bool vec = (D & 3) == 0 && ((((uintptr_t)mu) | ((uintptr_t)lv) | ((uintptr_t)z) | ((uintptr_t)eps_out)) & 15u) == 0;
  for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
    const int i = (int)(r / Kc);
    const uint32_t c0 = (uint32_t)item[i], c1 = (uint32_t)(k0 + (int)(r - (int64_t)i * Kc));
    int nr = rows[i];
    nr = nr < 1 ? 1 : (nr > Le ? Le : nr);            // the wrapper checks 1 <= rows <= Le; never read outside the molecule
    const float* mi = mu + (int64_t)i * Le * D;
    const float* li = lv + (int64_t)i * Le * D;
    float* zr = z + r * Le * D;
    float* er = eps_out ? eps_out + r * Le * D : nullptr;
    double acc = 0.0;
    int t = tid / nq, j = tid - t * nq;
    while (t < Le) {
      const int64_t off = (int64_t)t * D + 4 * j;
      float o[4] = {0.f, 0.f, 0.f, 0.f}, e[4] = {0.f, 0.f, 0.f, 0.f};
      if (t < nr) {
        float m[4], l[4];
        if (vec) {
          const float4 mv = *reinterpret_cast<const float4*>(mi + off), lq = *reinterpret_cast<const float4*>(li + off);
          m[0] = mv.x; m[1] = mv.y; m[2] = mv.z; m[3] = mv.w;
          l[0] = lq.x; l[1] = lq.y; l[2] = lq.z; l[3] = lq.w;
        } else {
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const bool in = 4 * j + x < D;
            m[x] = in ? mi[off + x] : 0.f;
            l[x] = in ? li[off + x] : 0.f;
          }
        }
        normals4(gct_philox(rng, c0, c1, 256u * (uint32_t)t + (uint32_t)j, GCT_IW_C3), e);
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (4 * j + x < D) {
            o[x] = fmaf(e[x], expf(0.5f * l[x]), m[x]);
            acc += (double)(0.5f * fmaf(e[x] - o[x], e[x] + o[x], l[x]));
          }
      }
      if (vec) {
        *reinterpret_cast<float4*>(zr + off) = make_float4(o[0], o[1], o[2], o[3]);
        if (er) *reinterpret_cast<float4*>(er + off) = make_float4(e[0], e[1], e[2], e[3]);
      } else {
#pragma unroll
        for (int x = 0; x < 4; ++x)
          if (4 * j + x < D) {
            zr[off + x] = o[x];
            if (er) er[off + x] = e[x];
          }
      }
      j += dj;
      t += dt;
      if (j >= nq) { j -= nq; ++t; }
    }
    acc = gct_wave_sum(acc);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) logw[r] = (float)((sh[0] + sh[1]) + (sh[2] + sh[3]));
    __syncthreads();                                  // sh is the next row's too
  }
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// one wave per molecule: lane l holds k = l, l + 64, ...; everything in fp64, one rounding per output
__global__ __launch_bounds__(256) void iw_combine_kernel(const float* logp, const float* logw, int n, int K,
                                                         float* iwae, float* elbo, float* recon, float* ess) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const float* p = logp + i * K;
  const float* w = logw + i * K;
  double m = -INFINITY, sa = 0.0, sp = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double a = (double)p[k] + (double)w[k];
    m = fmax(m, a);
    sa += a;
    sp += (double)p[k];
  }
  m = wave_max_f64(m);
  sa = gct_wave_sum(sa);
  sp = gct_wave_sum(sp);
  const double shift = m == -INFINITY ? 0.0 : m;      // every weight zero: iwae = -inf, not NaN
  double s1 = 0.0, s2 = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double e = exp(((double)p[k] + (double)w[k]) - shift);
    s1 += e;
    s2 += e * e;
  }
  s1 = gct_wave_sum(s1);
  s2 = gct_wave_sum(s2);
  if (lane == 0) {
    iwae[i] = (float)(shift + log(s1) - log((double)K));
    elbo[i] = (float)(sa / (double)K);
    recon[i] = (float)(sp / (double)K);
    ess[i] = (float)(s1 * s1 / s2);
  }
}

}  // namespace

extern "C" int gct_latent_iw(const float* mu, const float* log_var, int n, int Le, int D, const int32_t* rows,
                             const int32_t* item, int k0, int Kc, float* z, float* logw, float* eps_out,
                             uint64_t seed, void* stream) {
  GCT_CHECK_ARG(D >= 1 && D <= GCT_LATENT_MAX_DIM, "latent_iw: D=%d outside [1, %d]", D, GCT_LATENT_MAX_DIM);
  GCT_CHECK_ARG(Le >= 1 && Le <= (1 << 24) && n >= 0, "latent_iw: bad Le=%d (1..2^24) or n=%d", Le, n);
  GCT_CHECK_ARG(k0 >= 0 && Kc >= 0 && (int64_t)k0 + Kc <= 2147483647ll, "latent_iw: bad draw range k0=%d, Kc=%d", k0, Kc);
  const int64_t R = (int64_t)n * Kc;
  GCT_CHECK_ARG(R * Le <= ((int64_t)1 << 25), "latent_iw: n * Kc * Le = %lld rows of z exceed 2^25", (long long)(R * Le));
  if (R == 0) return GCT_OK;
  GCT_CHECK_ARG(mu && log_var && rows && item && z && logw, "latent_iw: null pointer");
  const int64_t cap = (int64_t)1 << 20;               // workgroups; a larger batch walks several rows per workgroup
  hipLaunchKernelGGL(latent_iw_kernel, dim3((unsigned)(R < cap ? R : cap)), dim3(256), 0, (hipStream_t)stream, mu,
                     log_var, rows, item, Le, D, k0, Kc, R, z, logw, eps_out, gct_rng_make(seed, GCT_IW_SITE));
  GCT_LAUNCH_CHECK("latent_iw");
  return GCT_OK;
}

extern "C" int gct_iw_combine(const float* logp, const float* logw, int n, int K, float* iwae, float* elbo,
                              float* recon, float* ess, void* stream) {
  GCT_CHECK_ARG(n >= 0 && K >= 1 && (int64_t)n * K <= 2147483647ll, "iw_combine: bad n=%d or K=%d", n, K);
  if (n == 0) return GCT_OK;
  GCT_CHECK_ARG(logp && logw && iwae && elbo && recon && ess, "iw_combine: null pointer");
  hipLaunchKernelGGL(iw_combine_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logp, logw,
                     n, K, iwae, elbo, recon, ess);
  GCT_LAUNCH_CHECK("iw_combine");
  return GCT_OK;
}

extern "C" int gct_latent_stats(const float* mu, const float* log_var, int n, int Le, int D, const int32_t* rows,
                                float* stats, void* stream) {
  GCT_CHECK_ARG(mu && log_var && rows && stats, "latent_stats: null pointer");
  GCT_CHECK_ARG(n >= 0 && n <= 65535 && Le >= 1, "latent_stats: bad n=%d (0..65535) or Le=%d", n, Le);
  GCT_CHECK_ARG(D >= 1 && D <= GCT_LATENT_MAX_DIM, "latent_stats: D=%d outside [1, %d]", D, GCT_LATENT_MAX_DIM);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(latent_stats_kernel, dim3((D + 255) / 256, n, 2), dim3(256), 0, (hipStream_t)stream, mu,
                     log_var, rows, Le, D, stats);
  GCT_LAUNCH_CHECK("latent_stats");
  return GCT_OK;
}

extern "C" int gct_latent_interp(const float* stats, int n, int D, const int32_t* a, const int32_t* b,
                                 const float* alpha, const float* noise_std, const int32_t* len,
                                 const int32_t* item, int64_t R, int T, float* z, uint64_t seed, void* stream) {
  GCT_CHECK_ARG(D >= 1 && D <= GCT_LATENT_MAX_DIM, "latent_interp: D=%d outside [1, %d]", D, GCT_LATENT_MAX_DIM);
  GCT_CHECK_ARG(R >= 0 && T >= 1 && n >= 1, "latent_interp: bad R=%lld, T=%d or n=%d", (long long)R, T, n);
  if (R == 0) return GCT_OK;
  GCT_CHECK_ARG(stats && a && b && alpha && noise_std && len && item && z, "latent_interp: null pointer");
  const int64_t waves = R * (int64_t)T;
  GCT_CHECK_ARG(waves <= ((int64_t)1 << 25), "latent_interp: R * T = %lld rows of z exceed 2^25", (long long)waves);
  hipLaunchKernelGGL(latent_interp_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                     stats, n, D, a, b, alpha, noise_std, len, item, R, T, z, gct_rng_make(seed, GCT_LATENT_SITE));
  GCT_LAUNCH_CHECK("latent_interp");
  return GCT_OK;
}
