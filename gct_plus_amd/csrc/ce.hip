// K7: final-vocabulary cross-entropy.
// Reference: Train/trainer1.py:21-22  F.cross_entropy(logits.view(-1,V), ys,
// ignore_index=pad, reduction='sum').  V <= 31 in practice: one wave per row (row = 120 B),
// wave-level max / sum-exp; per-block partial sums reduced in fixed order.
// Log-likelihoods (decode.py score_reference states the rule): gct_seq_logp scores given token rows against their
// teacher-forced logits, gct_chosen_logp the token a decode step has just picked.  Both go through wave_token_logp, the
// same wave-per-row log-softmax; every output has one writer and a fixed summation order (no atomics).
// gct_seq_logp_bwd (decode.py seq_logp_grad_reference states the rule) is gct_seq_logp's gradient with respect to the
// logits: ce_grad_row, the row arithmetic of gct_ce_bwd, with a weight per token column instead of one scalar.
// gct_seq_dist / gct_seq_dist_bwd (decode.py dist_reference / dist_grad_reference state the rules) are the entropy of
// the next-token distribution and its KL divergence from a second model's, per scored token and per sequence, and their
// gradient with respect to the first model's logits: the same layouts, around wave_row_dist.
// gct_seq_ppo / gct_seq_ppo_bwd (decode.py ppo_reference / ppo_grad_reference state the rules) are PPO's clipped
// surrogate of each scored token's probability ratio against the log-probabilities it was sampled with, per token and
// per sequence, and its gradient with respect to the logits: the same layouts again, wave_token_logp and ce_grad_write
// around ppo_token.
#include "common.h"
#include "decode_rows.h"

int gct_final_sum(const float* ws, int n, float scale, float* out, hipStream_t st);

namespace {

__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits,
                                                     const int64_t* __restrict__ target, float* ws,
                                                     int64_t rows, int V, int64_t pad_id) {
  __shared__ float sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t t = target[row];
    if (t == pad_id) continue;  // wave-uniform
    const float* lr = logits + row * V;
    float mx, se;
    gct_wave_softmax_stats(lr, V, lane, mx, se);
    if (lane == 0 && t >= 0 && t < V) acc += (mx + logf(se)) - lr[t];
  }
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// One wave, one logits row lr[0, V) whose softmax statistics (mx, se) the caller holds:
// dr[c] = g * (softmax(lr)[c] - [c == t]).  The one place where this arithmetic is written: gct_ce_bwd, gct_seq_logp_bwd
// and gct_seq_ppo_bwd give the same bits for the same row, target and weight.
__device__ __forceinline__ void ce_grad_write(const float* lr, float* dr, int V, int64_t t, float g, int lane, float mx,
                                              float se) {
  const float inv = 1.0f / se;
  for (int c = lane; c < V; c += 64) {
    float pr = expf(lr[c] - mx) * inv;
    if (c == t) pr -= 1.0f;
    dr[c] = g * pr;
  }
}

// ce_grad_write behind the row's own statistics.
__device__ __forceinline__ void ce_grad_row(const float* lr, float* dr, int V, int64_t t, float g, int lane) {
  float mx, se;
  gct_wave_softmax_stats(lr, V, lane, mx, se);
  ce_grad_write(lr, dr, V, t, g, lane, mx, se);
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits,
                                                     const int64_t* __restrict__ target,
                                                     const float* gout, float* dlogits,
                                                     int64_t rows, int V, int64_t pad_id) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float g = gout[0];
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t t = target[row];
    const float* lr = logits + row * V;
    float* dr = dlogits + row * V;
    if (t == pad_id) {
      for (int c = lane; c < V; c += 64) dr[c] = 0.f;
      continue;
    }
    ce_grad_row(lr, dr, V, t, g, lane);
  }
}

// One wave, one logits row lr[0, V), 0 <= tok < V (uniform over the wave): returns x[tok] - m - log(sum exp(x - m)) on
// every lane; hit = tok is the FIRST maximum of the row (torch.argmax).
__device__ __forceinline__ float wave_token_logp(const float* __restrict__ lr, int V, int tok, int lane, bool& hit) {
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, lr[c]);
  mx = gct_wave_max(mx);
  float se = 0.f;
  int first = 0x7fffffff;                               // lowest index that holds the maximum
  for (int c = lane; c < V; c += 64) {
    const float x = lr[c];
    se += expf(x - mx);
    if (x == mx && c < first) first = c;
  }
  se = gct_wave_sum(se);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  hit = first == tok;
  return (lr[tok] - mx) - logf(se);
}

constexpr int SEQ_LOGP_MAX_W = 256;

// one workgroup per sequence; wave w takes the token columns w, w + 4, ...  Each column's log-probability and flags
// go to LDS, and thread 0 adds them up in ascending column order: the sums do not depend on the grid or on which wave
// took a column.
__global__ __launch_bounds__(256) void seq_logp_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                       int64_t rows_per_seq, int row_shift,
                                                       const int64_t* __restrict__ ys, int64_t ld_ys,
                                                       const int32_t* __restrict__ prefix_lens, int64_t pad_id, int W,
                                                       float* __restrict__ token_logp, int64_t ld_out,
                                                       float* __restrict__ logp, int32_t* __restrict__ tokens,
                                                       int32_t* __restrict__ hits) {
  __shared__ float sh_lp[SEQ_LOGP_MAX_W];
  __shared__ uint8_t sh_flag[SEQ_LOGP_MAX_W];           // bit 0: scored, bit 1: hit
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int t0 = prefix_lens ? prefix_lens[r] : 1;
  const int64_t* yr = ys + r * ld_ys;
  for (int c = wave; c < W; c += 4) {                   // uniform over the wave
    const int64_t tok = yr[c];
    const bool scored = c >= t0 && c >= 1 && tok != pad_id && tok >= 0 && tok < V;
    float lp = 0.f;
    bool hit = false;
    if (scored) lp = wave_token_logp(logits + (r * rows_per_seq + row_shift + c - 1) * ld, V, (int)tok, lane, hit);
    if (lane == 0) {
      token_logp[r * ld_out + c] = lp;
      sh_lp[c] = lp;
      sh_flag[c] = (scored ? 1 : 0) | (hit ? 2 : 0);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
    int nt = 0, nh = 0;
    for (int c = 0; c < W; ++c) {
      const int f = sh_flag[c];
      if (f & 1) sum += sh_lp[c];
      nt += f & 1;
      nh += (f >> 1) & 1;
    }
    logp[r] = sum;
    tokens[r] = nt;
    hits[r] = nh;
  }
}

// one wave per logits row (r, j), four rows per workgroup, the grid strides over the rest (ce_bwd_kernel's layout).
// Row j of sequence r predicts token column c = j - row_shift + 1 and is scored under seq_logp_kernel's predicate; its
// weight is g = g_logp[r] + g_token[r][c] (a null table: 0).  A row that is not scored, or whose weight is 0, gets V
// exact zeros and its logits are NOT read (the decoder may never have computed them).  Everything a branch depends on
// is one value per wave.
__global__ __launch_bounds__(256) void seq_logp_bwd_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                           int64_t rows_per_seq, int row_shift,
                                                           const int64_t* __restrict__ ys, int64_t ld_ys,
                                                           const int32_t* __restrict__ prefix_lens, int64_t pad_id,
                                                           int W, const float* __restrict__ g_logp,
                                                           const float* __restrict__ g_token, int64_t ld_g,
                                                           float* __restrict__ dlogits, int64_t ld_d, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t r = row / rows_per_seq, j = row - r * rows_per_seq;
    const int64_t c = j - row_shift + 1;
    float* dr = dlogits + row * ld_d;
    int64_t tok = 0;
    float g = 0.f;
    if (j >= row_shift && c >= 1 && c < W) {
      const int t0 = prefix_lens ? prefix_lens[r] : 1;
      tok = ys[r * ld_ys + c];
      if (c >= t0 && tok != pad_id && tok >= 0 && tok < V)
        g = (g_logp ? g_logp[r] : 0.f) + (g_token ? g_token[r * ld_g + c] : 0.f);
    }
    if (g == 0.f) {                                     // not scored, or a zero weight
      for (int v = lane; v < V; v += 64) dr[v] = 0.f;
      continue;
    }
    ce_grad_row(logits + row * ld, dr, V, tok, -g, lane);
  }
}

// The clipped surrogate of one scored token (decode.py ppo_reference states the rule): lp its log-probability now, old
// the one it was sampled with, A its sequence's advantage.  rho = exp(lp - old); CLIPPED when A > 0 and rho > 1 +
// clip_hi, or A < 0 and rho < 1 - clip_lo (strict: rho == 1 never is).  Plain fp32, one value per wave.
struct PpoToken {
  float rho, surrogate, k3;
  bool clipped;
};
__device__ __forceinline__ PpoToken ppo_token(float lp, float old, float A, float clip_lo, float clip_hi) {
  PpoToken t;
  const float d = lp - old, hi = 1.0f + clip_hi, lo = 1.0f - clip_lo;
  t.rho = expf(d);
  const bool up = A > 0.f && t.rho > hi, down = A < 0.f && t.rho < lo;
  t.clipped = up || down;
  t.surrogate = up ? A * hi : (down ? A * lo : A * t.rho);
  t.k3 = (t.rho - 1.0f) - d;                            // the k3 estimator term of KL(old || new)
  return t;
}

// seq_logp_kernel's layout: one workgroup per sequence, wave w takes the token columns w, w + 4, ...; each column's
// log-probability (wave_token_logp: gct_seq_logp's bits), surrogate and KL term go to LDS and thread 0 adds them up in
// ascending column order.  Neither the logits row nor old_token_logp is read at a column that is not scored.
__global__ __launch_bounds__(256) void seq_ppo_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                      int64_t rows_per_seq, int row_shift,
                                                      const int64_t* __restrict__ ys, int64_t ld_ys,
                                                      const int32_t* __restrict__ prefix_lens, int64_t pad_id, int W,
                                                      const float* __restrict__ old_token_logp, int64_t ld_old,
                                                      const float* __restrict__ advantage, float clip_lo,
                                                      float clip_hi, float* __restrict__ token_logp,
                                                      float* __restrict__ token_surrogate, int64_t ld_out,
                                                      float* __restrict__ logp, float* __restrict__ surrogate,
                                                      float* __restrict__ approx_kl, int32_t* __restrict__ tokens,
                                                      int32_t* __restrict__ hits, int32_t* __restrict__ clipped) {
  __shared__ float sh_lp[SEQ_LOGP_MAX_W];
  __shared__ float sh_s[SEQ_LOGP_MAX_W];
  __shared__ float sh_k[SEQ_LOGP_MAX_W];
  __shared__ uint8_t sh_flag[SEQ_LOGP_MAX_W];           // bit 0: scored, bit 1: hit, bit 2: clipped
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int t0 = prefix_lens ? prefix_lens[r] : 1;
  const int64_t* yr = ys + r * ld_ys;
  const float A = advantage[r];
  for (int c = wave; c < W; c += 4) {                   // uniform over the wave
    const int64_t tok = yr[c];
    const bool scored = c >= t0 && c >= 1 && tok != pad_id && tok >= 0 && tok < V;
    float lp = 0.f;
    PpoToken t = {1.f, 0.f, 0.f, false};
    bool hit = false;
    if (scored) {
      lp = wave_token_logp(logits + (r * rows_per_seq + row_shift + c - 1) * ld, V, (int)tok, lane, hit);
      t = ppo_token(lp, old_token_logp[r * ld_old + c], A, clip_lo, clip_hi);
    }
    if (lane == 0) {
      token_logp[r * ld_out + c] = lp;
      token_surrogate[r * ld_out + c] = t.surrogate;
      sh_lp[c] = lp;
      sh_s[c] = t.surrogate;
      sh_k[c] = t.k3;
      sh_flag[c] = (scored ? 1 : 0) | (hit ? 2 : 0) | (t.clipped ? 4 : 0);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f, ss = 0.f, sk = 0.f;
    int nt = 0, nh = 0, nc = 0;
    for (int c = 0; c < W; ++c) {
      const int f = sh_flag[c];
      if (f & 1) {
        sum += sh_lp[c];
        ss += sh_s[c];
        sk += sh_k[c];
      }
      nt += f & 1;
      nh += (f >> 1) & 1;
      nc += (f >> 2) & 1;
    }
    logp[r] = sum;
    surrogate[r] = ss;
    approx_kl[r] = sk;
    tokens[r] = nt;
    hits[r] = nh;
    clipped[r] = nc;
  }
}

// seq_logp_bwd_kernel's layout: one wave per logits row (r, j), four rows per workgroup, the grid strides over the
// rest.  With A = advantage[r] and g = g_surrogate[r] + g_token_surrogate[r][c] (a null table: 0), a row that is not
// scored, or whose A or g is 0, gets V exact zeros and its logits are NOT read.  Otherwise the row's softmax statistics
// are taken once: lp (wave_token_logp's bits), rho and the clip decision follow from them, and the row is V zeros
// (clipped) or ce_grad_write with the weight -((g * A) * rho): rho == 1 gives gct_seq_logp_bwd's bits for g_logp =
// g * A.  Everything a branch depends on is one value per wave.
__global__ __launch_bounds__(256) void seq_ppo_bwd_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                          int64_t rows_per_seq, int row_shift,
                                                          const int64_t* __restrict__ ys, int64_t ld_ys,
                                                          const int32_t* __restrict__ prefix_lens, int64_t pad_id,
                                                          int W, const float* __restrict__ old_token_logp,
                                                          int64_t ld_old, const float* __restrict__ advantage,
                                                          float clip_lo, float clip_hi,
                                                          const float* __restrict__ g_surrogate,
                                                          const float* __restrict__ g_token, int64_t ld_g,
                                                          float* __restrict__ dlogits, int64_t ld_d, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t r = row / rows_per_seq, j = row - r * rows_per_seq;
    const int64_t c = j - row_shift + 1;
    float* dr = dlogits + row * ld_d;
    int64_t tok = 0;
    float g = 0.f, A = 0.f;
    if (j >= row_shift && c >= 1 && c < W) {
      const int t0 = prefix_lens ? prefix_lens[r] : 1;
      tok = ys[r * ld_ys + c];
      if (c >= t0 && tok != pad_id && tok >= 0 && tok < V) {
        g = (g_surrogate ? g_surrogate[r] : 0.f) + (g_token ? g_token[r * ld_g + c] : 0.f);
        A = advantage[r];
      }
    }
    bool live = g != 0.f && A != 0.f;                   // scored, and both weights count
    float mx = 0.f, se = 1.f, w = 0.f;
    const float* lr = logits + row * ld;
    if (live) {
      gct_wave_softmax_stats(lr, V, lane, mx, se);
      const float lp = (lr[tok] - mx) - logf(se);
      const PpoToken t = ppo_token(lp, old_token_logp[r * ld_old + c], A, clip_lo, clip_hi);
      live = !t.clipped;
      w = (g * A) * t.rho;
    }
    if (!live) {
      for (int v = lane; v < V; v += 64) dr[v] = 0.f;
      continue;
    }
    ce_grad_write(lr, dr, V, tok, -w, lane, mx, se);
  }
}

// One wave, one logits row lr[0, V) and -- pr non-null -- the prior's row pr[0, V); every lane gets the results.
//   m = max x, lse = log(sum exp(x - m));  H = lse - sum e_v (x_v - m) / se  with e_v = exp(x_v - m), se = sum e_v;
//   KL = sum (e_v / se) ((x_v - m - lse) - (y_v - m' - lse'))  (the primed ones: the same of the prior's row).
// wave_token_logp's numerics: one max pass, one expf pass with a lane-strided V loop, wave sums, logf.  A lane skips
// its term where e_v == 0 (a -inf logit: p_v log p_v -> 0), so p_v > 0 against q_v == 0 is the only way to +inf.
struct RowDist {
  float m, lse, inv, pm, plse, H, KL;
};
__device__ __forceinline__ RowDist wave_row_dist(const float* __restrict__ lr, const float* __restrict__ pr, int V,
                                                 int lane) {
  RowDist d;
  float mx = -INFINITY;
  for (int c = lane; c < V; c += 64) mx = fmaxf(mx, lr[c]);
  d.m = gct_wave_max(mx);
  float se = 0.f, sx = 0.f;
  for (int c = lane; c < V; c += 64) {
    const float y = lr[c] - d.m, e = expf(y);
    se += e;
    if (e != 0.f) sx += e * y;
  }
  se = gct_wave_sum(se);
  sx = gct_wave_sum(sx);
  d.lse = logf(se);
  d.inv = 1.0f / se;
  d.H = d.lse - sx / se;
  d.pm = d.plse = d.KL = 0.f;
  if (pr) {                                             // uniform over the wave
    gct_wave_softmax_stats(pr, V, lane, d.pm, se);
    d.plse = logf(se);
    float kl = 0.f;
    for (int c = lane; c < V; c += 64) {
      const float y = lr[c] - d.m, e = expf(y);
      if (e != 0.f) kl += (e * d.inv) * ((y - d.lse) - ((pr[c] - d.pm) - d.plse));
    }
    d.KL = gct_wave_sum(kl);
  }
  return d;
}

// seq_logp_kernel's layout: one workgroup per sequence, wave w takes the token columns w, w + 4, ...; each column's
// entropy and KL go to LDS and thread 0 adds them up in ascending column order.  Neither model's logits row is read
// at a column that is not scored.
__global__ __launch_bounds__(256) void seq_dist_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                       int64_t rows_per_seq, int row_shift,
                                                       const float* __restrict__ prior, int64_t ld_prior,
                                                       const int64_t* __restrict__ ys, int64_t ld_ys,
                                                       const int32_t* __restrict__ prefix_lens, int64_t pad_id, int W,
                                                       float* __restrict__ token_entropy, int64_t ld_out,
                                                       float* __restrict__ entropy, float* __restrict__ token_kl,
                                                       float* __restrict__ kl) {
  __shared__ float sh_h[SEQ_LOGP_MAX_W];
  __shared__ float sh_kl[SEQ_LOGP_MAX_W];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int t0 = prefix_lens ? prefix_lens[r] : 1;
  const int64_t* yr = ys + r * ld_ys;
  for (int c = wave; c < W; c += 4) {                   // uniform over the wave
    const int64_t tok = yr[c];
    const bool scored = c >= t0 && c >= 1 && tok != pad_id && tok >= 0 && tok < V;
    float h = 0.f, k = 0.f;
    if (scored) {
      const int64_t row = r * rows_per_seq + row_shift + c - 1;
      const RowDist d = wave_row_dist(logits + row * ld, prior ? prior + row * ld_prior : nullptr, V, lane);
      h = d.H;
      k = d.KL;
    }
    if (lane == 0) {
      token_entropy[r * ld_out + c] = h;
      sh_h[c] = h;
      if (prior) {
        token_kl[r * ld_out + c] = k;
        sh_kl[c] = k;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sh = 0.f, sk = 0.f;
    for (int c = 0; c < W; ++c) sh += sh_h[c];          // a column that is not scored holds 0
    entropy[r] = sh;
    if (prior) {
      for (int c = 0; c < W; ++c) sk += sh_kl[c];
      kl[r] = sk;
    }
  }
}

// seq_logp_bwd_kernel's layout: one wave per logits row (r, j), four rows per workgroup, the grid strides over the
// rest.  With a = g_entropy[r] + g_token_entropy[r][c] and b = g_kl[r] + g_token_kl[r][c] (a null table: 0) a scored
// row gets  a * (-p_v (log p_v + H)) + b * (p_v ((log p_v - log q_v) - KL)),  exact zeros where p_v == 0.  A row that
// is not scored, or whose a and b are both 0, gets V exact zeros and neither its logits nor the prior's are read.
// Everything a branch depends on is one value per wave.
__global__ __launch_bounds__(256) void seq_dist_bwd_kernel(const float* __restrict__ logits, int64_t ld, int V,
                                                           int64_t rows_per_seq, int row_shift,
                                                           const float* __restrict__ prior, int64_t ld_prior,
                                                           const int64_t* __restrict__ ys, int64_t ld_ys,
                                                           const int32_t* __restrict__ prefix_lens, int64_t pad_id,
                                                           int W, const float* __restrict__ g_entropy,
                                                           const float* __restrict__ g_token_entropy, int64_t ld_ge,
                                                           const float* __restrict__ g_kl,
                                                           const float* __restrict__ g_token_kl, int64_t ld_gk,
                                                           float* __restrict__ dlogits, int64_t ld_d, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t r = row / rows_per_seq, j = row - r * rows_per_seq;
    const int64_t c = j - row_shift + 1;
    float* dr = dlogits + row * ld_d;
    float a = 0.f, b = 0.f;
    if (j >= row_shift && c >= 1 && c < W) {
      const int t0 = prefix_lens ? prefix_lens[r] : 1;
      const int64_t tok = ys[r * ld_ys + c];
      if (c >= t0 && tok != pad_id && tok >= 0 && tok < V) {
        a = (g_entropy ? g_entropy[r] : 0.f) + (g_token_entropy ? g_token_entropy[r * ld_ge + c] : 0.f);
        b = (g_kl ? g_kl[r] : 0.f) + (g_token_kl ? g_token_kl[r * ld_gk + c] : 0.f);
      }
    }
    if (a == 0.f && b == 0.f) {                         // not scored, or zero weights
      for (int v = lane; v < V; v += 64) dr[v] = 0.f;
      continue;
    }
    const float* lr = logits + row * ld;
    const float* pr = b != 0.f ? prior + row * ld_prior : nullptr;   // b != 0 only with a prior (checked by the host)
    const RowDist d = wave_row_dist(lr, pr, V, lane);
    for (int v = lane; v < V; v += 64) {
      const float y = lr[v] - d.m, e = expf(y);
      float g = 0.f;
      if (e != 0.f) {
        const float p = e * d.inv, lp = y - d.lse;
        g = a * (-p * (lp + d.H));
        if (pr) g += b * (p * ((lp - ((pr[v] - d.pm) - d.plse)) - d.KL));
      }
      dr[v] = g;
    }
  }
}

// one wave per decode row, as select_token_kernel: the column the selection has just written (gct_row_slot)
__global__ __launch_bounds__(256) void chosen_logp_kernel(const float* __restrict__ logits, int V,
                                                          const int64_t* __restrict__ ys, int64_t ld_ys,
                                                          const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ row_off,
                                                          const int32_t* __restrict__ item,
                                                          const int32_t* __restrict__ prefix_len, int64_t pad_id,
                                                          float* __restrict__ out, int64_t ld_out, int out_rows,
                                                          int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= n) return;
  const GctRowSlot s = gct_row_slot(*pos + 1, row, row_off != nullptr, row_off, item != nullptr, item, prefix_len);
  if (!s.acts()) return;                                // parked, or a prefix token: not a generated one (uniform
  const int p = s.pos, dst = s.item;                    // over the wave: a whole wave leaves)
  if (p < 0 || p >= ld_out || p >= ld_ys || dst >= out_rows) return;
  const int64_t tok = ys[(int64_t)row * ld_ys + p];
  float lp = 0.f;
  bool hit = false;
  if (tok != pad_id && tok >= 0 && tok < V) lp = wave_token_logp(logits + (int64_t)row * V, V, (int)tok, lane, hit);
  if (lane == 0) out[(int64_t)dst * ld_out + p] = lp;
}

}  // namespace

extern "C" int gct_ce_fwd(const float* logits, const int64_t* target, float* out, float* ws,
                          int64_t rows, int V, int64_t pad_id, void* stream) {
  GCT_CHECK_ARG(logits && target && out && ws && rows >= 0 && V > 0, "ce_fwd: bad args");
  hipStream_t st = (hipStream_t)stream;
  int64_t g = (rows + 3) / 4;
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)g), dim3(256), 0, st, logits, target, ws, rows,
                     V, pad_id);
  GCT_LAUNCH_CHECK("ce_fwd");
  return gct_final_sum(ws, (int)g, 1.0f, out, st);
}

extern "C" int gct_ce_bwd(const float* logits, const int64_t* target, const float* gout,
                          float* dlogits, int64_t rows, int V, int64_t pad_id, void* stream) {
  GCT_CHECK_ARG(logits && target && gout && dlogits && rows >= 0 && V > 0, "ce_bwd: bad args");
  if (rows == 0) return GCT_OK;
  int64_t g = (rows + 3) / 4;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, logits,
                     target, gout, dlogits, rows, V, pad_id);
  GCT_LAUNCH_CHECK("ce_bwd");
  return GCT_OK;
}

extern "C" int gct_seq_logp(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                            const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                            int W, float* token_logp, int64_t ld_out, float* logp, int32_t* tokens, int32_t* hits,
                            void* stream) {
  GCT_CHECK_ARG(logits && ys && token_logp && logp && tokens && hits, "seq_logp: null pointer");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V, "seq_logp: bad shape (n %d, V %d, ld %lld)", n, V, (long long)ld);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_logp: rows of %d tokens (1 .. %d supported)", W, SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && ld_out >= W, "seq_logp: ld_ys / ld_out narrower than the %d token columns", W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_logp: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift, W - 1);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(seq_logp_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, logits, ld, V,
                     rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W, token_logp, ld_out, logp, tokens, hits);
  GCT_LAUNCH_CHECK("seq_logp");
  return GCT_OK;
}

extern "C" int gct_seq_logp_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                                const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                                int W, const float* g_logp, const float* g_token, int64_t ld_g, float* dlogits,
                                int64_t ld_d, void* stream) {
  GCT_CHECK_ARG(logits && ys && dlogits, "seq_logp_bwd: null pointer");
  GCT_CHECK_ARG(g_logp || g_token, "seq_logp_bwd: both gradients are null (g_logp, g_token)");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V && ld_d >= V, "seq_logp_bwd: bad shape (n %d, V %d, ld %lld, ld_d %lld)", n,
                V, (long long)ld, (long long)ld_d);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_logp_bwd: rows of %d tokens (1 .. %d supported)", W,
                SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && (!g_token || ld_g >= W), "seq_logp_bwd: ld_ys / ld_g narrower than the %d token columns",
                W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_logp_bwd: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift,
                W - 1);
  const int64_t rows = (int64_t)n * rows_per_seq;
  if (rows == 0) return GCT_OK;
  int64_t g = (rows + 3) / 4;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(seq_logp_bwd_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, logits, ld, V,
                     rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W, g_logp, g_token, ld_g, dlogits, ld_d,
                     rows);
  GCT_LAUNCH_CHECK("seq_logp_bwd");
  return GCT_OK;
}

extern "C" int gct_seq_ppo(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                           const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W,
                           const float* old_token_logp, int64_t ld_old, const float* advantage, float clip_lo,
                           float clip_hi, float* token_logp, float* token_surrogate, int64_t ld_out, float* logp,
                           float* surrogate, float* approx_kl, int32_t* tokens, int32_t* hits, int32_t* clipped,
                           void* stream) {
  GCT_CHECK_ARG(logits && ys && token_logp && token_surrogate && logp && surrogate && approx_kl && tokens && hits &&
                    clipped,
                "seq_ppo: null pointer");
  GCT_CHECK_ARG(old_token_logp && advantage, "seq_ppo: null pointer (old_token_logp, advantage)");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V, "seq_ppo: bad shape (n %d, V %d, ld %lld)", n, V, (long long)ld);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_ppo: rows of %d tokens (1 .. %d supported)", W, SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && ld_out >= W && ld_old >= W,
                "seq_ppo: ld_ys / ld_out / ld_old narrower than the %d token columns", W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_ppo: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift, W - 1);
  GCT_CHECK_ARG(clip_lo >= 0.f && clip_lo < 1.f && clip_hi >= 0.f,
                "seq_ppo: clip (%g, %g) outside 0 <= clip_lo < 1, clip_hi >= 0", (double)clip_lo, (double)clip_hi);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(seq_ppo_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, logits, ld, V, rows_per_seq,
                     row_shift, ys, ld_ys, prefix_lens, pad_id, W, old_token_logp, ld_old, advantage, clip_lo, clip_hi,
                     token_logp, token_surrogate, ld_out, logp, surrogate, approx_kl, tokens, hits, clipped);
  GCT_LAUNCH_CHECK("seq_ppo");
  return GCT_OK;
}

extern "C" int gct_seq_ppo_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                               const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                               int W, const float* old_token_logp, int64_t ld_old, const float* advantage,
                               float clip_lo, float clip_hi, const float* g_surrogate,
                               const float* g_token_surrogate, int64_t ld_g, float* dlogits, int64_t ld_d,
                               void* stream) {
  GCT_CHECK_ARG(logits && ys && dlogits, "seq_ppo_bwd: null pointer");
  GCT_CHECK_ARG(old_token_logp && advantage, "seq_ppo_bwd: null pointer (old_token_logp, advantage)");
  GCT_CHECK_ARG(g_surrogate || g_token_surrogate,
                "seq_ppo_bwd: both gradients are null (g_surrogate, g_token_surrogate)");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V && ld_d >= V, "seq_ppo_bwd: bad shape (n %d, V %d, ld %lld, ld_d %lld)", n,
                V, (long long)ld, (long long)ld_d);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_ppo_bwd: rows of %d tokens (1 .. %d supported)", W,
                SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && ld_old >= W && (!g_token_surrogate || ld_g >= W),
                "seq_ppo_bwd: ld_ys / ld_old / ld_g narrower than the %d token columns", W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_ppo_bwd: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift,
                W - 1);
  GCT_CHECK_ARG(clip_lo >= 0.f && clip_lo < 1.f && clip_hi >= 0.f,
                "seq_ppo_bwd: clip (%g, %g) outside 0 <= clip_lo < 1, clip_hi >= 0", (double)clip_lo, (double)clip_hi);
  const int64_t rows = (int64_t)n * rows_per_seq;
  if (rows == 0) return GCT_OK;
  int64_t g = (rows + 3) / 4;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(seq_ppo_bwd_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, logits, ld, V,
                     rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W, old_token_logp, ld_old, advantage,
                     clip_lo, clip_hi, g_surrogate, g_token_surrogate, ld_g, dlogits, ld_d, rows);
  GCT_LAUNCH_CHECK("seq_ppo_bwd");
  return GCT_OK;
}

extern "C" int gct_seq_dist(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                            const float* prior_logits, int64_t ld_prior, const int64_t* ys, int64_t ld_ys,
                            const int32_t* prefix_lens, int64_t pad_id, int n, int W, float* token_entropy,
                            int64_t ld_out, float* entropy, float* token_kl, float* kl, void* stream) {
  GCT_CHECK_ARG(logits && ys && token_entropy && entropy, "seq_dist: null pointer");
  GCT_CHECK_ARG(prior_logits || (!token_kl && !kl), "seq_dist: kl outputs without prior logits");
  GCT_CHECK_ARG(!prior_logits || (token_kl && kl), "seq_dist: prior logits without kl outputs (null pointer)");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V && (!prior_logits || ld_prior >= V),
                "seq_dist: bad shape (n %d, V %d, ld %lld, ld_prior %lld)", n, V, (long long)ld, (long long)ld_prior);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_dist: rows of %d tokens (1 .. %d supported)", W, SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && ld_out >= W, "seq_dist: ld_ys / ld_out narrower than the %d token columns", W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_dist: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift,
                W - 1);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(seq_dist_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, logits, ld, V, rows_per_seq,
                     row_shift, prior_logits, ld_prior, ys, ld_ys, prefix_lens, pad_id, W, token_entropy, ld_out,
                     entropy, token_kl, kl);
  GCT_LAUNCH_CHECK("seq_dist");
  return GCT_OK;
}

extern "C" int gct_seq_dist_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                                const float* prior_logits, int64_t ld_prior, const int64_t* ys, int64_t ld_ys,
                                const int32_t* prefix_lens, int64_t pad_id, int n, int W, const float* g_entropy,
                                const float* g_token_entropy, int64_t ld_ge, const float* g_kl,
                                const float* g_token_kl, int64_t ld_gk, float* dlogits, int64_t ld_d, void* stream) {
  GCT_CHECK_ARG(logits && ys && dlogits, "seq_dist_bwd: null pointer");
  GCT_CHECK_ARG(g_entropy || g_token_entropy || g_kl || g_token_kl,
                "seq_dist_bwd: all four gradients are null (g_entropy, g_token_entropy, g_kl, g_token_kl)");
  GCT_CHECK_ARG(prior_logits || (!g_kl && !g_token_kl), "seq_dist_bwd: kl gradients without prior logits");
  GCT_CHECK_ARG(n >= 0 && V > 0 && ld >= V && ld_d >= V && (!prior_logits || ld_prior >= V),
                "seq_dist_bwd: bad shape (n %d, V %d, ld %lld, ld_prior %lld, ld_d %lld)", n, V, (long long)ld,
                (long long)ld_prior, (long long)ld_d);
  GCT_CHECK_ARG(W >= 1 && W <= SEQ_LOGP_MAX_W, "seq_dist_bwd: rows of %d tokens (1 .. %d supported)", W,
                SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(ld_ys >= W && (!g_token_entropy || ld_ge >= W) && (!g_token_kl || ld_gk >= W),
                "seq_dist_bwd: ld_ys / ld_ge / ld_gk narrower than the %d token columns", W);
  GCT_CHECK_ARG(row_shift >= 0 && rows_per_seq >= (int64_t)row_shift + W - 1,
                "seq_dist_bwd: %lld logits rows per sequence do not hold %d + %d", (long long)rows_per_seq, row_shift,
                W - 1);
  const int64_t rows = (int64_t)n * rows_per_seq;
  if (rows == 0) return GCT_OK;
  int64_t g = (rows + 3) / 4;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(seq_dist_bwd_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, logits, ld, V,
                     rows_per_seq, row_shift, prior_logits, ld_prior, ys, ld_ys, prefix_lens, pad_id, W, g_entropy,
                     g_token_entropy, ld_ge, g_kl, g_token_kl, ld_gk, dlogits, ld_d, rows);
  GCT_LAUNCH_CHECK("seq_dist_bwd");
  return GCT_OK;
}

extern "C" int gct_chosen_logp(const float* logits, int V, const int64_t* ys, int64_t ld_ys, const int32_t* pos,
                               const int32_t* row_off, const int32_t* item, const int32_t* prefix_len, int64_t pad_id,
                               float* out, int64_t ld_out, int out_rows, int n, void* stream) {
  GCT_CHECK_ARG(logits && ys && pos && out && n >= 0 && V > 0 && ld_ys > 0 && ld_out > 0 && out_rows >= 0,
                "chosen_logp: bad args");
  GCT_CHECK_ARG(!item == !prefix_len && (!item || row_off), "chosen_logp: streamed rows need item, prefix_len and row_off");
  GCT_CHECK_ARG(item || out_rows >= n, "chosen_logp: %d output rows for %d decode rows", out_rows, n);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(chosen_logp_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, V,
                     ys, ld_ys, pos, row_off, item, prefix_len, pad_id, out, ld_out, out_rows, n);
  GCT_LAUNCH_CHECK("chosen_logp");
  return GCT_OK;
}
