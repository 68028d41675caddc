// K7: final-vocabulary cross-entropy.
// Reference: Train/trainer1.py:21-22  F.cross_entropy(logits.view(-1,V), ys,
// ignore_index=pad, reduction='sum').  V <= 31 in practice: one wave per row (row = 120 B),
// wave-level max / sum-exp; per-block partial sums reduced in fixed order.
//
// The scored-token family: three forward / backward pairs over one data layout, the token rows ys [n, W] next to their
// teacher-forced logits (SeqView: the geometry, THE scored predicate, the row address and its inverse).
//   seq_fwd_kernel<Op>  one workgroup per sequence, a wave per token column; per-token tables, and per-sequence sums
//                       added up by one thread in ascending column order: one writer per output, no atomics.
//   seq_bwd_kernel<Op>  one wave per logits row; a row that is not scored, or whose weights are 0, gets V exact zeros
//                       and its logits are not read.
// An Op holds what one entry point adds to the view and computes per scored token (decode.py states the rules):
//   gct_seq_logp / _bwd  score_reference / seq_logp_grad_reference: the log-probability of the given token
//                        (wave_token_logp) and its gradient, ce_grad_row with a weight per token column;
//   gct_seq_ppo / _bwd   ppo_reference / ppo_grad_reference: PPO's clipped surrogate of the token's probability ratio
//                        against the log-probability it was sampled with (ppo_token around wave_token_logp) and its
//                        gradient (ce_grad_write);
//   gct_seq_dist / _bwd  dist_reference / dist_grad_reference: the entropy of the next-token distribution and its KL
//                        divergence from a second model's (wave_row_dist) and their gradient.
// gct_chosen_logp scores the token a decode step has just picked, through wave_token_logp too.
#include <algorithm>
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
  float mx, lse;
  return gct_wave_token_logp(lr, V, tok, lane, hit, mx, lse);                // (common.h: shared with gct_step_stats)
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

// ------------------------------------------------------------------------------------------- the scored-token skeleton
constexpr int SEQ_LOGP_MAX_W = 256;

// A token id that can be scored at all: not pad, and inside the vocabulary.
__device__ __forceinline__ bool token_scored(int64_t tok, int64_t pad_id, int V) {
  return gct_token_scored(tok, pad_id, V);
}

// The geometry every seq_* entry point takes: token rows ys [n, W] (row stride ld_ys), prefix lengths (null: 1 each),
// and logits of rows_per_seq rows per sequence (row stride ld), of which row row_shift + c - 1 predicts token column c.
struct SeqView {
  const float* logits;
  int64_t ld;
  int V;
  int64_t rows_per_seq;
  int row_shift;
  const int64_t* ys;
  int64_t ld_ys;
  const int32_t* prefix_lens;
  int64_t pad_id;
  int W;

  __device__ __forceinline__ int t0(int64_t r) const { return prefix_lens ? prefix_lens[r] : 1; }
  // THE predicate: column c < W of sequence r (prefix length t0) is scored; tok = its token either way.
  __device__ __forceinline__ bool scored(int t0, int64_t r, int64_t c, int64_t& tok) const {
    tok = ys[r * ld_ys + c];
    return c >= t0 && c >= 1 && token_scored(tok, pad_id, V);
  }
  __device__ __forceinline__ int64_t row_of(int64_t r, int64_t c) const { return r * rows_per_seq + row_shift + c - 1; }
  __device__ __forceinline__ const float* logits_row(int64_t row) const { return logits + row * ld; }
  // row_of's inverse: false for a row that predicts no token column (a shift row, or one behind column W - 1)
  __device__ __forceinline__ bool column_of(int64_t row, int64_t& r, int64_t& c) const {
    r = row / rows_per_seq;
    const int64_t j = row - r * rows_per_seq;
    c = j - row_shift + 1;
    return j >= row_shift && c >= 1 && c < W;
  }
};

// One workgroup per sequence; wave w takes the token columns w, w + 4, ...  At a scored column Op::token fills the
// column's NSUM values (an unscored column keeps zeros, and no row of it is read) and returns its flag bits above bit 0
// (scored).  Lane 0 hands the values to Op::store_token and to LDS, and thread 0 adds each of them up in ascending
// column order and counts each flag for Op::store_seq: the sums do not depend on the grid or on which wave took a
// column.  Everything a branch depends on is one value per wave.
template <class Op>
__global__ __launch_bounds__(256) void seq_fwd_kernel(SeqView v, Op op) {
  constexpr int NSUM = Op::NSUM, NFLAG = Op::NFLAG;
  __shared__ float sh[NSUM * SEQ_LOGP_MAX_W + (NFLAG ? SEQ_LOGP_MAX_W / 4 : 0)];
  uint8_t* sh_flag = reinterpret_cast<uint8_t*>(sh + NSUM * SEQ_LOGP_MAX_W);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int t0 = v.t0(r);
  for (int c = wave; c < v.W; c += 4) {                 // uniform over the wave
    int64_t tok;
    const bool scored = v.scored(t0, r, c, tok);
    float s[NSUM] = {};
    int flags = scored ? 1 : 0;
    if (scored) flags |= op.token(v, r, c, (int)tok, lane, s);
    if (lane == 0) {
      op.store_token(r, c, s);
#pragma unroll
      for (int k = 0; k < NSUM; ++k) sh[k * SEQ_LOGP_MAX_W + c] = s[k];
      if constexpr (NFLAG > 0) sh_flag[c] = (uint8_t)flags;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum[NSUM] = {};
    int cnt[NFLAG + 1] = {};
    for (int c = 0; c < v.W; ++c) {                     // a column that is not scored holds 0
#pragma unroll
      for (int k = 0; k < NSUM; ++k) sum[k] += sh[k * SEQ_LOGP_MAX_W + c];
#pragma unroll
      for (int b = 0; b < NFLAG; ++b) cnt[b] += (sh_flag[c] >> b) & 1;
    }
    op.store_seq(r, sum, cnt);
  }
}

// One wave per logits row, four rows per workgroup, the grid strides over the rest (ce_bwd_kernel's layout).  A row
// that predicts a scored column asks Op::weight for its weights (every other row keeps Weight{}: zeros), and a row
// whose weights are not Op::dead asks Op::row for the row of dlogits (false: nothing written).  Every other row gets V
// exact zeros and its logits are NOT read (the decoder may never have computed them).  Everything a branch depends on
// is one value per wave.  The SGPR budget keeps the widest Op (DistBwd) at 8 waves per SIMD; it costs no spill.
template <class Op>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(100))) void
seq_bwd_kernel(SeqView v, Op op, float* __restrict__ dlogits, int64_t ld_d, int64_t rows) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    int64_t r, c, tok = 0;
    float* dr = dlogits + row * ld_d;
    typename Op::Weight w{};
    if (v.column_of(row, r, c) && v.scored(v.t0(r), r, c, tok)) w = op.weight(r, c);
    if (Op::dead(w) || !op.row(v, r, c, row, tok, w, dr, lane))
      for (int i = lane; i < v.V; i += 64) dr[i] = 0.f;
  }
}

// g_row[r] + g_table[r][c], a null pointer counting as 0
__device__ __forceinline__ float seq_weight(const float* g_row, const float* g_table, int64_t ld_g, int64_t r,
                                            int64_t c) {
  return (g_row ? g_row[r] : 0.f) + (g_table ? g_table[r * ld_g + c] : 0.f);
}

// ---- log-probability of the given token.  Sum: logp; flags: scored, hit.
struct LogpFwd {
  static constexpr int NSUM = 1, NFLAG = 2;
  float* token_logp;
  int64_t ld_out;
  float* logp;
  int32_t *tokens, *hits;
  __device__ __forceinline__ int token(const SeqView& v, int64_t r, int c, int tok, int lane, float* s) const {
    bool hit;
    s[0] = wave_token_logp(v.logits_row(v.row_of(r, c)), v.V, tok, lane, hit);
    return hit ? 2 : 0;
  }
  __device__ __forceinline__ void store_token(int64_t r, int c, const float* s) const {
    token_logp[r * ld_out + c] = s[0];
  }
  __device__ __forceinline__ void store_seq(int64_t r, const float* sum, const int* cnt) const {
    logp[r] = sum[0];
    tokens[r] = cnt[0];
    hits[r] = cnt[1];
  }
};

// Weight g = g_logp[r] + g_token[r][c]; the row is ce_grad_row, the row arithmetic of gct_ce_bwd, with -g.
struct LogpBwd {
  using Weight = float;
  const float *g_logp, *g_token;
  int64_t ld_g;
  __device__ __forceinline__ float weight(int64_t r, int64_t c) const {
    return seq_weight(g_logp, g_token, ld_g, r, c);
  }
  static __device__ __forceinline__ bool dead(float g) { return g == 0.f; }
  __device__ __forceinline__ bool row(const SeqView& v, int64_t r, int64_t c, int64_t row, int64_t tok, float g,
                                      float* dr, int lane) const {
    ce_grad_row(v.logits_row(row), dr, v.V, tok, -g, lane);
    return true;
  }
};

// ---- PPO.  What both directions read beside the view; old_token_logp is not read at a column that is not scored.
struct PpoIn {
  const float* old_token_logp;
  int64_t ld_old;
  const float* advantage;
  float clip_lo, clip_hi;
  __device__ __forceinline__ PpoToken token(float lp, float A, int64_t r, int64_t c) const {
    return ppo_token(lp, old_token_logp[r * ld_old + c], A, clip_lo, clip_hi);
  }
};

// Sums: logp (wave_token_logp: gct_seq_logp's bits), surrogate, the k3 terms; flags: scored, hit, clipped.
struct PpoFwd {
  static constexpr int NSUM = 3, NFLAG = 3;
  PpoIn in;
  float *token_logp, *token_surrogate;
  int64_t ld_out;
  float *logp, *surrogate, *approx_kl;
  int32_t *tokens, *hits, *clipped;
  __device__ __forceinline__ int token(const SeqView& v, int64_t r, int c, int tok, int lane, float* s) const {
    bool hit;
    s[0] = wave_token_logp(v.logits_row(v.row_of(r, c)), v.V, tok, lane, hit);
    const PpoToken t = in.token(s[0], in.advantage[r], r, c);
    s[1] = t.surrogate;
    s[2] = t.k3;
    return (hit ? 2 : 0) | (t.clipped ? 4 : 0);
  }
  __device__ __forceinline__ void store_token(int64_t r, int c, const float* s) const {
    token_logp[r * ld_out + c] = s[0];
    token_surrogate[r * ld_out + c] = s[1];
  }
  __device__ __forceinline__ void store_seq(int64_t r, const float* sum, const int* cnt) const {
    logp[r] = sum[0];
    surrogate[r] = sum[1];
    approx_kl[r] = sum[2];
    tokens[r] = cnt[0];
    hits[r] = cnt[1];
    clipped[r] = cnt[2];
  }
};

// Weights g = g_surrogate[r] + g_token[r][c] and A = advantage[r]: both must count.  The row's softmax statistics are
// taken once: lp (wave_token_logp's bits), rho and the clip decision follow from them, and the row is left to the
// zeros (clipped) or is ce_grad_write with the weight -((g * A) * rho): rho == 1 gives gct_seq_logp_bwd's bits for
// g_logp = g * A.
struct PpoBwd {
  struct Weight {
    float g, A;
  };
  PpoIn in;
  const float *g_surrogate, *g_token;
  int64_t ld_g;
  __device__ __forceinline__ Weight weight(int64_t r, int64_t c) const {
    return {seq_weight(g_surrogate, g_token, ld_g, r, c), in.advantage[r]};
  }
  static __device__ __forceinline__ bool dead(Weight w) { return w.g == 0.f || w.A == 0.f; }
  __device__ __forceinline__ bool row(const SeqView& v, int64_t r, int64_t c, int64_t row, int64_t tok, Weight w,
                                      float* dr, int lane) const {
    const float* lr = v.logits_row(row);
    float mx, se;
    gct_wave_softmax_stats(lr, v.V, lane, mx, se);
    const float lp = (lr[tok] - mx) - logf(se);
    const PpoToken t = in.token(lp, w.A, r, c);
    if (t.clipped) return false;
    ce_grad_write(lr, dr, v.V, tok, -((w.g * w.A) * t.rho), lane, mx, se);
    return true;
  }
};

// ---- entropy and KL from a prior (null: entropy alone).  Sums: entropy, kl; no flags.
struct DistFwd {
  static constexpr int NSUM = 2, NFLAG = 0;
  const float* prior;
  int64_t ld_prior;
  float* token_entropy;
  int64_t ld_out;
  float *entropy, *token_kl, *kl;
  __device__ __forceinline__ int token(const SeqView& v, int64_t r, int c, int tok, int lane, float* s) const {
    const int64_t row = v.row_of(r, c);
    const RowDist d = wave_row_dist(v.logits_row(row), prior ? prior + row * ld_prior : nullptr, v.V, lane);
    s[0] = d.H;
    s[1] = d.KL;
    return 0;
  }
  __device__ __forceinline__ void store_token(int64_t r, int c, const float* s) const {
    token_entropy[r * ld_out + c] = s[0];
    if (prior) token_kl[r * ld_out + c] = s[1];
  }
  __device__ __forceinline__ void store_seq(int64_t r, const float* sum, const int*) const {
    entropy[r] = sum[0];
    if (prior) kl[r] = sum[1];
  }
};

// Weights a = g_entropy[r] + g_token_entropy[r][c] and b = g_kl[r] + g_token_kl[r][c]; the row is
// a * (-p_v (log p_v + H)) + b * (p_v ((log p_v - log q_v) - KL)),  exact zeros where p_v == 0.  The prior's row is
// read only where b != 0 (b != 0 only with a prior: checked by the host).
struct DistBwd {
  struct Weight {
    float a, b;
  };
  const float* prior;
  int64_t ld_prior;
  const float *g_entropy, *g_token_entropy;
  int64_t ld_ge;
  const float *g_kl, *g_token_kl;
  int64_t ld_gk;
  __device__ __forceinline__ Weight weight(int64_t r, int64_t c) const {
    return {seq_weight(g_entropy, g_token_entropy, ld_ge, r, c), seq_weight(g_kl, g_token_kl, ld_gk, r, c)};
  }
  static __device__ __forceinline__ bool dead(Weight w) { return w.a == 0.f && w.b == 0.f; }
  __device__ __forceinline__ bool row(const SeqView& v, int64_t r, int64_t c, int64_t row, int64_t tok, Weight w,
                                      float* dr, int lane) const {
    const float* lr = v.logits_row(row);
    const float* pr = w.b != 0.f ? prior + row * ld_prior : nullptr;
    const RowDist d = wave_row_dist(lr, pr, v.V, lane);
    for (int i = lane; i < v.V; i += 64) {
      const float y = lr[i] - d.m, e = expf(y);
      float g = 0.f;
      if (e != 0.f) {
        const float p = e * d.inv, lp = y - d.lse;
        g = w.a * (-p * (lp + d.H));
        if (pr) g += w.b * (p * ((lp - ((pr[i] - d.pm) - d.plse)) - d.KL));
      }
      dr[i] = g;
    }
    return true;
  }
};

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
  if (token_scored(tok, pad_id, V)) lp = wave_token_logp(logits + (int64_t)row * V, V, (int)tok, lane, hit);
  if (lane == 0) out[(int64_t)dst * ld_out + p] = lp;
}

// The checks the six seq_* entry points share, behind their own pointer checks; `name` opens every message.  row_ld:
// the narrowest of the caller's logits-like row strides (ld, ld_prior, ld_d), table_ld: the narrowest of its [n, W]
// tables' (ld_out, ld_old, ld_g ...), each counted only where the pointer is there.
int seq_check_view(const char* name, const SeqView& v, int n, int64_t row_ld, int64_t table_ld) {
  GCT_CHECK_ARG(v.logits && v.ys, "%s: null pointer (logits, ys)", name);
  GCT_CHECK_ARG(n >= 0 && v.V > 0 && row_ld >= v.V, "%s: bad shape (n %d, V %d, narrowest row stride %lld)", name, n,
                v.V, (long long)row_ld);
  GCT_CHECK_ARG(v.W >= 1 && v.W <= SEQ_LOGP_MAX_W, "%s: rows of %d tokens (1 .. %d supported)", name, v.W,
                SEQ_LOGP_MAX_W);
  GCT_CHECK_ARG(v.ld_ys >= v.W && table_ld >= v.W,
                "%s: a row stride (ys %lld, narrowest table %lld) narrower than the %d token columns", name,
                (long long)v.ld_ys, (long long)table_ld, v.W);
  GCT_CHECK_ARG(v.row_shift >= 0 && v.rows_per_seq >= (int64_t)v.row_shift + v.W - 1,
                "%s: %lld logits rows per sequence do not hold %d + %d", name, (long long)v.rows_per_seq, v.row_shift,
                v.W - 1);
  return GCT_OK;
}

int seq_check_clip(const char* name, float clip_lo, float clip_hi) {
  GCT_CHECK_ARG(clip_lo >= 0.f && clip_lo < 1.f && clip_hi >= 0.f,
                "%s: clip (%g, %g) outside 0 <= clip_lo < 1, clip_hi >= 0", name, (double)clip_lo, (double)clip_hi);
  return GCT_OK;
}

// the stride of a table that may be null: one that is not there narrows nothing
int64_t ld_if(const void* table, int64_t ld) { return table ? ld : INT64_MAX; }

template <class Op>
int seq_launch_fwd(const char* name, const SeqView& v, int n, const Op& op, void* stream) {
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(seq_fwd_kernel<Op>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, v, op);
  GCT_LAUNCH_CHECK(name);
  return GCT_OK;
}

// four rows per workgroup, at most 4096 workgroups
unsigned seq_bwd_grid(int64_t rows) { return (unsigned)std::min<int64_t>((rows + 3) / 4, 4096); }

template <class Op>
int seq_launch_bwd(const char* name, const SeqView& v, int n, const Op& op, float* dlogits, int64_t ld_d,
                   void* stream) {
  const int64_t rows = (int64_t)n * v.rows_per_seq;
  if (rows == 0) return GCT_OK;
  hipLaunchKernelGGL(seq_bwd_kernel<Op>, dim3(seq_bwd_grid(rows)), dim3(256), 0, (hipStream_t)stream, v, op, dlogits,
                     ld_d, rows);
  GCT_LAUNCH_CHECK(name);
  return GCT_OK;
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
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(token_logp && logp && tokens && hits, "seq_logp: null pointer (outputs)");
  if (int rc = seq_check_view("seq_logp", v, n, ld, ld_out)) return rc;
  return seq_launch_fwd("seq_logp", v, n, LogpFwd{token_logp, ld_out, logp, tokens, hits}, stream);
}

extern "C" int gct_seq_logp_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                                const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                                int W, const float* g_logp, const float* g_token, int64_t ld_g, float* dlogits,
                                int64_t ld_d, void* stream) {
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(dlogits, "seq_logp_bwd: null pointer (dlogits)");
  GCT_CHECK_ARG(g_logp || g_token, "seq_logp_bwd: both gradients are null (g_logp, g_token)");
  if (int rc = seq_check_view("seq_logp_bwd", v, n, std::min(ld, ld_d), ld_if(g_token, ld_g))) return rc;
  return seq_launch_bwd("seq_logp_bwd", v, n, LogpBwd{g_logp, g_token, ld_g}, dlogits, ld_d, stream);
}

extern "C" int gct_seq_ppo(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                           const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n, int W,
                           const float* old_token_logp, int64_t ld_old, const float* advantage, float clip_lo,
                           float clip_hi, float* token_logp, float* token_surrogate, int64_t ld_out, float* logp,
                           float* surrogate, float* approx_kl, int32_t* tokens, int32_t* hits, int32_t* clipped,
                           void* stream) {
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(token_logp && token_surrogate && logp && surrogate && approx_kl && tokens && hits && clipped,
                "seq_ppo: null pointer (outputs)");
  GCT_CHECK_ARG(old_token_logp && advantage, "seq_ppo: null pointer (old_token_logp, advantage)");
  if (int rc = seq_check_view("seq_ppo", v, n, ld, std::min(ld_out, ld_old))) return rc;
  if (int rc = seq_check_clip("seq_ppo", clip_lo, clip_hi)) return rc;
  const PpoIn in{old_token_logp, ld_old, advantage, clip_lo, clip_hi};
  return seq_launch_fwd("seq_ppo", v, n, PpoFwd{in, token_logp, token_surrogate, ld_out, logp, surrogate, approx_kl,
                                                tokens, hits, clipped}, stream);
}

extern "C" int gct_seq_ppo_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                               const int64_t* ys, int64_t ld_ys, const int32_t* prefix_lens, int64_t pad_id, int n,
                               int W, const float* old_token_logp, int64_t ld_old, const float* advantage,
                               float clip_lo, float clip_hi, const float* g_surrogate,
                               const float* g_token_surrogate, int64_t ld_g, float* dlogits, int64_t ld_d,
                               void* stream) {
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(dlogits, "seq_ppo_bwd: null pointer (dlogits)");
  GCT_CHECK_ARG(old_token_logp && advantage, "seq_ppo_bwd: null pointer (old_token_logp, advantage)");
  GCT_CHECK_ARG(g_surrogate || g_token_surrogate,
                "seq_ppo_bwd: both gradients are null (g_surrogate, g_token_surrogate)");
  if (int rc = seq_check_view("seq_ppo_bwd", v, n, std::min(ld, ld_d),
                              std::min(ld_old, ld_if(g_token_surrogate, ld_g))))
    return rc;
  if (int rc = seq_check_clip("seq_ppo_bwd", clip_lo, clip_hi)) return rc;
  const PpoIn in{old_token_logp, ld_old, advantage, clip_lo, clip_hi};
  return seq_launch_bwd("seq_ppo_bwd", v, n, PpoBwd{in, g_surrogate, g_token_surrogate, ld_g}, dlogits, ld_d, stream);
}

extern "C" int gct_seq_dist(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                            const float* prior_logits, int64_t ld_prior, const int64_t* ys, int64_t ld_ys,
                            const int32_t* prefix_lens, int64_t pad_id, int n, int W, float* token_entropy,
                            int64_t ld_out, float* entropy, float* token_kl, float* kl, void* stream) {
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(token_entropy && entropy, "seq_dist: null pointer (outputs)");
  GCT_CHECK_ARG(prior_logits || (!token_kl && !kl), "seq_dist: kl outputs without prior logits");
  GCT_CHECK_ARG(!prior_logits || (token_kl && kl), "seq_dist: prior logits without kl outputs (null pointer)");
  if (int rc = seq_check_view("seq_dist", v, n, std::min(ld, ld_if(prior_logits, ld_prior)), ld_out)) return rc;
  return seq_launch_fwd("seq_dist", v, n,
                        DistFwd{prior_logits, ld_prior, token_entropy, ld_out, entropy, token_kl, kl}, stream);
}

extern "C" int gct_seq_dist_bwd(const float* logits, int64_t ld, int V, int64_t rows_per_seq, int row_shift,
                                const float* prior_logits, int64_t ld_prior, const int64_t* ys, int64_t ld_ys,
                                const int32_t* prefix_lens, int64_t pad_id, int n, int W, const float* g_entropy,
                                const float* g_token_entropy, int64_t ld_ge, const float* g_kl,
                                const float* g_token_kl, int64_t ld_gk, float* dlogits, int64_t ld_d, void* stream) {
  const SeqView v{logits, ld, V, rows_per_seq, row_shift, ys, ld_ys, prefix_lens, pad_id, W};
  GCT_CHECK_ARG(dlogits, "seq_dist_bwd: null pointer (dlogits)");
  GCT_CHECK_ARG(g_entropy || g_token_entropy || g_kl || g_token_kl,
                "seq_dist_bwd: all four gradients are null (g_entropy, g_token_entropy, g_kl, g_token_kl)");
  GCT_CHECK_ARG(prior_logits || (!g_kl && !g_token_kl), "seq_dist_bwd: kl gradients without prior logits");
  if (int rc = seq_check_view("seq_dist_bwd", v, n, std::min({ld, ld_d, ld_if(prior_logits, ld_prior)}),
                              std::min(ld_if(g_token_entropy, ld_ge), ld_if(g_token_kl, ld_gk))))
    return rc;
  return seq_launch_bwd("seq_dist_bwd", v, n,
                        DistBwd{prior_logits, ld_prior, g_entropy, g_token_entropy, ld_ge, g_kl, g_token_kl, ld_gk},
                        dlogits, ld_d, stream);
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
