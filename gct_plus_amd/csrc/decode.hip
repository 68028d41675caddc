// KV-cached autoregressive decode helpers (reference
// Inference/sampling_tool.py:140-184 re-runs the WHOLE decoder on ys[:, :i+1] every step).
//   gct_attn_decode  : one query row per (sample, head) against cached keys/values
//   gct_select_token : softmax over the vocabulary + greedy / multinomial choice (optionally through a top-k /
//                      nucleus / temperature filter), appends the token, updates the key-valid flags and the
//                      per-sample finished mask
//   gct_grammar_mask : constrained decoding -- a copy of the step's logits with -inf on every token the SMILES grammar
//                      or the row's length budget forbids, for gct_select_token to choose from
//   gct_step_stats   : behind the selection -- the model's entropy and the log-probability, entropy and KL divergence of
//                      the distribution the token was really drawn from (gct_select_token's probs_out)
//   gct_stream_refill : continuous batching -- rows that finished hand out their tokens and take the next pool item
//   gct_attn_decode_beam / gct_beam_select : the same two for beam search, with the self-attention caches
//                      shared by ancestry through a per-row map (kv_src) instead of copied
//   gct_beam_select_gumbel : stochastic beam search -- the other instantiation of gct_beam_select's kernel template,
//                      ordering the candidates by Gumbel-perturbed log-probabilities conditioned on their parent's
//   gct_grammar_mask_anc / gct_smc_select : sequential Monte Carlo under the grammar on the same beam-shaped rows -- the
//                      grammar kernel's other instantiation reads a particle's history through kv_src; the selection
//                      weights the particles by the mass the mask leaves, resamples their ancestors and draws
//   gct_attn_decode_z / gct_decode_embed / gct_decode_advance : cross-attention over the latent rows, one position's
//                      embedding, the device counter
// All are small and HBM/latency-bound; they exist so a whole decode step is a fixed kernel chain with no host round
// trip (graph-capturable).  Where a row of a step sits is stated once, in decode_rows.h.
#include <climits>
#include <type_traits>

#include "common.h"
#include "decode_rows.h"
#include "smiles_grammar.h"

namespace {

// one wave per (b, h); 16 lanes per key for the scores (4 keys per pass), lanes over d for P.V.
// pos (nullable): DEVICE-side step counter -- the cache holds Lc = cache_off + *pos keys, and the step's own key /
// value (knew / vnew, row b of a [n][ldn] step buffer) are the last key: they are appended to the caches here
// (row Lc) and scored from registers, so ONE captured graph serves every step of the decode loop.
// MAPPED (beam search, pos required): key / value j of row b and the valid flag masking it live in physical row
// kv_src[b][j] (Lc_host = cache rows, the bound of every map entry's position); the step's own key still goes to row b.
// RAGGED (pos required, not MAPPED): row b sits at its own position (gct_row_slot): Lold = cache_off + that position,
// and the step's key is appended at that row.
template <int DK, bool MAPPED, bool RAGGED>
__global__ __launch_bounds__(256) void attn_decode_kernel(
    const float* __restrict__ q, int64_t ldq, float* __restrict__ k, float* __restrict__ v,
    int64_t kv_row, int64_t kv_batch, const uint8_t* __restrict__ valid, int64_t valid_sb,
    float* __restrict__ o, int64_t ldo, int n, int H, int Lc_host, float scale,
    const int32_t* __restrict__ pos, int cache_off, const float* __restrict__ knew,
    const float* __restrict__ vnew, int64_t ldn, const int32_t* __restrict__ klen,
    const int32_t* __restrict__ kv_src, int64_t ld_src, const int32_t* __restrict__ row_off) {
  static_assert(!(MAPPED && RAGGED), "ragged rows are not supported by the beam (mapped) form");
  __shared__ float sc[4][256];
  __shared__ int32_t rs[4][256];     // MAPPED: physical row of key j
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
  if (pair >= (int64_t)n * H) return;
  const int b = (int)(pair / H), h = (int)(pair - (int64_t)b * H);
  // klen (nullable, without pos): the keys of sample b beyond klen[b] are masked (`valid` says so too) and b sees at
  // least one key, so they weigh exactly 0: their cache rows are never read (the padded latent positions of the
  // cross-attention memory are most of it at MOSES-like lengths)
  int Lold;                                                                        // keys already in the cache
  if constexpr (RAGGED) Lold = gct_row_slot(cache_off + *pos, b, true, row_off).pos;   // uniform over the wave
  else Lold = pos ? cache_off + *pos : (klen ? min(klen[b], Lc_host) : Lc_host);   // klen clamped to Lc, as in _z
  const int Lc = pos ? Lold + 1 : Lold;
  const float* qp = q + (int64_t)b * ldq + h * DK;
  float* kp = k + (int64_t)b * kv_batch + h * DK;
  float* vp = v + (int64_t)b * kv_batch + h * DK;
  const uint8_t* vl = valid ? valid + (int64_t)b * valid_sb : nullptr;
  constexpr int LPK = DK / 4;        // lanes per key (float4 each)
  constexpr int KPP = 64 / LPK;      // keys per pass
  const int sub = lane % LPK, kslot = lane / LPK;
  const float4 qv = *reinterpret_cast<const float4*>(qp + sub * 4);
  if constexpr (MAPPED) {
    if (Lold >= Lc_host) return;                  // no room for this step's key (the host sizes the caches)
    const int32_t* sr = kv_src + (int64_t)b * ld_src;
    for (int j = lane; j < Lold; j += 64) {
      const int r = sr[j];
      rs[wave][j] = r < 0 ? 0 : (r >= n ? n - 1 : r);
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
  }
  float vlast = 0.f;
  if (pos) {
    // this step's key: score it from the step buffer and append key / value to the caches
    const float* kn = knew + (int64_t)b * ldn + h * DK;
    const float* vn = vnew + (int64_t)b * ldn + h * DK;
    float s = 0.f;
    if (lane < LPK) {
      const float4 kv4 = *reinterpret_cast<const float4*>(kn + lane * 4);
      s = (qv.x * kv4.x + qv.y * kv4.y) + (qv.z * kv4.z + qv.w * kv4.w);   // sub == lane here
      *reinterpret_cast<float4*>(kp + (int64_t)Lold * kv_row + lane * 4) = kv4;
      *reinterpret_cast<float4*>(vp + (int64_t)Lold * kv_row + lane * 4) = *reinterpret_cast<const float4*>(vn + lane * 4);
    }
#pragma unroll
    for (int off = LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
      s *= scale;
      if (vl && vl[Lold] == 0) s = -1e9f;
      sc[wave][Lold] = s;
    }
    if (lane < DK) vlast = vn[lane];
  }
  float m = -INFINITY;
  for (int j0 = 0; j0 < Lold; j0 += KPP) {
    const int j = j0 + kslot;
    float s = 0.f;
    if (j < Lold) {
      const float* kj;
      if constexpr (MAPPED) kj = k + (int64_t)rs[wave][j] * kv_batch + h * DK + (int64_t)j * kv_row;
      else kj = kp + (int64_t)j * kv_row;
      const float4 kv4 = *reinterpret_cast<const float4*>(kj + sub * 4);
      s = (qv.x * kv4.x + qv.y * kv4.y) + (qv.z * kv4.z + qv.w * kv4.w);
    }
#pragma unroll
    for (int off = LPK / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (j < Lold && sub == 0) {
      s *= scale;
      if constexpr (MAPPED) {
        if (valid && valid[(int64_t)rs[wave][j] * valid_sb + j] == 0) s = -1e9f;
      } else {
        if (vl && vl[j] == 0) s = -1e9f;            // masked_fill(mask == 0, -1e9)
      }
      sc[wave][j] = s;
    }
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  for (int j = lane; j < Lc; j += 64) m = fmaxf(m, sc[wave][j]);
  m = gct_wave_max(m);
  float l = 0.f;
  for (int j = lane; j < Lc; j += 64) {
    const float e = expf(sc[wave][j] - m);
    sc[wave][j] = e;
    l += e;
  }
  l = gct_wave_sum(l);
  const float inv = 1.0f / l;
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_wave_barrier();
  if (lane < DK) {
    float acc = 0.f;
    if constexpr (MAPPED) {
      const float* vh = v + h * DK + lane;
      for (int j = 0; j < Lold; ++j)
        acc = fmaf(sc[wave][j] * inv, vh[(int64_t)rs[wave][j] * kv_batch + (int64_t)j * kv_row], acc);
    } else {
      for (int j = 0; j < Lold; ++j) acc = fmaf(sc[wave][j] * inv, vp[(int64_t)j * kv_row + lane], acc);
    }
    if (pos) acc = fmaf(sc[wave][Lold] * inv, vlast, acc);
    o[(int64_t)b * ldo + h * DK + lane] = acc;
  }
}

// Cross-attention of one decode step over the LATENT memory itself.  The cross-attention keys / values of the
// reference are projections of e_j = fc_z(z_j): k_{j,h} = G_h z_j + c_h, v_{j,h} = H_h z_j + d_h with G_h = W_k,h W_z
// and H_h = W_v,h W_z (64 x latent).  A score q_h . k_{j,h} is (G_h^T q_h) . z_j plus a term that is the same for
// every key of the row (softmax-invariant), and sum_j p_j v_{j,h} = H_h (sum_j p_j z_j) + d_h.  With G_h^T folded into
// the query projection and H_h into the output projection (host side, once per sequence), a step reads the z rows of
// a sample ONCE for all heads -- latent x 4 B per key instead of 2 x d_model x 4 B (8 x less at latent 128, d 512).
// One workgroup per sample: z rows -> LDS, scores for (head, key) pairs, softmax per head, context (head, latent).
// The n_c condition rows of a cond2lat memory are not functions of z: they keep explicit per-head keys / values
// (shifted by -c_h / -d_h on the host so that the two kinds of key share one softmax).
__global__ __launch_bounds__(256) void attn_decode_z_kernel(
    const float* __restrict__ q, int64_t ldq, int qoff, const float* __restrict__ z, int64_t z_batch, int lat, int Le,
    const float* __restrict__ ckv, int64_t ckv_batch, int64_t ld_ckv, int nc, int d, const uint8_t* __restrict__ valid,
    int64_t valid_sb, const int32_t* __restrict__ klen, float* __restrict__ out, int64_t ldo, int ooff, int H, int dk,
    float scale) {
  extern __shared__ __attribute__((aligned(16))) float zl[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Lk = nc + Le, zs_ld = lat + 4, lat4 = lat >> 2, Lp = (Lk + 3) & ~3;
  float* zs = zl;                              // [Le][lat + 4]
  float* qs = zl + (size_t)Le * zs_ld;         // [H][lat]
  float* ps = qs + (size_t)H * lat;            // [H][Lp]
  // keys beyond klen[b] are masked and the sample sees a key: weight exactly 0, never read
  const int Lvis = klen ? (klen[b] < Lk ? klen[b] : Lk) : Lk;
  const int ncv = nc < Lvis ? nc : Lvis, nz = Lvis - ncv;
  const float* zb = z + (int64_t)b * z_batch;
  const float* qb = q + (int64_t)b * ldq;
  for (int i = tid; i < nz * lat4; i += 256) {
    const int row = i / lat4, c4 = i - row * lat4;
    *reinterpret_cast<float4*>(zs + row * zs_ld + c4 * 4) = *reinterpret_cast<const float4*>(zb + (int64_t)row * lat + c4 * 4);
  }
  for (int i = tid; i < H * lat4; i += 256)
    *reinterpret_cast<float4*>(qs + i * 4) = *reinterpret_cast<const float4*>(qb + qoff + i * 4);
  __syncthreads();
  const uint8_t* vl = valid ? valid + (int64_t)b * valid_sb : nullptr;
  for (int i = tid; i < H * nz; i += 256) {          // consecutive lanes: consecutive keys of one head
    const int h = i / nz, j = i - h * nz;
    const float* zr = zs + j * zs_ld;
    const float* qh = qs + h * lat;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = 0; c < lat; c += 4) {
      const float4 a = *reinterpret_cast<const float4*>(qh + c), k4 = *reinterpret_cast<const float4*>(zr + c);
      s0 = fmaf(a.x, k4.x, s0); s1 = fmaf(a.y, k4.y, s1); s2 = fmaf(a.z, k4.z, s2); s3 = fmaf(a.w, k4.w, s3);
    }
    float sc = ((s0 + s1) + (s2 + s3)) * scale;
    if (vl && vl[ncv + j] == 0) sc = -1e9f;          // masked_fill(mask == 0, -1e9)
    ps[h * Lp + ncv + j] = sc;
  }
  for (int i = tid; i < H * ncv; i += 256) {         // explicit condition rows: q_h . k'_{j,h} over the head dim
    const int h = i / ncv, j = i - h * ncv;
    const float* kr = ckv + (int64_t)b * ckv_batch + (int64_t)j * ld_ckv + h * dk;
    const float* qh = qb + h * dk;
    float sc = 0.f;
    for (int c = 0; c < dk; ++c) sc = fmaf(qh[c], kr[c], sc);
    sc *= scale;
    if (vl && vl[j] == 0) sc = -1e9f;
    ps[h * Lp + j] = sc;
  }
  __syncthreads();
  for (int h = wave; h < H; h += 4) {                // softmax of one head per wave
    float* pr = ps + h * Lp;
    float m = -INFINITY;
    for (int j = lane; j < Lvis; j += 64) m = fmaxf(m, pr[j]);
    m = gct_wave_max(m);
    float l = 0.f;
    for (int j = lane; j < Lvis; j += 64) {
      const float e = expf(pr[j] - m);
      pr[j] = e;
      l += e;
    }
    l = gct_wave_sum(l);
    const float inv = 1.0f / l;
    for (int j = lane; j < Lvis; j += 64) pr[j] *= inv;
  }
  __syncthreads();
  float* ob = out + (int64_t)b * ldo;
  for (int i = tid; i < H * lat4; i += 256) {        // context of head h in the latent space: sum_j p_j z_j
    const int h = i / lat4, c4 = i - h * lat4;
    const float* pr = ps + h * Lp + ncv;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = 0; j < nz; ++j) {
      const float w = pr[j];
      const float4 z4 = *reinterpret_cast<const float4*>(zs + j * zs_ld + c4 * 4);
      acc.x = fmaf(w, z4.x, acc.x); acc.y = fmaf(w, z4.y, acc.y); acc.z = fmaf(w, z4.z, acc.z); acc.w = fmaf(w, z4.w, acc.w);
    }
    *reinterpret_cast<float4*>(ob + ooff + h * lat + c4 * 4) = acc;
  }
  if (nc > 0) {
    for (int i = tid; i < d; i += 256) {             // condition rows: sum_j p_j v'_{j,h}, head-major like the reference
      const int h = i / dk;
      const float* pr = ps + h * Lp;
      float acc = 0.f;
      for (int j = 0; j < ncv; ++j) acc = fmaf(pr[j], ckv[(int64_t)b * ckv_batch + (int64_t)j * ld_ckv + d + i], acc);
      ob[i] = acc;
    }
  }
}

// x[b][:] = table[ys[b][*pos]] * scale + pe[pe_off + *pos][:]   (Embeddings + PositionalEncoding of ONE position)
// RAGGED: row b at its own position (gct_row_slot; one load per thread, consecutive threads still store float4s in a row)
template <bool RAGGED>
__global__ __launch_bounds__(256) void decode_embed_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, const int32_t* __restrict__ pos, int pe_off,
    const float* __restrict__ table, int vocab, const float* __restrict__ pe, float* __restrict__ out, int n, int d,
    float scale, const int32_t* __restrict__ row_off) {
  const int p0 = *pos;
  const int64_t total = (int64_t)n * (d / 4);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / (d / 4)), c = (int)(i - (int64_t)b * (d / 4));
    const int p = gct_row_slot(p0, b, RAGGED, row_off).pos;
    int64_t tok = ys[(int64_t)b * ld_ys + p];
    tok = tok < 0 ? 0 : (tok >= vocab ? vocab - 1 : tok);
    const float4 e = *reinterpret_cast<const float4*>(table + tok * d + c * 4);
    const float4 q = *reinterpret_cast<const float4*>(pe + (int64_t)(pe_off + p) * d + c * 4);
    *reinterpret_cast<float4*>(out + (int64_t)b * d + c * 4) =
        make_float4(e.x * scale + q.x, e.y * scale + q.y, e.z * scale + q.z, e.w * scale + q.w);
  }
}

__global__ void decode_advance_kernel(int32_t* pos) { *pos += 1; }

// the draw's uniform, in (0, 1]: the fp32 addition rounds to even once x >> 8 >= 2^23, so x >> 8 = 2^24 - 1 gives 1.0
// and a row whose cumulative sums never exceed u takes the fallback (the last token of nonzero weight)
__device__ __forceinline__ float u01_draw(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// ---------------------------------------------------------------------------------------------- token selection
// What the two select kernels share.  None of the three helpers holds a multiply that feeds an add, so they compute the
// same under select_token_filtered_kernel's `fp contract(off)` (the pragma is lexical and does not reach them).
//
// The prologue: the row's slot (gct_row_slot at the column *pos_dev + 1, or pos_host), the seed_dev override of the
// by-value seed, and the Philox key (row | item_base + item, token position) -- a streamed row's draw depends neither on
// the row that makes it nor on the slice of a larger pool the item came in.  false: the wave leaves -- no such row, a
// parked row, a position inside the item's prefix (the slot keeps the prefix token the refill laid there: ys and valid, done
// untouched) or a streamed row without room for its valid flag.  All of it is uniform over the wave.
template <bool RAGGED, bool STREAM>
__device__ __forceinline__ bool select_prologue(int row, int n, int pos_host, const int32_t* pos_dev, const int32_t* row_off,
                                                const int32_t* item, const int32_t* prefix_len, int item_base,
                                                int valid_off, int64_t valid_sb, const uint64_t* seed_dev, GctRng& rng,
                                                int& pos, uint32_t& key) {
  static_assert(RAGGED || !STREAM, "streamed rows sit at their own positions");
  const int step = pos_dev ? *pos_dev + 1 : pos_host;
  if (seed_dev) rng = gct_rng_make(*seed_dev, 0xDEC0DEu);
  if (row >= n) return false;
  const GctRowSlot s = gct_row_slot(step, row, RAGGED, row_off, STREAM, item, prefix_len);
  pos = s.pos;
  key = (uint32_t)(STREAM ? item_base + s.item : row);
  return !STREAM || (s.acts() && valid_off + pos < valid_sb);
}

// One 64-token chunk of the inverse-CDF scan: lane l holds the probability p of token c = c0 + l; the first token
// whose cumulative sum exceeds u takes the hit.  (p > 0: the wave scan is not monotone in fp32 -- a lane of probability
// exactly 0, a token the grammar mask forbids, may hold a prefix sum one ulp above its left neighbour's -- so such a
// lane never takes the hit.)
__device__ __forceinline__ void cdf_scan_chunk(float p, int c0, int V, float u, int lane, float& cum, bool& found,
                                               int& pick) {
  float incl = p;                                           // inclusive scan over the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  const bool hit = !found && c0 + lane < V && (cum + incl) > u && p > 0.f;
  const unsigned long long ball = __ballot(hit);
  if (ball && !found) {
    pick = c0 + (int)__builtin_ctzll(ball);
    found = true;
  }
  cum += __shfl(incl, 63, 64);
}

// The plain multinomial draw of one row over the wave: p = exp(x - mx) * inv per token (to probs_row when given), the
// scan chunk by chunk, and the rounding fallback (the sum stayed below u): the last token of nonzero probability -- V - 1,
// unless its logit is -inf (a token the grammar mask forbids) or underflows.  select_token_kernel's and smc_select_kernel's.
__device__ __forceinline__ int multinomial_pick(const float* lr, int V, float mx, float inv, float u, int lane,
                                                float* probs_row) {
  float cum = 0.f;
  int pick = V - 1, lastnz = -1;
  bool found = false;
  for (int c0 = 0; c0 < V; c0 += 64) {
    const int c = c0 + lane;
    float p = c < V ? expf(lr[c] - mx) * inv : 0.f;
    if (p > 0.f) lastnz = c;
    if (probs_row && c < V) probs_row[c] = p;
    cdf_scan_chunk(p, c0, V, u, lane, cum, found, pick);
  }
  if (!found) {
    lastnz = gct_wave_max_i32(lastnz);
    if (lastnz >= 0) pick = lastnz;
  }
  return pick;
}

// The commit: the token, its key-valid flag and the sticky finished flag.
__device__ __forceinline__ void commit_token(int lane, int row, int pos, int tok, int64_t* ys, int64_t ld_ys,
                                             uint8_t* valid, int64_t valid_sb, int valid_off, uint8_t* done,
                                             int64_t pad_id, int64_t eos_id) {
  if (lane != 0) return;
  ys[(int64_t)row * ld_ys + pos] = tok;
  if (valid) valid[(int64_t)row * valid_sb + valid_off + pos] = (tok != pad_id) ? 1 : 0;
  if (done && tok == eos_id) done[row] = 1;
}

// one wave per sample row.  pos_dev (nullable): device-side step counter -- the token is written at ys[.., *pos_dev + 1]
// and valid[.., valid_off + *pos_dev + 1]; seed_dev (nullable) replaces the by-value seed of the multinomial draw.
// RAGGED (pos_dev required) / STREAM (continuous batching, RAGGED required): the row sits at its own position and
// decodes pool item item[r] (select_prologue).  The two select kernels take one parameter list; filt is the other one's.
template <bool RAGGED, bool STREAM>
__global__ __launch_bounds__(256) void select_token_kernel(
    const float* __restrict__ logits, int V, int64_t* ys, int64_t ld_ys, int pos_host, uint8_t* valid, int64_t valid_sb,
    uint8_t* done, float* probs_out, int n, int mode, int64_t pad_id, int64_t eos_id, GctRng rng,
    const int32_t* __restrict__ pos_dev, int valid_off, const uint64_t* __restrict__ seed_dev,
    const int32_t* __restrict__ row_off, const GctSampleFilter* __restrict__ /*filt*/, const int32_t* __restrict__ item,
    const int32_t* __restrict__ prefix_len, int item_base) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  int pos;
  uint32_t key;
  if (!select_prologue<RAGGED, STREAM>(row, n, pos_host, pos_dev, row_off, item, prefix_len, item_base, valid_off,
                                       valid_sb, seed_dev, rng, pos, key))
    return;
  const float* lr = logits + (int64_t)row * V;
  float mx, se;
  gct_wave_softmax_stats(lr, V, lane, mx, se);
  const float inv = 1.0f / se;
  int best = 0;
  if (mode == 0) {
    // greedy: first index of the maximum probability (torch.max semantics)
    float bp = -1.f;
    int bi = 0x7fffffff;
    for (int c = lane; c < V; c += 64) {
      const float p = expf(lr[c] - mx) * inv;
      if (probs_out) probs_out[(int64_t)row * V + c] = p;
      if (p > bp) { bp = p; bi = c; }
    }
    gct_wave_argmax(bp, bi);
    best = bi;
  } else {
    // multinomial: inverse CDF with one Philox uniform per (row, position)
    const uint4 r = gct_philox(rng, key, (uint32_t)pos, 0x452821E6u, 0x38D01377u);
    best = multinomial_pick(lr, V, mx, inv, u01_draw(r.x), lane, probs_out ? probs_out + (int64_t)row * V : nullptr);
  }
  commit_token(lane, row, pos, best, ys, ld_ys, valid, valid_sb, valid_off, done, pad_id, eos_id);
}

// ---------------------------------------------------------------------------------------------- filtered sampling
// The multinomial draw of select_token_kernel with top-k / nucleus / temperature between the softmax and the inverse CDF
// (semantics: decode.py sample_filter_reference).  Settings come from device memory (*filt), so one captured graph serves
// any settings.  One wave per row; lane l holds tokens l + 64 t, t < TPL.  Both filters are "count / mass of the tokens
// with a strictly larger value" per token: TPL == 1 (V <= 64) reads the other tokens with readlane, TPL > 1 stages the
// row in LDS (broadcast reads).  A row the filter leaves unchanged (no token out of the top k or the nucleus) draws with
// the plain kernel's arithmetic -- same softmax, same scan, uniform not rescaled -- so at T = 1 it picks the same token.
// RAGGED / STREAM and the parameter list: as in select_token_kernel (mode is the other kernel's: always 1 here).
template <bool RAGGED, int TPL, bool STREAM>
__global__ __launch_bounds__(256) void select_token_filtered_kernel(
    const float* __restrict__ logits, int V, int64_t* ys, int64_t ld_ys, int pos_host, uint8_t* valid, int64_t valid_sb,
    uint8_t* done, float* probs_out, int n, int /*mode*/, int64_t pad_id, int64_t eos_id, GctRng rng,
    const int32_t* __restrict__ pos_dev, int valid_off, const uint64_t* __restrict__ seed_dev,
    const int32_t* __restrict__ row_off, const GctSampleFilter* __restrict__ filt, const int32_t* __restrict__ item,
    const int32_t* __restrict__ prefix_len, int item_base) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float stage[4][TPL > 1 ? TPL * 64 : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  int pos;
  uint32_t key;
  if (!select_prologue<RAGGED, STREAM>(row, n, pos_host, pos_dev, row_off, item, prefix_len, item_base, valid_off,
                                       valid_sb, seed_dev, rng, pos, key))
    return;
  const int top_k = filt->k;
  const float top_p = filt->top_p, inv_temp = filt->inv_temp;
  const float* lr = logits + (int64_t)row * V;
  float x[TPL], w[TPL];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < TPL; ++t) {
    const int c = lane + 64 * t;
    x[t] = c < V ? lr[c] : -INFINITY;
    mx = fmaxf(mx, x[t]);
  }
  mx = gct_wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int t = 0; t < TPL; ++t) {
    w[t] = lane + 64 * t < V ? expf((x[t] - mx) * inv_temp) : 0.f;
    se += w[t];
  }
  se = gct_wave_sum(se);
  const float inv = 1.0f / se;
#pragma unroll
  for (int t = 0; t < TPL; ++t) w[t] *= inv;                 // p = softmax(x / T), 0 beyond V
  bool changed = false;
  const int Vr = (V + 3) & ~3;                              // LDS reads: float4, padded with values that never count
  if (top_k < V) {                                          // top-k: in iff fewer than k logits are strictly larger
    int cnt[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) cnt[t] = 0;
    if constexpr (TPL == 1) {
      for (int j = 0; j < V; ++j) cnt[0] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[0]), j)) > x[0];
    } else {
#pragma unroll
      for (int t = 0; t < TPL; ++t) stage[wave][lane + 64 * t] = x[t];
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      for (int j = 0; j < Vr; j += 4) {
        const float4 q = *reinterpret_cast<const float4*>(&stage[wave][j]);
#pragma unroll
        for (int t = 0; t < TPL; ++t) cnt[t] += (q.x > x[t]) + (q.y > x[t]) + (q.z > x[t]) + (q.w > x[t]);
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t)
      if (lane + 64 * t < V && cnt[t] >= top_k && x[t] != -INFINITY) {   // (a -inf logit, a token the grammar mask
        w[t] = 1e-6f;                                       // forbids, keeps the weight 0: it never gets the floor)
        changed = true;                                     // the reference's floor (torch.multinomial renormalises)
      }
  }
  if (top_p < 1.f) {                                        // nucleus over s = w / sum w: kept iff the mass of the
    float sw = 0.f;                                         // tokens with a strictly larger s is < top_p
#pragma unroll
    for (int t = 0; t < TPL; ++t) sw += w[t];
    sw = gct_wave_sum(sw);
    const float invw = 1.0f / sw;
    float s[TPL], mass[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      s[t] = w[t] * invw;
      mass[t] = 0.f;
    }
    if constexpr (TPL == 1) {
      for (int j = 0; j < V; ++j) {
        const float sj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s[0]), j));
        mass[0] += sj > s[0] ? sj : 0.f;
      }
    } else {
#pragma unroll
      for (int t = 0; t < TPL; ++t) stage[wave][lane + 64 * t] = s[t];
      __builtin_amdgcn_s_waitcnt(0xC07F);
      __builtin_amdgcn_wave_barrier();
      for (int j = 0; j < Vr; j += 4) {
        const float4 q = *reinterpret_cast<const float4*>(&stage[wave][j]);
#pragma unroll
        for (int t = 0; t < TPL; ++t) {
          mass[t] += q.x > s[t] ? q.x : 0.f;
          mass[t] += q.y > s[t] ? q.y : 0.f;
          mass[t] += q.z > s[t] ? q.z : 0.f;
          mass[t] += q.w > s[t] ? q.w : 0.f;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t)
      if (lane + 64 * t < V && !(mass[t] < top_p)) {
        w[t] = 0.f;
        changed = true;
      }
  }
  changed = __ballot(changed) != 0ull;                      // wave-uniform from here on
  const uint4 r = gct_philox(rng, key, (uint32_t)pos, 0x452821E6u, 0x38D01377u);
  float u = u01_draw(r.x);
  float pscale = 1.f;
  int pick = V - 1, last = -1;
#pragma unroll
  for (int t = 0; t < TPL; ++t)
    if (w[t] > 0.f) last = lane + 64 * t;
  last = gct_wave_max_i32(last);
  if (last >= 0) pick = last;                               // rounding fallback: the last token of nonzero weight
  if (changed) {                                            // draw c with probability w_c / sum w
    float sw = 0.f;
#pragma unroll
    for (int t = 0; t < TPL; ++t) sw += w[t];
    sw = gct_wave_sum(sw);
    u *= sw;
    pscale = 1.0f / sw;
  }
  float cum = 0.f;
  bool found = false;
#pragma unroll
  for (int t = 0; t < TPL; ++t) {
    if (64 * t >= V) break;
    const int c = 64 * t + lane;
    const float p = w[t];
    if (probs_out && c < V) probs_out[(int64_t)row * V + c] = changed ? p * pscale : p;
    cdf_scan_chunk(p, 64 * t, V, u, lane, cum, found, pick);  // (a token of weight 0 is never drawn)
  }
  commit_token(lane, row, pos, pick, ys, ld_ys, valid, valid_sb, valid_off, done, pad_id, eos_id);
}

// ---------------------------------------------------------------------------------------------- grammar mask
// The states GP_* of the SMILES grammar are smiles_grammar.h's (decode.py SmilesGrammar is the statement; the classes are
// GCT_GRAMMAR_*).

// May a row in state (prev, depth, open, here) take a token of class cls (ring number r) when `left` slots remain behind
// it?  The transition must exist and min_finish(state') <= left, with the closed form of min_finish.
__device__ __forceinline__ bool grammar_allows(int prev, int depth, uint64_t open, uint64_t here, int cls, int r,
                                               int left) {
  if (prev == GP_END || left < 0) return cls == GCT_GRAMMAR_PAD;          // finished, or past the budget: pad only
  const bool ar = prev == GP_ATOM || prev == GP_RING, arc = ar || prev == GP_CLOSE;
  int np;
  switch (cls) {
    case GCT_GRAMMAR_ATOM:
      np = GP_ATOM;
      here = 0;
      break;
    case GCT_GRAMMAR_BOND:
      if (ar) np = GP_BOND_A;
      else if (prev == GP_OPEN || prev == GP_CLOSE) np = GP_BOND_B;
      else return false;
      break;
    case GCT_GRAMMAR_OPEN:
      if (!arc) return false;
      np = GP_OPEN;
      ++depth;
      break;
    case GCT_GRAMMAR_CLOSE:
      if (!arc || depth <= 0) return false;
      np = GP_CLOSE;
      --depth;
      break;
    case GCT_GRAMMAR_RING: {
      if (!(ar || prev == GP_BOND_A)) return false;
      const uint64_t bit = 1ull << (r & 63);
      if (open & bit) {
        if (here & bit) return false;                       // a ring does not close on the atom that opened it
        open ^= bit;
      } else {
        open |= bit;
        here |= bit;
      }
      np = GP_RING;
      break;
    }
    case GCT_GRAMMAR_DOT:
      if (!arc || depth != 0) return false;
      np = GP_DOT;
      break;
    case GCT_GRAMMAR_EOS:
      return arc && depth == 0 && open == 0;                // min_finish(END) = 0 <= left
    default:
      return false;
  }
  const bool oh = (open & here) != 0;
  int a;
  if (np == GP_BOND_B || np == GP_OPEN || np == GP_DOT) a = 1;
  else if (np == GP_CLOSE) a = open != 0;
  else if (np == GP_BOND_A) a = open == 0 || oh;
  else a = oh;                                              // ATOM, RING
  return depth + __popcll(open) + 1 + a <= left;
}

// One wave per row, stateless: the row's generated tokens ys[r][t0, p) -- at most 199 under the 200-row positional table,
// 255 at T = 256; lane l holds tokens l + 64 t, four per lane --
// are classified through the table and reduced to the grammar state; then lane l masks tokens l, l + 64, ... of the row's
// logits.  depth = #OPEN - #CLOSE; every RING token toggles its bit, so open = the xor of the ring bits; a ring is in
// `here` iff it appears behind the last ATOM and is open now (its last toggle there was the opening one: closing it
// again on the same atom is what the grammar forbids), so here = open & (or of the ring bits behind the last ATOM).
// ANC (uniform rows of a beam-shaped decode: no row_off, no items): the history view goes through the ancestry map --
// generated token j of row r lies in the physical row kv_src[r][valid_off + t0 + j] that wrote it (KVDecoder._beam_tokens'
// rule; entries clamped to [0, n)), column t0 + j as ever.  Everything behind the view is the one code.
template <bool ANC>
__global__ __launch_bounds__(256) void grammar_mask_kernel(
    const float* __restrict__ logits, float* __restrict__ masked, int V, const int32_t* __restrict__ table,
    const int64_t* __restrict__ ys, int64_t ld_ys, int T, int n, const int32_t* __restrict__ pos_dev,
    const int32_t* __restrict__ row_off, const int32_t* __restrict__ gram, const int32_t* __restrict__ item,
    const int32_t* __restrict__ prefix_len, const int32_t* __restrict__ limit, const int32_t* __restrict__ kv_src,
    int64_t ld_src, int valid_off) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= n) return;
  const int step = *pos_dev + 1;                            // the column the selection behind this launch writes
  const GctRowSlot s = gct_row_slot(step, row, row_off != nullptr, row_off, item != nullptr, item, prefix_len);
  if (s.item < 0) return;                                   // parked (uniform over the wave: a whole wave leaves)
  const int p = s.pos;
  const int t0 = item ? s.t0 : gram[1] - (step - p);        // (gram: the shared prefix width, in the row's own columns)
  const int G = item ? limit[s.item] : gram[0];
  const int g = p - t0;                                     // tokens generated so far
  if (g < 0 || t0 < 0 || p >= T) return;                    // inside the prefix / no such column: 0 <= t0 <= p < T <= 256
  const int64_t* yr = ys + (int64_t)row * ld_ys + t0;
  auto entry = [&](int j) -> int {
    int64_t tok;
    if constexpr (ANC) {
      const int r = kv_src[(int64_t)row * ld_src + valid_off + t0 + j];
      tok = ys[(int64_t)(r < 0 ? 0 : (r >= n ? n - 1 : r)) * ld_ys + t0 + j];
    } else {
      tok = yr[j];
    }
    return tok >= 0 && tok < V ? table[tok] : GCT_GRAMMAR_BANNED;
  };
  int e[4];
  int net = 0, last_atom = -1;
  uint64_t tog = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    e[t] = j < g ? entry(j) : GCT_GRAMMAR_BANNED;
    const int cls = e[t] & 0xFF;
    net += (cls == GCT_GRAMMAR_OPEN) - (cls == GCT_GRAMMAR_CLOSE);
    if (cls == GCT_GRAMMAR_RING) tog ^= 1ull << ((e[t] >> 8) & 63);
    if (cls == GCT_GRAMMAR_ATOM) last_atom = j;
  }
  const int depth = gct_wave_sum(net);
  const uint64_t open = gct_wave_or64(tog, true);
  last_atom = gct_wave_max_i32(last_atom);
  uint64_t behind = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if ((e[t] & 0xFF) == GCT_GRAMMAR_RING && lane + 64 * t > last_atom) behind |= 1ull << ((e[t] >> 8) & 63);
  const uint64_t here = open & gct_wave_or64(behind, false);
  int prev = GP_START;
  if (g > 0) {
    const int c1 = entry(g - 1) & 0xFF, c2 = g > 1 ? entry(g - 2) & 0xFF : GCT_GRAMMAR_BANNED;
    switch (c1) {
      case GCT_GRAMMAR_ATOM: prev = GP_ATOM; break;
      case GCT_GRAMMAR_RING: prev = GP_RING; break;
      case GCT_GRAMMAR_BOND: prev = c2 == GCT_GRAMMAR_ATOM || c2 == GCT_GRAMMAR_RING ? GP_BOND_A : GP_BOND_B; break;
      case GCT_GRAMMAR_OPEN: prev = GP_OPEN; break;
      case GCT_GRAMMAR_CLOSE: prev = GP_CLOSE; break;
      case GCT_GRAMMAR_DOT: prev = GP_DOT; break;
      default: prev = GP_END; break;                        // <eos>, <pad> behind it (or a token no constrained row wrote)
    }
  }
  const int left = G - g - 1;
  const float* lr = logits + (int64_t)row * V;
  float* mr = masked + (int64_t)row * V;
  for (int c = lane; c < V; c += 64) {
    const int en = table[c];
    mr[c] = grammar_allows(prev, depth, open, here, en & 0xFF, (en >> 8) & 63, left) ? lr[c] : -INFINITY;
  }
}

// ---------------------------------------------------------------------------------------------- step statistics
// Behind the selection (decode.py step_stats_reference states the rules): one wave per row, chosen_logp_kernel's slot
// and early returns.  pi = softmax of the RAW logits row, through gct_wave_token_logp (gct_chosen_logp's bits); q = the
// distribution the token was drawn from -- the probs row gct_select_token wrote, pi itself without one, the one-hot at
// the token under greedy.  Lane l handles tokens l, l + 64, ...: one pass over both rows behind the log-softmax's two
// (a row is at most a few KB: it comes from HBM once and from the cache after that; the probs row is read once, the
// chosen token's entry is picked up on the way).  A term with q == 0 (pi == 0) adds exactly 0.
__global__ __launch_bounds__(256) void step_stats_kernel(
    const float* __restrict__ logits, const float* __restrict__ probs, int V, const int64_t* __restrict__ ys,
    int64_t ld_ys, const int32_t* __restrict__ pos, const int32_t* __restrict__ row_off,
    const int32_t* __restrict__ item, const int32_t* __restrict__ prefix_len, int64_t pad_id, int greedy,
    float* __restrict__ model_entropy, float* __restrict__ behaviour_logp, float* __restrict__ behaviour_entropy,
    float* __restrict__ behaviour_kl, int64_t ld_out, int out_rows, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= n) return;
  const GctRowSlot s = gct_row_slot(*pos + 1, row, row_off != nullptr, row_off, item != nullptr, item, prefix_len);
  if (!s.acts()) return;                                    // parked, or a prefix token (uniform: a whole wave leaves)
  const int p = s.pos, dst = s.item;
  if (p < 0 || p >= ld_out || p >= ld_ys || dst >= out_rows) return;
  const int64_t tok64 = ys[(int64_t)row * ld_ys + p];
  float me = 0.f, bl = 0.f, be = 0.f, kl = 0.f;             // pad (a finished row): all four stay 0
  if (gct_token_scored(tok64, pad_id, V)) {
    const int tok = (int)tok64;
    const float* lr = logits + (int64_t)row * V;
    const float* qr = probs && !greedy ? probs + (int64_t)row * V : nullptr;
    bool hit;
    float mx, lse;
    const float lp = gct_wave_token_logp(lr, V, tok, lane, hit, mx, lse);
    float s_pi = 0.f, s_q = 0.f, s_kl = 0.f, qt = 0.f;      // sums of pi log pi, q log q, q (log q - log pi)
    for (int c = lane; c < V; c += 64) {
      const float lpi = (lr[c] - mx) - lse, pi = expf(lpi);
      if (pi != 0.f) s_pi += pi * lpi;
      if (qr) {
        const float q = qr[c];
        if (q > 0.f) {
          const float lq = logf(q);
          s_q += q * lq;
          s_kl += q * (lq - lpi);
        }
        if (c == tok) qt = q;
      }
    }
    me = 0.f - gct_wave_sum(s_pi);
    if (greedy) {                                           // one-hot at tok: log q = 0, H(q) = 0, KL = -log pi(tok)
      kl = 0.f - lp;
    } else if (!qr) {                                       // q = pi
      bl = lp;
      be = me;
    } else {
      bl = logf(__shfl(qt, tok & 63, 64));
      be = 0.f - gct_wave_sum(s_q);
      kl = gct_wave_sum(s_kl);
    }
  }
  if (lane == 0) {
    const int64_t o = (int64_t)dst * ld_out + p;
    if (model_entropy) model_entropy[o] = me;
    if (behaviour_logp) behaviour_logp[o] = bl;
    if (behaviour_entropy) behaviour_entropy[o] = be;
    if (behaviour_kl) behaviour_kl[o] = kl;
  }
}

// ---------------------------------------------------------------------------------------------- continuous batching
// gct_stream_refill, kernel 1 of 2 (decode.py stream_schedule_reference states the rule): one workgroup walks the rows
// in ascending order, 256 at a time.  A row is FINISHED when its item set `done` or produced limit[item] tokens in the
// step just run (its generated length goes to out_len[item]); a finished or empty row WANTS an item.  The wanting rows
// take items next_item, next_item + 1, ... in ascending row order (ballot + prefix count: no race decides it); a row
// that finds the pool empty gets item -1 (parked).  harvest[r] = the item to copy out (-1: none), fresh[r] = the row's
// slots are to be laid out again; the copies are kernel 2's.  *enable == 0: nothing happens.
__global__ __launch_bounds__(256) void stream_scan_kernel(GctStreamState s) {
  if (*s.enable == 0) return;
  __shared__ int wcnt[4], hcnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = (int)s.rows, N = (int)s.items;
  const int p = *s.pos;                                     // index of the token the step just run consumed
  int next = *s.next_item, harvested = 0;
  for (int base = 0; base < R; base += 256) {
    const int r = base + tid;
    bool want = false, harv = false;
    int it = -1;
    if (r < R) {
      it = s.item[r];
      if (it < 0 || it >= N) {
        want = true;
        it = -1;
      } else {
        // tokens generated so far (<= 0: in the prefix): the row's next column (gct_row_slot) less its prefix
        const int gen = gct_row_slot(p + 2, r, true, s.row_off).pos - s.prefix_len[it];
        if (gen > 0 && (s.done[r] != 0 || gen >= s.limit[it])) {
          want = harv = true;
          s.out_len[it] = gen;
        }
      }
    }
    const unsigned long long wb = __ballot(want), hb = __ballot(harv);
    if (lane == 0) {
      wcnt[wave] = __popcll(wb);
      hcnt[wave] = __popcll(hb);
    }
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) before += wcnt[w];
      total += wcnt[w];
      harvested += hcnt[w];
    }
    if (r < R) {
      s.harvest[r] = harv ? it : -1;
      s.fresh[r] = want ? 1 : 0;
      if (want) {
        const int rank = before + __popcll(wb & ((1ull << lane) - 1ull));
        const int ni = next + rank < N ? next + rank : -1;
        s.item[r] = ni;
        if (ni >= 0) {
          s.row_of[ni] = r;
          s.start_step[ni] = p + 1;                         // the shared step that consumes the item's token 0
        }
      }
    }
    next = next + total < N ? next + total : N;
    __syncthreads();                                        // wcnt / hcnt are rewritten by the next 256 rows
  }
  if (tid == 0) {
    *s.next_item = next;
    *s.n_harvested += harvested;
  }
}

// gct_stream_refill, kernel 2 of 2: one workgroup per row.  harvest[r] >= 0: the row's tokens go to out_ys[that item].
// fresh[r]: the row restarts at its own position 0 in the next step (row_off = *pos + 1) -- with a new item its latent
// rows, memory masks and condition rows come from the pools, ys becomes prefix + pad, valid the prefix's flags and
// done 0; a parked row (item -1) gets the offset only, every step, so it stays at position 0 and touches nothing but
// its own slot 0.  Every index is below T (ys, valid), the row's z / mask / condition slots, or the item's pool rows.
__global__ __launch_bounds__(256) void stream_refill_kernel(GctStreamState s) {
  if (*s.enable == 0) return;
  const int r = blockIdx.x, tid = threadIdx.x;
  const int h = s.harvest[r];
  const bool fresh = s.fresh[r] != 0;
  if (h < 0 && !fresh) return;
  int64_t* yr = s.ys + (int64_t)r * s.ld_ys;
  const int W = (int)s.width, T = (int)s.T;
  if (h >= 0) {
    int64_t* orow = s.out_ys + (int64_t)h * W;
    for (int j = tid; j < W; j += 256) orow[j] = yr[j];
  }
  if (!fresh) return;
  __syncthreads();                                          // the row's tokens are out before they are overwritten
  const int it = s.item[r];
  if (tid == 0) s.row_off[r] = *s.pos + 1;
  if (it < 0) return;
  if (tid == 0) {
    s.done[r] = 0;
    s.src_klen[r] = s.klen_pool[it];
  }
  const int plen = s.prefix_len[it];
  const int64_t* pr = s.prefix_pool + (int64_t)it * s.t0_max;
  uint8_t* vr = s.valid + (int64_t)r * s.valid_sb + s.valid_off;
  for (int j = tid; j < T; j += 256) {
    const int64_t tok = j < plen ? pr[j] : s.pad_id;
    yr[j] = tok;
    vr[j] = tok != s.pad_id ? 1 : 0;
  }
  const int Lk = (int)s.Lk;
  for (int j = tid; j < Lk; j += 256) s.src_valid[(int64_t)r * Lk + j] = s.valid_pool[(int64_t)it * Lk + j];
  const int z4 = (int)(s.z_row / 4);
  const float4* zp = reinterpret_cast<const float4*>(s.z_pool + (int64_t)it * s.z_row);
  float4* zr = reinterpret_cast<float4*>(s.z3 + (int64_t)r * s.z_row);
  for (int j = tid; j < z4; j += 256) zr[j] = zp[j];
  const int c4 = (int)(s.ckv_row / 4);
  if (c4 > 0) {
    for (int l = 0; l < (int)s.layers; ++l) {
      const float4* cp = reinterpret_cast<const float4*>(s.ckv_pool[l] + (int64_t)it * s.ckv_row);
      float4* cr = reinterpret_cast<float4*>(s.ckv[l] + (int64_t)r * s.ckv_row);
      for (int j = tid; j < c4; j += 256) cr[j] = cp[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------- beam search
// Candidate order of the selection: higher score first, then the lower flat index beam * V + token.
__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

// One thread's KM best candidates, sorted by their ordering value v; PHI: each carries its score phi beside it.
template <int KM, bool PHI>
struct BeamList {
  float v[KM];
  int i[KM];
  float phi[PHI ? KM : 1];
};

// The new candidate enters at the tail and bubbles up (constant indices: registers).
template <int KM, bool PHI>
__device__ __forceinline__ void beam_insert(BeamList<KM, PHI>& L, float v, int i, float phi) {
  if (!beam_better(v, i, L.v[KM - 1], L.i[KM - 1])) return;
  L.v[KM - 1] = v;
  L.i[KM - 1] = i;
  if constexpr (PHI) L.phi[KM - 1] = phi;
#pragma unroll
  for (int t = KM - 1; t > 0; --t) {
    if (beam_better(L.v[t], L.i[t], L.v[t - 1], L.i[t - 1])) {
      const float tv = L.v[t]; L.v[t] = L.v[t - 1]; L.v[t - 1] = tv;
      const int ti = L.i[t]; L.i[t] = L.i[t - 1]; L.i[t - 1] = ti;
      if constexpr (PHI) { const float tp = L.phi[t]; L.phi[t] = L.phi[t - 1]; L.phi[t - 1] = tp; }
    }
  }
}

// ------------------------------------------------------------------------ rows that share caches by ancestry
// What the selections over a group of K rows behind the map kv_src share (beam_select_kernel's two instantiations and
// smc_select_kernel): the state every one of them keeps per row, and the children's write-back.
// The load: finished / lengths of the group's rows and their map rows -> LDS (the caller's __syncthreads follows).
__device__ __forceinline__ void group_load_state(int tid, int K, int T, int64_t row0, const uint8_t* finished,
                                                 const int32_t* lengths, const int32_t* kv_src, int64_t ld_src,
                                                 uint8_t* s_fin, int32_t* s_len, int32_t (*s_map)[256]) {
  if (tid < K) {
    s_fin[tid] = finished[row0 + tid];
    s_len[tid] = lengths[row0 + tid];
  }
  for (int i = tid; i < K * T; i += 256) {
    const int b = i / T, j = i - b * T;
    s_map[b][j] = kv_src[(row0 + b) * ld_src + j];
  }
}

// Child tid (< K) of parent b: finished, length, parent, the token at ys[row][p] and its flag at valid[row][slot]; the
// parent and the flag stay in LDS for group_write_map.
__device__ __forceinline__ void group_commit_child(int tid, int64_t row, int p, int slot, int b, int tok, bool fin, int len,
                                                   uint8_t* finished, int32_t* lengths, int32_t* parent_out, int64_t* ys,
                                                   int64_t ld_ys, uint8_t* valid, int64_t valid_sb, int64_t pad_id,
                                                   int32_t* s_par, uint8_t* s_cfin) {
  finished[row] = fin ? 1 : 0;
  lengths[row] = len;
  if (parent_out) parent_out[row] = b;
  ys[row * ld_ys + p] = tok;
  valid[row * valid_sb + slot] = tok != pad_id ? 1 : 0;
  s_par[tid] = b;
  s_cfin[tid] = fin ? 1 : 0;
}

// Behind the __syncthreads that follows group_commit_child: child row = parent's map row (as loaded), plus its own new
// slot; done = every child finished.
__device__ __forceinline__ void group_write_map(int tid, int K, int T, int64_t row0, int slot, int32_t* kv_src,
                                                int64_t ld_src, const int32_t (*s_map)[256], const int32_t* s_par,
                                                const uint8_t* s_cfin, uint8_t* done) {
  for (int i = tid; i < K * T; i += 256) {
    const int c = i / T, j = i - c * T;
    kv_src[(row0 + c) * ld_src + j] = j == slot ? (int32_t)(row0 + c) : s_map[s_par[c]][j];
  }
  if (tid == 0) {
    uint8_t all = 1;
    for (int c = 0; c < K; ++c) all &= s_cfin[c];
    done[blockIdx.x] = all;
  }
}

// ------------------------------------------------------------------------ stochastic beam search (gct_beam_select_gumbel)
// What the stochastic instantiation of beam_select_kernel adds (include/gctplus_hip.h states the rules).
struct BeamGumbel {
  float* gumbels;             // [n*K] in place
  GctRng rng;                 // key of (seed, GCT_SBS_SITE)
  const uint64_t* seed_dev;   // nullable: replaces the by-value seed
  const float* noise_in;      // nullable [n*K][V]: these variates instead of the draw
  float* noise_out;           // nullable [n*K][V]: the variates used for live beams
};

// The standard Gumbel variate of (row, token position p, token c): word c & 3 of the call that serves tokens 4 (c >> 2) ..
// 4 (c >> 2) + 3; u = (float32(x >> 9) + 0.5f) * 2^-23 is exact in fp32 and lies strictly inside (0, 1).
__device__ __forceinline__ float sbs_noise(GctRng rng, uint32_t row, uint32_t p, int c, const float* noise_row) {
  if (noise_row) return noise_row[c];
  const uint32_t x = gct_pick(gct_philox(rng, row, p, (uint32_t)c >> 2, GCT_SBS_C3), c & 3);
  const float u = ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f);
  return -logf(-logf(u));
}

// phi = score_b + logp_b(c) and the perturbed value g = phi + noise: THE one evaluation, used by the pass that finds
// Z_b = max g and by the pass that conditions every g on it, so that both see the same bits (additions only, and
// contraction is off in any case: nothing here can be fused differently at the two sites).
__device__ __forceinline__ float sbs_perturbed(float sb, float x, float m, float ls, float noise, float& phi) {
#pragma clang fp contract(off)
  phi = sb + ((x - m) - ls);
  return phi + noise;
}

// g~ = -log(exp(-G) - exp(-Z) + exp(-g)) in the stable form of Kool et al. 2019, appendix B.3.  d is clamped: a
// positive d would make log1mexp a NaN, and a NaN poisons beam_better.
__device__ __forceinline__ float sbs_child_gumbel(float G, float Z, float g) {
  const float d = fminf(g - Z, 0.f);
  const float l = d > -0.69314718f ? logf(-expm1f(d)) : log1pf(-expf(d));      // log(1 - exp(d))
  const float w = (G - g) + l;
  return (G - fmaxf(w, 0.f)) - log1pf(expf(-fabsf(w)));
}

// One workgroup per sample s, whose K beams are rows s*K .. s*K+K-1 (semantics: decode.py beam_step_reference, and
// sbs_step_reference for GUMBEL).
//   1. beam state and the group's kv_src rows -> LDS;
//   2. per live beam (one wave each): m = max logit, ls = log sum exp(x - m); a candidate scores
//      score_b + ((x - m) - ls); a finished beam offers only (score_b, token pad); beams at -inf offer nothing;
//      GUMBEL: the same wave then finds Z_b = max g and its first argmax v*_b over the offered tokens;
//   3. each thread keeps its KM best candidates, then K rounds of a workgroup argmax pop the winners in order; the
//      ordering value is the score, or with GUMBEL the conditioned Gumbel value g~ (v*_b: G_b itself, by its index; a
//      finished beam: G_b) with the score carried beside it;
//   4. child c of parent b: score, finished = fin_b || token == eos, length = len_b + !fin_b, the token at
//      ys[row][p] / valid[row][valid_off + p], and the parent's kv_src row with entry valid_off + p = the child's row.
// p = *pos_dev + 1 (device counter, as select_token_kernel): no host round trip, one captured graph for every step.
template <int KM, bool GUMBEL>
__global__ __launch_bounds__(256) void beam_select_kernel(
    const float* __restrict__ logits, int V, int K, float* __restrict__ scores, uint8_t* __restrict__ finished,
    int32_t* __restrict__ lengths, int32_t* __restrict__ parent_out, int64_t* __restrict__ ys, int64_t ld_ys,
    uint8_t* __restrict__ valid, int64_t valid_sb, int valid_off, int32_t* __restrict__ kv_src, int64_t ld_src, int T,
    uint8_t* __restrict__ done, const int32_t* __restrict__ pos_dev, int64_t pad_id, int64_t eos_id, BeamGumbel sa) {
  constexpr int KG = GUMBEL ? KM : 1;
  __shared__ float s_score[KM], s_m[KM], s_ls[KM], s_winv[KM], s_wv[2][4];
  __shared__ float s_gum[KG], s_z[KG], s_winp[KG];
  __shared__ int32_t s_len[KM], s_win[KM], s_par[KM], s_wi[2][4], s_vstar[KG];
  __shared__ uint8_t s_fin[KM], s_cfin[KM];
  __shared__ int32_t s_map[KM][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = *pos_dev + 1;                               // index of the token chosen now
  const int slot = valid_off + p;
  if (p < 0 || slot >= T) return;                          // no room (the host sizes the caches)
  const int64_t row0 = (int64_t)blockIdx.x * K;
  if constexpr (GUMBEL)
    if (sa.seed_dev) sa.rng = gct_rng_make(*sa.seed_dev, GCT_SBS_SITE);
  if (tid < K) {
    s_score[tid] = scores[row0 + tid];
    if constexpr (GUMBEL) s_gum[tid] = sa.gumbels[row0 + tid];
  }
  group_load_state(tid, K, T, row0, finished, lengths, kv_src, ld_src, s_fin, s_len, s_map);
  __syncthreads();
  for (int b = wave; b < K; b += 4) {                       // log-softmax statistics, one wave per live beam
    if (s_fin[b] || s_score[b] == -INFINITY) continue;
    const float* lr = logits + (row0 + b) * V;
    float m, se;
    gct_wave_softmax_stats(lr, V, lane, m, se);
    if (lane == 0) {
      s_m[b] = m;
      s_ls[b] = logf(se);
    }
    if constexpr (GUMBEL) {                                 // Z_b and v*_b over the offered tokens (phi > -inf)
      const float sb = s_score[b], ls = logf(se);           // (se is the same on every lane: the bits of s_ls[b])
      const float* nr = sa.noise_in ? sa.noise_in + (row0 + b) * V : nullptr;
      float zv = -INFINITY;
      int zi = INT_MAX;
      for (int c = lane; c < V; c += 64) {                  // ascending per lane: > keeps the first
        const float nz = sbs_noise(sa.rng, (uint32_t)(row0 + b), (uint32_t)p, c, nr);
        if (sa.noise_out) sa.noise_out[(row0 + b) * V + c] = nz;
        float phi;
        const float g = sbs_perturbed(sb, lr[c], m, ls, nz, phi);
        if (phi > -INFINITY && (g > zv || zi == INT_MAX)) { zv = g; zi = c; }
      }
      gct_wave_argmax(zv, zi);
      if (lane == 0) {
        s_z[b] = zv;
        s_vstar[b] = zi;
      }
    }
  }
  __syncthreads();
  BeamList<KM, GUMBEL> L;
#pragma unroll
  for (int t = 0; t < KM; ++t) {
    L.v[t] = -INFINITY;
    L.i[t] = INT_MAX;
    if constexpr (GUMBEL) L.phi[t] = -INFINITY;
  }
  for (int b = 0; b < K; ++b) {                             // ascending flat index per thread
    const float sb = s_score[b];
    if (sb == -INFINITY) continue;
    if (s_fin[b]) {
      if (tid == 0) beam_insert<KM, GUMBEL>(L, GUMBEL ? s_gum[GUMBEL ? b : 0] : sb, b * V + (int)pad_id, sb);
      continue;
    }
    const float m = s_m[b], ls = s_ls[b];
    const float* lr = logits + (row0 + b) * V;
    if constexpr (GUMBEL) {
      const float G = s_gum[b], Z = s_z[b];
      const int vs = s_vstar[b];
      if (vs == INT_MAX) continue;                          // every token at -inf: nothing offered
      const float* nr = sa.noise_in ? sa.noise_in + (row0 + b) * V : nullptr;
      for (int c = tid; c < V; c += 256) {
        float phi;
        const float g = sbs_perturbed(sb, lr[c], m, ls, sbs_noise(sa.rng, (uint32_t)(row0 + b), (uint32_t)p, c, nr), phi);
        if (!(phi > -INFINITY)) continue;                   // not offered
        beam_insert<KM, true>(L, c == vs ? G : sbs_child_gumbel(G, Z, g), b * V + c, phi);
      }
    } else {
      for (int c = tid; c < V; c += 256) beam_insert<KM, false>(L, sb + ((lr[c] - m) - ls), b * V + c, 0.f);
    }
  }
  for (int r = 0; r < K; ++r) {                             // K rounds: workgroup argmax of the threads' heads
    float bv = L.v[0];
    int bi = L.i[0];
    gct_wave_argmax(bv, bi);                                // beam_better's order
    if (lane == 0) {
      s_wv[r & 1][wave] = bv;
      s_wi[r & 1][wave] = bi;
    }
    __syncthreads();                                        // (double buffer: round r+1 writes the other slot)
    float wv = s_wv[r & 1][0];
    int wi = s_wi[r & 1][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (beam_better(s_wv[r & 1][w], s_wi[r & 1][w], wv, wi)) { wv = s_wv[r & 1][w]; wi = s_wi[r & 1][w]; }
    if (L.i[0] == wi && wi != INT_MAX) {                    // the owner pops its head
      if constexpr (GUMBEL) s_winp[r] = L.phi[0];
#pragma unroll
      for (int t = 0; t < KM - 1; ++t) {
        L.v[t] = L.v[t + 1];
        L.i[t] = L.i[t + 1];
        if constexpr (GUMBEL) L.phi[t] = L.phi[t + 1];
      }
      L.v[KM - 1] = -INFINITY;
      L.i[KM - 1] = INT_MAX;
    }
    if (tid == 0) {
      s_win[r] = wi;
      s_winv[r] = wv;
    }
  }
  __syncthreads();
  if (tid < K) {
    const int f = s_win[tid];
    const int64_t row = row0 + tid;
    int b, tok;
    float sc, gv;
    if (f == INT_MAX) {                                     // fewer than K candidates (beam search: cannot happen with K <= V)
      b = tid; tok = (int)pad_id; sc = gv = -INFINITY;
    } else {
      b = f / V; tok = f - b * V; gv = s_winv[tid]; sc = GUMBEL ? s_winp[GUMBEL ? tid : 0] : gv;
    }
    const bool fin = f == INT_MAX || s_fin[b] || tok == eos_id;
    scores[row] = sc;
    if constexpr (GUMBEL) sa.gumbels[row] = gv;
    group_commit_child(tid, row, p, slot, b, tok, fin, s_len[b] + (s_fin[b] ? 0 : 1), finished, lengths, parent_out, ys,
                       ld_ys, valid, valid_sb, pad_id, s_par, s_cfin);
  }
  __syncthreads();
  group_write_map(tid, K, T, row0, slot, kv_src, ld_src, s_map, s_par, s_cfin, done);
}

// ---------------------------------------------------------------------------------------------- sequential Monte Carlo
// The K-element arithmetic of one sample, by ONE thread in the stated order (include/gctplus_hip.h, step 2; decode.py
// smc_step_reference): logw[] are the weights after step 1.  Writes the ancestors par[] and the children's log-weights
// cw[]; returns true when it resampled (then *lz_add is the term log_z gains) -- all_dead: every weight is -inf.
// No multiply here may fuse into an add: S2 and the thresholds are compared against a host restatement.
__device__ __forceinline__ bool smc_resample(int K, const float* logw, float tau, float u, float* w, float* cum,
                                             int32_t* par, float* cw, double* lz_add, bool* all_dead) {
#pragma clang fp contract(off)
  float M = -INFINITY;
  for (int b = 0; b < K; ++b) M = fmaxf(M, logw[b]);
  *all_dead = M == -INFINITY;
  bool res = false;
  if (!*all_dead) {
    float S1 = 0.f, S2 = 0.f;
    for (int b = 0; b < K; ++b) {
      w[b] = expf(logw[b] - M);
      S1 += w[b];
      S2 += w[b] * w[b];
      cum[b] = S1;
    }
    const float ess = (S1 * S1) / S2;
    res = tau >= 1.f || ess < tau * (float)K;
    if (res) {
      const float each = S1 / (float)K;
      int last = 0;
      for (int b = 0; b < K; ++b)
        if (w[b] > 0.f) last = b;
      for (int c = 0; c < K; ++c) {
        const float thr = (u + (float)c) * each;
        int a = last;
        for (int b = K - 1; b >= 0; --b)
          if (cum[b] > thr && w[b] > 0.f) a = b;            // the first such b
        par[c] = a;
        cw[c] = 0.f;
      }
      *lz_add = (double)M + log((double)S1 / (double)K);
    }
  }
  if (!res)
    for (int c = 0; c < K; ++c) {
      par[c] = c;
      cw[c] = logw[c];
    }
  return res;
}

// One workgroup per sample s, whose K particles are rows s*K .. s*K+K-1 (semantics: include/gctplus_hip.h
// gct_smc_select; decode.py smc_step_reference).  beam_select_kernel's frame:
//   1. particle state and the group's kv_src rows -> LDS (group_load_state);
//   2. per live particle (one wave each): the softmax statistics of its raw and of its masked row -> the weight;
//   3. thread 0: ESS, the decision, the systematic ancestors, log_z and resamples (smc_resample);
//   4. per child (one wave each): select_token_kernel's multinomial draw from the parent's masked row;
//   5. the write-back (group_commit_child, group_write_map).
template <int KM>
__global__ __launch_bounds__(256) void smc_select_kernel(
    const float* __restrict__ logits, const float* __restrict__ masked, int V, int K, float* __restrict__ logw,
    float* __restrict__ logp, uint8_t* __restrict__ finished, int32_t* __restrict__ lengths,
    int32_t* __restrict__ parent_out, int64_t* __restrict__ ys, int64_t ld_ys, uint8_t* __restrict__ valid,
    int64_t valid_sb, int valid_off, int32_t* __restrict__ kv_src, int64_t ld_src, int T, uint8_t* __restrict__ done,
    const int32_t* __restrict__ pos_dev, int64_t pad_id, int64_t eos_id, double* __restrict__ log_z,
    int32_t* __restrict__ resamples, const float* __restrict__ tau_dev, GctRng rng, GctRng rng_res,
    const uint64_t* __restrict__ seed_dev, const float* __restrict__ u_in, float* __restrict__ u_out) {
  __shared__ float s_logw[KM], s_logp[KM], s_mx[KM], s_lsx[KM], s_my[KM], s_sy[KM], s_w[KM], s_cum[KM], s_cw[KM];
  __shared__ float s_clogp[KM];
  __shared__ int32_t s_len[KM], s_par[KM], s_anc[KM], s_tok[KM], s_clen[KM];
  __shared__ uint8_t s_fin[KM], s_cfin[KM], s_kfin[KM];
  __shared__ int32_t s_map[KM][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = *pos_dev + 1;                               // index of the token chosen now
  const int slot = valid_off + p;
  if (p < 0 || slot >= T) return;                          // no room (the host sizes the caches)
  const int s = blockIdx.x;
  const int64_t row0 = (int64_t)s * K;
  if (seed_dev) {
    rng = gct_rng_make(*seed_dev, 0xDEC0DEu);
    rng_res = gct_rng_make(*seed_dev, GCT_SMC_SITE);
  }
  if (tid < K) {
    s_logw[tid] = logw[row0 + tid];
    s_logp[tid] = logp[row0 + tid];
  }
  group_load_state(tid, K, T, row0, finished, lengths, kv_src, ld_src, s_fin, s_len, s_map);
  __syncthreads();
  for (int b = wave; b < K; b += 4) {                       // step 1, one wave per live particle
    if (s_fin[b]) continue;
    float mx, sx, my, sy;
    gct_wave_softmax_stats(logits + (row0 + b) * V, V, lane, mx, sx);
    gct_wave_softmax_stats(masked + (row0 + b) * V, V, lane, my, sy);
    if (lane == 0) {
      const float lsx = logf(sx);
      s_mx[b] = mx;
      s_lsx[b] = lsx;
      s_my[b] = my;
      s_sy[b] = sy;
      s_logw[b] = my == -INFINITY ? -INFINITY : s_logw[b] + ((my - mx) + (logf(sy) - lsx));
    }
  }
  __syncthreads();
  if (tid == 0) {                                           // steps 0 and 2
    bool idle = true;
    for (int b = 0; b < K; ++b) idle = idle && s_fin[b] != 0;
    const float u = u_in ? u_in[(int64_t)s * (K + 1) + K]
                         : u01_draw(gct_philox(rng_res, (uint32_t)s, (uint32_t)p, 0x452821E6u, 0x38D01377u).x);
    if (u_out) u_out[(int64_t)s * (K + 1) + K] = u;
    if (idle) {
      for (int c = 0; c < K; ++c) {
        s_anc[c] = c;
        s_cw[c] = s_logw[c];
      }
    } else {
      double add = 0.0;
      bool all_dead;
      if (smc_resample(K, s_logw, *tau_dev, u, s_w, s_cum, s_anc, s_cw, &add, &all_dead)) {
        log_z[s] += add;
        resamples[s] += 1;
      }
      if (all_dead) log_z[s] = -INFINITY;
    }
  }
  __syncthreads();
  for (int c = wave; c < K; c += 4) {                       // step 3, one wave per child
    const int a = s_anc[c];
    const int64_t row = row0 + c;
    const float u = u_in ? u_in[(int64_t)s * (K + 1) + c]
                         : u01_draw(gct_philox(rng, (uint32_t)row, (uint32_t)p, 0x452821E6u, 0x38D01377u).x);
    int tok = (int)pad_id, len = s_len[a];
    float lp = s_logp[a], cw = s_cw[c];
    bool fin = true;
    if (!s_fin[a] && s_logw[a] == -INFINITY) {              // dead: pad, finished from now on
      cw = -INFINITY;
    } else if (!s_fin[a]) {
      const float* xr = logits + (row0 + a) * V;
      tok = multinomial_pick(masked + (row0 + a) * V, V, s_my[a], 1.0f / s_sy[a], u, lane, nullptr);
      lp = lp + ((xr[tok] - s_mx[a]) - s_lsx[a]);
      fin = tok == eos_id;
      len += 1;
    }
    if (lane == 0) {
      if (u_out) u_out[(int64_t)s * (K + 1) + c] = u;
      s_tok[c] = tok;
      s_clogp[c] = lp;
      s_cw[c] = cw;
      s_kfin[c] = fin ? 1 : 0;
      s_clen[c] = len;
    }
  }
  __syncthreads();
  if (tid < K) {
    const int64_t row = row0 + tid;
    logw[row] = s_cw[tid];
    logp[row] = s_clogp[tid];
    group_commit_child(tid, row, p, slot, s_anc[tid], s_tok[tid], s_kfin[tid] != 0, s_clen[tid], finished, lengths,
                       parent_out, ys, ld_ys, valid, valid_sb, pad_id, s_par, s_cfin);
  }
  __syncthreads();
  group_write_map(tid, K, T, row0, slot, kv_src, ld_src, s_map, s_par, s_cfin, done);
}

// ---------------------------------------------------------------------------------------------- launches
// Compile-time dispatch on a run-time value: f gets std::integral_constant<int, v> for the first listed value equal
// to v, the last listed one otherwise.
template <int A, int... Rest, class F>
void with_int(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, A>{});
  else if (v == A) f(std::integral_constant<int, A>{});
  else with_int<Rest...>(v, f);
}

// The one launch of attn_decode_kernel.  The entry points have checked what is theirs and decided which optional
// pointer is set: klen only without pos, kv_src only when mapped (beam search), row_off only when ragged.
int launch_attn_decode(const char* who, const float* q, int64_t ldq, float* k, float* v, int64_t kv_row, int64_t kv_batch,
                       const uint8_t* valid, int64_t valid_sb, float* o, int64_t ldo, int n, int H, int Lc, int dk,
                       float scale, const int32_t* pos, int cache_off, const float* knew, const float* vnew, int64_t ldn,
                       const int32_t* klen, const int32_t* kv_src, int64_t ld_src, const int32_t* row_off, void* stream) {
  GCT_CHECK_ARG(dk == 16 || dk == 32 || dk == 64, "%s: head dim %d unsupported", who, dk);
  GCT_CHECK_ARG(ldq % 4 == 0 && kv_row % 4 == 0 && kv_batch % 4 == 0 && gct_aligned16(q) && gct_aligned16(k) &&
                    gct_aligned16(v),
                "%s: operands must be 16-B aligned", who);
  if (n == 0) return GCT_OK;
  const dim3 grid((unsigned)(((int64_t)n * H + 3) / 4));
  with_int<64, 32, 16>(dk, [&](auto DK) {
    with_int<2, 1, 0>(kv_src ? 2 : (row_off ? 1 : 0), [&](auto ROWS) {      // 2 mapped, 1 ragged, 0 plain
      hipLaunchKernelGGL((attn_decode_kernel<DK, ROWS == 2, ROWS == 1>), grid, dim3(256), 0, (hipStream_t)stream, q, ldq,
                         k, v, kv_row, kv_batch, valid, valid_sb, o, ldo, n, H, Lc, scale, pos, cache_off, knew, vnew,
                         ldn, klen, kv_src, ld_src, row_off);
    });
  });
  GCT_LAUNCH_CHECK(who);
  return GCT_OK;
}

}  // namespace

extern "C" int gct_attn_decode(const float* q, int64_t ldq, float* k, float* v,
                               int64_t kv_row, int64_t kv_batch, const uint8_t* valid,
                               int64_t valid_sb, float* o, int64_t ldo, int n, int H, int Lc, int dk,
                               float scale, const int32_t* pos, int cache_off, const float* knew,
                               const float* vnew, int64_t ldn, const int32_t* klen, const int32_t* row_off,
                               void* stream) {
  GCT_CHECK_ARG(q && k && v && o && n >= 0 && H > 0 && Lc >= 0 && Lc <= 256, "attn_decode: bad args");
  GCT_CHECK_ARG(!row_off || pos, "attn_decode: row_off needs the device-position form");
  GCT_CHECK_ARG(!(klen && pos), "attn_decode: klen is for a fixed cache (cross-attention), not the device-position form");
  GCT_CHECK_ARG(pos || Lc > 0, "attn_decode: no keys");
  GCT_CHECK_ARG(!pos || (knew && vnew && ldn % 4 == 0 && gct_aligned16(knew) && gct_aligned16(vnew) && cache_off >= 0),
                "attn_decode: the device-position form needs this step's key / value rows");
  return launch_attn_decode("attn_decode", q, ldq, k, v, kv_row, kv_batch, valid, valid_sb, o, ldo, n, H, Lc, dk, scale, pos,
                            cache_off, knew, vnew, ldn, klen, nullptr, 0, row_off, stream);
}

extern "C" int gct_attn_decode_z(const float* q, int64_t ldq, int qoff, const float* z, int64_t z_batch, int lat, int Le,
                                 const float* ckv, int64_t ckv_batch, int64_t ld_ckv, int nc, const uint8_t* valid,
                                 int64_t valid_sb, const int32_t* klen, float* out, int64_t ldo, int ooff, int n, int H,
                                 int dk, float scale, void* stream) {
  GCT_CHECK_ARG(q && z && out && n >= 0 && H > 0 && dk > 0 && Le >= 0 && nc >= 0 && nc + Le > 0 && nc + Le <= 259,
                "attn_decode_z: bad args");
  GCT_CHECK_ARG(lat > 0 && lat % 4 == 0 && lat <= 128 && Le <= 256, "attn_decode_z: latent size %d / %d rows unsupported", lat, Le);
  GCT_CHECK_ARG(nc == 0 || (ckv && ld_ckv >= 2 * (int64_t)H * dk), "attn_decode_z: condition rows without their keys / values");
  GCT_CHECK_ARG(ldq % 4 == 0 && qoff % 4 == 0 && ooff % 4 == 0 && ldo % 4 == 0 && z_batch % 4 == 0 && gct_aligned16(q) &&
                    gct_aligned16(z) && gct_aligned16(out),
                "attn_decode_z: operands must be 16-B aligned");
  if (n == 0) return GCT_OK;
  const size_t lds = ((size_t)Le * (lat + 4) + (size_t)H * lat + (size_t)H * ((nc + Le + 3) & ~3)) * sizeof(float);
  GCT_CHECK_ARG(lds <= 160 * 1024, "attn_decode_z: %zu bytes of LDS needed", lds);
  static size_t lds_set = 0;
  if (lds > 48 * 1024 && lds > lds_set) {
    hipError_t e = hipFuncSetAttribute((const void*)attn_decode_z_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024));
    if (e != hipSuccess) {
      gct_set_error("attn_decode_z: cannot reserve LDS: %s", hipGetErrorString(e));
      return GCT_ERR_HIP;
    }
    lds_set = 160 * 1024;
  }
  hipLaunchKernelGGL(attn_decode_z_kernel, dim3((unsigned)n), dim3(256), lds, (hipStream_t)stream, q, ldq, qoff, z, z_batch,
                     lat, Le, ckv, ckv_batch, ld_ckv, nc, H * dk, valid, valid_sb, klen, out, ldo, ooff, H, dk, scale);
  GCT_LAUNCH_CHECK("attn_decode_z");
  return GCT_OK;
}

extern "C" int gct_decode_embed(const int64_t* ys, int64_t ld_ys, const int32_t* pos, int pe_off, const float* table,
                                int vocab, const float* pe, float* out, int n, int d, float scale,
                                const int32_t* row_off, void* stream) {
  GCT_CHECK_ARG(ys && pos && table && pe && out && n >= 0 && d > 0 && d % 4 == 0 && vocab > 0 && pe_off >= 0 &&
                    gct_aligned16(table) && gct_aligned16(pe) && gct_aligned16(out),
                "decode_embed: bad args");
  if (n == 0) return GCT_OK;
  const dim3 grid((unsigned)(((int64_t)n * (d / 4) + 255) / 256));
  with_int<1, 0>(row_off != nullptr, [&](auto RAGGED) {
    hipLaunchKernelGGL(decode_embed_kernel<RAGGED != 0>, grid, dim3(256), 0, (hipStream_t)stream, ys, ld_ys, pos, pe_off,
                       table, vocab, pe, out, n, d, scale, row_off);
  });
  GCT_LAUNCH_CHECK("decode_embed");
  return GCT_OK;
}

extern "C" int gct_decode_advance(int32_t* pos, void* stream) {
  GCT_CHECK_ARG(pos, "decode_advance: null pointer");
  hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, pos);
  GCT_LAUNCH_CHECK("decode_advance");
  return GCT_OK;
}

extern "C" int gct_select_token(const float* logits, int V, int64_t* ys, int64_t ld_ys, int pos,
                                uint8_t* valid, int64_t valid_sb, uint8_t* done, float* probs_out,
                                int n, int mode, int64_t pad_id, int64_t eos_id, uint64_t seed,
                                const int32_t* pos_dev, int valid_off, const uint64_t* seed_dev,
                                const int32_t* row_off, const GctSampleFilter* filt, const int32_t* item,
                                const int32_t* prefix_len, int item_base, void* stream) {
  GCT_CHECK_ARG(logits && ys && V > 0 && n >= 0 && pos >= 0 && (mode == 0 || mode == 1) && valid_off >= 0,
                "select_token: bad args");
  GCT_CHECK_ARG(!row_off || pos_dev, "select_token: row_off needs the device position");
  GCT_CHECK_ARG(!filt || mode == 1, "select_token: the sampling filter is for the multinomial mode");
  GCT_CHECK_ARG(!filt || V <= GCT_SAMPLE_FILTER_MAX_VOCAB, "select_token: the sampling filter supports up to %d tokens, "
                "not %d", GCT_SAMPLE_FILTER_MAX_VOCAB, V);
  GCT_CHECK_ARG(!item == !prefix_len && (!item || (row_off && valid && done && item_base >= 0)),
                "select_token: streamed rows need item, prefix_len, row_off, valid and done");
  if (n == 0) return GCT_OK;
  const GctRng rng = gct_rng_make(seed, 0xDEC0DEu);
  constexpr int TPL = GCT_SAMPLE_FILTER_MAX_VOCAB / 64;
  // streamed rows (item set, hence row_off) are ragged rows; the filter keeps 0 (none: the plain kernel), 1 or TPL
  // tokens per lane.  Plain rows are keyed by the row alone, whatever item_base says.
  with_int<2, 1, 0>(item ? 2 : (row_off ? 1 : 0), [&](auto ROWS) {
    with_int<0, 1, TPL>(!filt ? 0 : (V <= 64 ? 1 : TPL), [&](auto PER_LANE) {
      auto kernel = select_token_kernel<ROWS != 0, ROWS == 2>;
      if constexpr (PER_LANE != 0) kernel = select_token_filtered_kernel<ROWS != 0, PER_LANE, ROWS == 2>;
      hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, V, ys, ld_ys,
                         pos, valid, valid_sb, done, probs_out, n, mode, pad_id, eos_id, rng, pos_dev, valid_off,
                         seed_dev, row_off, filt, item, prefix_len, item ? item_base : 0);
    });
  });
  GCT_LAUNCH_CHECK("select_token");
  return GCT_OK;
}

extern "C" int gct_grammar_mask(const float* logits, float* masked, int V, const int32_t* table, const int64_t* ys,
                                int64_t ld_ys, int T, int n, const int32_t* pos, const int32_t* row_off,
                                const int32_t* gram, const int32_t* item, const int32_t* prefix_len,
                                const int32_t* limit, void* stream) {
  GCT_CHECK_ARG(logits && masked && logits != masked && table && ys && pos && V > 0 && n >= 0, "grammar_mask: bad args");
  GCT_CHECK_ARG(T >= 1 && T <= 256 && ld_ys >= T, "grammar_mask: %d token columns (1 .. 256) in rows of %lld", T,
                (long long)ld_ys);
  GCT_CHECK_ARG(!item == !prefix_len && !item == !limit && (!item || row_off),
                "grammar_mask: streamed rows need item, prefix_len, limit and row_off");
  GCT_CHECK_ARG(item || gram, "grammar_mask: no budget (gram, or the stream's limit)");
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(grammar_mask_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits,
                     masked, V, table, ys, ld_ys, T, n, pos, row_off, gram, item, prefix_len, limit, nullptr, 0, 0);
  GCT_LAUNCH_CHECK("grammar_mask");
  return GCT_OK;
}

extern "C" int gct_grammar_mask_anc(const float* logits, float* masked, int V, const int32_t* table, const int64_t* ys,
                                    int64_t ld_ys, int T, int n, const int32_t* pos, const int32_t* gram,
                                    const int32_t* kv_src, int64_t ld_src, int valid_off, void* stream) {
  GCT_CHECK_ARG(logits && masked && logits != masked && table && ys && pos && gram && kv_src && V > 0 && n >= 0,
                "grammar_mask_anc: bad args");
  GCT_CHECK_ARG(T >= 1 && T <= 256 && ld_ys >= T, "grammar_mask_anc: %d token columns (1 .. 256) in rows of %lld", T,
                (long long)ld_ys);
  GCT_CHECK_ARG(valid_off >= 0 && ld_src >= (int64_t)valid_off + T, "grammar_mask_anc: map rows of %lld entries for %d + %d",
                (long long)ld_src, valid_off, T);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(grammar_mask_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits,
                     masked, V, table, ys, ld_ys, T, n, pos, nullptr, gram, nullptr, nullptr, nullptr, kv_src, ld_src,
                     valid_off);
  GCT_LAUNCH_CHECK("grammar_mask_anc");
  return GCT_OK;
}

extern "C" int gct_step_stats(const float* logits, const float* probs, int V, const int64_t* ys, int64_t ld_ys,
                              const int32_t* pos, const int32_t* row_off, const int32_t* item,
                              const int32_t* prefix_len, int64_t pad_id, int greedy, float* model_entropy,
                              float* behaviour_logp, float* behaviour_entropy, float* behaviour_kl, int64_t ld_out,
                              int out_rows, int n, void* stream) {
  GCT_CHECK_ARG(logits && ys && pos && n >= 0 && V >= 1 && ld_ys > 0 && ld_out > 0 && out_rows >= 0,
                "step_stats: bad args");
  GCT_CHECK_ARG(model_entropy || behaviour_logp || behaviour_entropy || behaviour_kl,
                "step_stats: all four outputs are null");
  GCT_CHECK_ARG(!item == !prefix_len && (!item || row_off), "step_stats: streamed rows need item, prefix_len and row_off");
  GCT_CHECK_ARG(item || out_rows >= n, "step_stats: %d output rows for %d decode rows", out_rows, n);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(step_stats_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, logits, probs,
                     V, ys, ld_ys, pos, row_off, item, prefix_len, pad_id, greedy, model_entropy, behaviour_logp,
                     behaviour_entropy, behaviour_kl, ld_out, out_rows, n);
  GCT_LAUNCH_CHECK("step_stats");
  return GCT_OK;
}

// Continuous batching: harvest the rows that finished in the step just run and hand them the next pool items.
extern "C" int gct_stream_refill(const GctStreamState* state, void* stream) {
  GCT_CHECK_ARG(state, "stream_refill: null state");
  const GctStreamState& s = *state;
  GCT_CHECK_ARG(s.ys && s.valid && s.done && s.row_off && s.pos && s.z3 && s.src_valid && s.src_klen && s.item &&
                    s.harvest && s.fresh && s.z_pool && s.valid_pool && s.klen_pool && s.prefix_pool && s.prefix_len &&
                    s.limit && s.out_ys && s.out_len && s.row_of && s.start_step && s.next_item && s.n_harvested &&
                    s.enable,
                "stream_refill: null pointer");
  GCT_CHECK_ARG(s.rows >= 1 && s.rows <= GCT_STREAM_MAX_ROWS && s.items >= 0 && s.items <= INT_MAX - 256,
                "stream_refill: %lld rows (1 .. %d) / %lld items", (long long)s.rows, GCT_STREAM_MAX_ROWS,
                (long long)s.items);
  GCT_CHECK_ARG(s.T >= 1 && s.width >= 1 && s.width <= s.T && s.ld_ys >= s.T && s.valid_sb >= s.valid_off + s.T &&
                    s.valid_off >= 0 && s.t0_max >= 1 && s.t0_max <= s.width,
                "stream_refill: row width %lld / cache rows %lld / prefix width %lld", (long long)s.width,
                (long long)s.T, (long long)s.t0_max);
  GCT_CHECK_ARG(s.z_row >= 0 && s.z_row % 4 == 0 && gct_aligned16(s.z3) && gct_aligned16(s.z_pool) && s.Lk >= 1,
                "stream_refill: the latent rows must be 16-B aligned");
  GCT_CHECK_ARG(s.layers >= 0 && s.layers <= GCT_STREAM_MAX_LAYERS && s.ckv_row >= 0 && s.ckv_row % 4 == 0,
                "stream_refill: %lld layers of condition rows (at most %d)", (long long)s.layers, GCT_STREAM_MAX_LAYERS);
  for (int l = 0; l < (int)s.layers && s.ckv_row > 0; ++l)
    GCT_CHECK_ARG(s.ckv[l] && s.ckv_pool[l] && gct_aligned16(s.ckv[l]) && gct_aligned16(s.ckv_pool[l]),
                  "stream_refill: condition rows of layer %d missing or not 16-B aligned", l);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(stream_scan_kernel, dim3(1), dim3(256), 0, st, s);
  hipLaunchKernelGGL(stream_refill_kernel, dim3((unsigned)s.rows), dim3(256), 0, st, s);
  GCT_LAUNCH_CHECK("stream_refill");
  return GCT_OK;
}

extern "C" int gct_attn_decode_beam(const float* q, int64_t ldq, float* k, float* v, int64_t kv_row, int64_t kv_batch,
                                    const uint8_t* valid, int64_t valid_sb, float* o, int64_t ldo, int n, int H, int T,
                                    int dk, float scale, const int32_t* pos, int cache_off, const float* knew,
                                    const float* vnew, int64_t ldn, const int32_t* kv_src, int64_t ld_src,
                                    void* stream) {
  GCT_CHECK_ARG(q && k && v && o && pos && kv_src && n >= 0 && H > 0 && T > 0 && T <= 256 && ld_src >= T &&
                    cache_off >= 0,
                "attn_decode_beam: bad args");
  GCT_CHECK_ARG(knew && vnew && ldn % 4 == 0 && gct_aligned16(knew) && gct_aligned16(vnew),
                "attn_decode_beam: needs this step's key / value rows");
  return launch_attn_decode("attn_decode_beam", q, ldq, k, v, kv_row, kv_batch, valid, valid_sb, o, ldo, n, H, T, dk, scale,
                            pos, cache_off, knew, vnew, ldn, nullptr, kv_src, ld_src, nullptr, stream);
}

// The one launch of beam_select_kernel: gct_beam_select's checks, which gct_beam_select_gumbel shares.
template <bool GUMBEL>
static int launch_beam_select(const char* name, const float* logits, int V, int n, int k, float* scores, uint8_t* finished,
                              int32_t* lengths, int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid,
                              int64_t valid_sb, int valid_off, int32_t* kv_src, int64_t ld_src, int T, uint8_t* done,
                              const int32_t* pos_dev, int64_t pad_id, int64_t eos_id, const BeamGumbel& sa, void* stream) {
  GCT_CHECK_ARG(logits && scores && finished && lengths && ys && valid && kv_src && done && pos_dev && n >= 0 &&
                    (!GUMBEL || sa.gumbels),
                "%s: bad args", name);
  GCT_CHECK_ARG(k >= 1 && k <= GCT_BEAM_MAX_K && V >= k && V <= GCT_BEAM_MAX_VOCAB,
                "%s: beam size %d / vocabulary %d unsupported", name, k, V);
  GCT_CHECK_ARG(T > 0 && T <= 256 && valid_off >= 0 && valid_off < T && ld_src >= T && valid_sb >= T &&
                    ld_ys >= T - valid_off,
                "%s: cache rows %d / map %lld / valid %lld / ys %lld", name, T, (long long)ld_src,
                (long long)valid_sb, (long long)ld_ys);
  GCT_CHECK_ARG(pad_id >= 0 && pad_id < V, "%s: pad id %lld outside the vocabulary", name, (long long)pad_id);
  if (n == 0) return GCT_OK;
  with_int<4, 8, 16>(k <= 4 ? 4 : (k <= 8 ? 8 : 16), [&](auto KM) {
    hipLaunchKernelGGL((beam_select_kernel<KM, GUMBEL>), dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, logits, V,
                       k, scores, finished, lengths, parent, ys, ld_ys, valid, valid_sb, valid_off, kv_src, ld_src, T,
                       done, pos_dev, pad_id, eos_id, sa);
  });
  GCT_LAUNCH_CHECK(name);
  return GCT_OK;
}

extern "C" int gct_beam_select(const float* logits, int V, int n, int k, float* scores, uint8_t* finished,
                               int32_t* lengths, int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid,
                               int64_t valid_sb, int valid_off, int32_t* kv_src, int64_t ld_src, int T, uint8_t* done,
                               const int32_t* pos_dev, int64_t pad_id, int64_t eos_id, void* stream) {
  return launch_beam_select<false>("beam_select", logits, V, n, k, scores, finished, lengths, parent, ys, ld_ys, valid,
                                   valid_sb, valid_off, kv_src, ld_src, T, done, pos_dev, pad_id, eos_id, BeamGumbel{},
                                   stream);
}

extern "C" int gct_beam_select_gumbel(const float* logits, int V, int n, int k, float* scores, uint8_t* finished,
                                      int32_t* lengths, int32_t* parent, int64_t* ys, int64_t ld_ys, uint8_t* valid,
                                      int64_t valid_sb, int valid_off, int32_t* kv_src, int64_t ld_src, int T,
                                      uint8_t* done, const int32_t* pos_dev, int64_t pad_id, int64_t eos_id,
                                      float* gumbels, uint64_t seed, const uint64_t* seed_dev, const float* noise_in,
                                      float* noise_out, void* stream) {
  const BeamGumbel sa{gumbels, gct_rng_make(seed, GCT_SBS_SITE), seed_dev, noise_in, noise_out};
  return launch_beam_select<true>("beam_select_gumbel", logits, V, n, k, scores, finished, lengths, parent, ys, ld_ys,
                                  valid, valid_sb, valid_off, kv_src, ld_src, T, done, pos_dev, pad_id, eos_id, sa, stream);
}

// Sequential Monte Carlo under the grammar: gct_beam_select's geometry checks, with the particle state in place of the
// beam scores (include/gctplus_hip.h states the step).
extern "C" int gct_smc_select(const float* logits, const float* masked, int V, int n, int k, float* logw, float* logp,
                              uint8_t* finished, int32_t* lengths, int32_t* parent, int64_t* ys, int64_t ld_ys,
                              uint8_t* valid, int64_t valid_sb, int valid_off, int32_t* kv_src, int64_t ld_src, int T,
                              uint8_t* done, const int32_t* pos_dev, int64_t pad_id, int64_t eos_id, double* log_z,
                              int32_t* resamples, const float* tau_dev, uint64_t seed, const uint64_t* seed_dev,
                              const float* u_in, float* u_out, void* stream) {
  GCT_CHECK_ARG(logits && masked && masked != logits && logw && logp && finished && lengths && ys && valid && kv_src &&
                    done && pos_dev && log_z && resamples && tau_dev && n >= 0,
                "smc_select: bad args");
  GCT_CHECK_ARG(k >= 1 && k <= GCT_BEAM_MAX_K && V >= 1, "smc_select: %d particles / vocabulary %d unsupported", k, V);
  GCT_CHECK_ARG(T > 0 && T <= 256 && valid_off >= 0 && valid_off < T && ld_src >= T && valid_sb >= T &&
                    ld_ys >= T - valid_off,
                "smc_select: cache rows %d / map %lld / valid %lld / ys %lld", T, (long long)ld_src, (long long)valid_sb,
                (long long)ld_ys);
  GCT_CHECK_ARG(pad_id >= 0 && pad_id < V, "smc_select: pad id %lld outside the vocabulary", (long long)pad_id);
  if (n == 0) return GCT_OK;
  const GctRng rng = gct_rng_make(seed, 0xDEC0DEu), rng_res = gct_rng_make(seed, GCT_SMC_SITE);
  with_int<4, 8, 16>(k <= 4 ? 4 : (k <= 8 ? 8 : 16), [&](auto KM) {
    hipLaunchKernelGGL(smc_select_kernel<KM>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, logits, masked, V, k,
                       logw, logp, finished, lengths, parent, ys, ld_ys, valid, valid_sb, valid_off, kv_src, ld_src, T,
                       done, pos_dev, pad_id, eos_id, log_z, resamples, tau_dev, rng, rng_res, seed_dev, u_in, u_out);
  });
  GCT_LAUNCH_CHECK("smc_select");
  return GCT_OK;
}
