// Murcko scaffolds on the device: gct_smiles_scaffold against scaffold.py SmilesScaffolds (scaffold is the statement for
// one part, scaffold_reference the batch rule).  One wave per row, four rows per workgroup, in smiles_key_kernel's shape:
// lane l stages tokens l + 64 t of the row's span -- the table word and the token's 64-bit label -- in the wave's own LDS
// and the wave finds the first <eos> and the first <sep> in front of it.  The part in front of the <sep> (the scaffold the
// row was given) gets gct_smiles_key's path, unchanged.  The molecule goes through
//   lane 0    the parse (rand_parse of smiles_graph.h);
//   lanes     bond labels; member = 1 and the live degree of every atom;
//   lane 0    the peel: a worklist of atoms with at most one live neighbour -- an atom enters it once, when its live
//             degree is at most 1 at the start or falls to 1, so a chain of 255 atoms costs 255 pops;
//   lanes     shell marks over the bonds (label 2 between a core atom and a dropped one), then over the atoms the [nH]
//             rule: a kept bare `n` that loses a neighbour takes [nH]'s label and aromatic bit;
//   lane 0    compaction of atoms, bonds and bond lists to the kept ones, ascending and in place;
//   lanes     key_bond_label / key_profile / key_refine / key_wave_sum exactly as gct_smiles_key runs them;
//   lane 0    rand_walk from atom 0 into the LDS row (smiles_walk.h);
// and all lanes write tokens, member, key and info.  No atomics; nothing per-lane is indexed at run time in registers.
// LDS: a record is KeyWave's size (13 088 bytes: 6 656 the parsed graph, 2 048 the labels, 4 096 the colour buffers, 256
// the bond labels, 32 the header), 52 352 per workgroup of four rows -- three workgroups per CU, as gct_smiles_key has.
// Two things keep it there.  The walk's buffers (the output row, seen / pbond / left, role / rnum, perm: 2 560 bytes)
// alias the colour buffers, which are done with when the wave sum is taken.  And what only the parse needs of
// SmilesGraph is free behind it: par[a] holds member[a] by INPUT atom index to the end, stamp[a] the live degree during
// the peel and then the atom's new index, stk the worklist, then bond -> new bond, then the walk's stack.
#include "smiles_key.h"
#include "smiles_walk.h"

namespace {

constexpr int kBareN = 1 << 25, kSubst = 1 << 26;            // bits of e[i] beside the table word and <sep> << 24

struct ScaWave : SmilesGraph {                               // e[i]: as KeyWave's | kBareN (the token is `n`) | kSubst
  uint64_t lab[256];                                         //  (the atom is spelled [nH])
  union {
    uint64_t col[2][256];                                    // the key's colours, then the walk's:
    struct {
      int32_t out[256];
      uint8_t seen[256], pbond[256], left[256];
      uint8_t role[256], rnum[256];
      uint8_t perm[256];
    };
  };
  uint8_t blab[256];
  int32_t res[8];                                            // graph?, atoms, bonds, core atoms, input atoms
};
static_assert(sizeof(ScaWave) * 4 <= 64 * 1024, "four rows per workgroup must fit 64 KB of LDS");
static_assert(sizeof(ScaWave) * 4 * 3 <= 160 * 1024, "three workgroups per CU");

// Lane 0: the core of a parsed part of A atoms.  In: par[a] = 1, stamp[a] = deg[a].  Out: par[a] = 0 on every atom that
// is not on a ring or between two; returns the number of atoms left.
template <class Rec>
__host__ __device__ inline int sca_peel(Rec& w, int A) {
  int sp = 0, core = A;
  for (int a = 0; a < A; ++a)
    if (w.stamp[a] <= 1) w.stk[sp++] = (uint16_t)a;          // (every atom is pushed at most once: sp <= A <= 255)
  while (sp > 0) {
    const int a = w.stk[--sp];
    w.par[a] = 0;
    --core;
    const int d = w.deg[a];
    for (int i = 0; i < d; ++i) {
      const int e = w.adj[a][i], v = w.ba[e] ^ w.bb[e] ^ a;
      if (w.par[v] && --w.stamp[v] == 1) w.stk[sp++] = (uint16_t)v;   // (a live v has a live neighbour: stamp[v] >= 1)
    }
  }
  return core;
}

// A lane's bond e: the shell mark.  (Lanes race only to write the same 2, and test `== 1`, which no lane writes.)
template <class Rec>
__host__ __device__ inline void sca_shell(Rec& w, int e) {
  if (w.blab[e] != 2) return;
  const int a = w.ba[e], b = w.bb[e];
  const bool ca = w.par[a] == 1, cb = w.par[b] == 1;
  if (ca && !cb) w.par[b] = 2;
  if (cb && !ca) w.par[a] = 2;
}

// A lane's atom a: the [nH] rule.  Returns true when the atom needs the token and the vocabulary has none.
template <class Rec>
__host__ __device__ inline bool sca_nh(Rec& w, int a, int nh_id, int nh_word, uint64_t nh_label) {
  const int p = w.apos[a];
  if (!w.par[a] || !(w.e[p] & kBareN)) return false;
  const int d = w.deg[a];
  int kept = 0;
  for (int i = 0; i < d; ++i) {
    const int e = w.adj[a][i];
    kept += w.par[w.ba[e] ^ w.bb[e] ^ a] != 0;
  }
  if (kept == d) return false;
  if (nh_id < 0) return true;
  w.e[p] = (w.e[p] & ~(1 << 21)) | (nh_word & (1 << 21)) | kSubst;
  w.lab[p] = nh_label;
  return false;
}

// Lane 0: atoms, bonds and bond lists compacted to the atoms with par != 0, ascending and in place (a new index never
// exceeds the old one).  par keeps the INPUT indexing.
template <class Rec>
__host__ __device__ inline void sca_compact(Rec& w, int A, int nb, int& atoms, int& bonds) {
  int nK = 0, nBk = 0;
  for (int a = 0; a < A; ++a)
    if (w.par[a]) {
      w.stamp[a] = (uint16_t)nK;
      w.apos[nK++] = w.apos[a];
    }
  for (int e = 0; e < nb; ++e) {
    const int a = w.ba[e], b = w.bb[e];
    if (w.par[a] && w.par[b]) {
      w.stk[e] = (uint16_t)nBk;
      w.ba[nBk] = (uint8_t)w.stamp[a], w.bb[nBk] = (uint8_t)w.stamp[b];
      w.bsym[nBk++] = w.bsym[e];
    } else {
      w.stk[e] = 0xFFFF;
    }
  }
  for (int a = 0; a < A; ++a) {
    if (!w.par[a]) continue;
    const int na = w.stamp[a], d = w.deg[a];
    int k = 0;
    for (int i = 0; i < d; ++i) {
      const int ne = w.stk[w.adj[a][i]];
      if (ne != 0xFFFF) w.adj[na][k++] = (uint8_t)ne;
    }
    w.deg[na] = (uint8_t)k;
  }
  atoms = nK, bonds = nBk;
}

__global__ __launch_bounds__(256) void smiles_scaffold_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start, int V,
    const int32_t* __restrict__ table, const int64_t* __restrict__ label, const int32_t* __restrict__ ring_ids,
    int n_rings, int open_id, int close_id, int pad_id, int eos_id, int sep_id, int n_id, int nh_id,
    int64_t* __restrict__ tok_out, int out_width, int64_t* __restrict__ key_out, int32_t* __restrict__ info_out,
    int32_t* __restrict__ member_out) {
  __shared__ ScaWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  ScaWave& w = sh[wave];
  const int t0 = live ? start[row] : W;
  const bool in_range = live && t0 >= 0 && t0 <= W && W - t0 <= 256;
  const int g = in_range ? W - t0 : 0;                       // 0 <= g <= 256 tokens in the span
  const int64_t* yr = ys + (int64_t)row * ld_ys + (in_range ? t0 : 0);   // (read only under j < g)
  const int nh_word = nh_id >= 0 ? table[nh_id] : 0;
  const uint64_t nh_label = nh_id >= 0 ? (uint64_t)label[nh_id] : 0;
  int E = kNone, sep_at = 0;                                 // first <eos>; bit t: token lane + 64 t is <sep>
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    if (j < g) {
      const int64_t tok = yr[j];
      const bool known = tok >= 0 && tok < V;
      int word = known ? table[tok] & 0xFFFFFF : GCT_GRAMMAR_BANNED;
      if (tok == sep_id) word |= 1 << 24, sep_at |= 1 << t;  // (sep_id -1: none)
      if (tok == n_id) word |= kBareN;                       // (n_id -1: none)
      w.e[j] = word;
      w.lab[j] = known ? (uint64_t)label[tok] : key_unknown_label(tok);
      if (tok == eos_id) E = min(E, j);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) E = min(E, __shfl_xor(E, o, 64));
  int S = kNone;                                             // first <sep> in front of the <eos>
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (((sep_at >> t) & 1) && lane + 64 * t < E) S = min(S, lane + 64 * t);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) S = min(S, __shfl_xor(S, o, 64));
  const bool row_bad = E == kNone;                           // (a dead wave and a row out of range: g = 0, no <eos>)
  const bool two = S != kNone;
  uint64_t k_sca = 0, k_giv = 0;                             // lane 0's
  int st_giv = -1;

  // ---- the given part: gct_smiles_key's path (key_part of smiles_key.h, restated: see smiles_graph.h)
  {
    const bool active = !row_bad && two;
    int status = GCT_KEY_STRING_SYNTAX;
    __syncthreads();                                         // the staged row
    if (lane == 0) {
      int A = 0, nb = 0;
      if (active) {
        bool unsup;
        const bool parsed = rand_parse(w, 0, S, A, nb, unsup);
        status = !parsed ? GCT_KEY_STRING_SYNTAX : unsup ? GCT_KEY_STRING_UNSUPPORTED : GCT_KEY_GRAPH;
      }
      w.res[0] = active && status == GCT_KEY_GRAPH, w.res[1] = A, w.res[2] = nb;
    }
    __syncthreads();
    const bool graph = w.res[0] != 0;                        // (the same for the whole wave)
    const int nA = w.res[1], nB = w.res[2];
    const uint64_t sum = key_graph_sum(w, graph, nA, nB, lane);
    if (active && lane == 0) k_giv = graph ? key_combine(sum, nA, nB) : key_string(w, 0, S), st_giv = status;
  }

  // ---- the molecule: parse, peel, shell, [nH], compaction, key, spelling
  const int lo = two ? S + 1 : 0;
  int status = GCT_SCA_SYNTAX;                               // lane 0's
  __syncthreads();                                           // the given part's lists are done with
  if (lane == 0) {
    int A = 0, nb = 0;
    if (!row_bad) {
      bool unsup;
      const bool parsed = rand_parse(w, lo, E, A, nb, unsup);
      status = !parsed ? GCT_SCA_SYNTAX : unsup ? GCT_SCA_UNSUPPORTED : GCT_SCA_OK;
    }
    const bool graph = !row_bad && status == GCT_SCA_OK;
    w.res[0] = graph, w.res[1] = A, w.res[2] = nb, w.res[4] = graph ? A : 0;
  }
  __syncthreads();
  const bool graph = w.res[0] != 0;
  const int A = w.res[1], nb = w.res[2], atoms_in = w.res[4];
  if (graph) {
    for (int e = lane; e < nb; e += 64) w.blab[e] = (uint8_t)key_bond_label(w, e);
    for (int a = lane; a < A; a += 64) w.par[a] = 1, w.stamp[a] = w.deg[a];
  }
  __syncthreads();
  if (graph && lane == 0) w.res[3] = sca_peel(w, A);
  __syncthreads();
  const bool has = graph && w.res[3] > 0;                    // a non-empty core
  if (has)
    for (int e = lane; e < nb; e += 64) sca_shell(w, e);
  __syncthreads();
  bool missing = false;
  if (has)
    for (int a = lane; a < A; a += 64) missing |= sca_nh(w, a, nh_id, nh_word, nh_label);
  const bool no_token = __ballot(missing) != 0;
  __syncthreads();
  if (has && lane == 0) {
    int nK, nBk;
    sca_compact(w, A, nb, nK, nBk);
    w.res[1] = nK, w.res[2] = nBk;
  }
  __syncthreads();
  const int nK = has ? w.res[1] : 0, nBk = has ? w.res[2] : 0;
  const bool keyed = has && !no_token;
  const uint64_t sum = key_graph_sum(w, keyed, nK, nBk, lane);
  __syncthreads();                                           // the colours are done with: the walk's buffers alias them
  if (keyed) {
    for (int e = lane; e < nBk; e += 64) w.role[e] = 0;
    for (int a = lane; a < nK; a += 64) w.seen[a] = 0, w.left[a] = 0;
  }
  __syncthreads();
  if (lane == 0) {
    int len = 0;
    if (graph && !has) status = GCT_SCA_ACYCLIC;
    else if (has && no_token) status = GCT_SCA_NO_TOKEN;
    if (keyed) {
      const int room = min(out_width, 256) - 1;              // the spelling and its <eos> fit the row and 256 tokens
      k_sca = key_combine(sum, nK, nBk);
      len = rand_walk(w, nK, 0, 0, room, 0, ring_ids, n_rings, open_id, close_id);
      if (len < 0) status = GCT_SCA_NO_RING;
      else if (len > room) status = GCT_SCA_TOO_LONG;
      if (status != GCT_SCA_OK) len = 0;
    }
    w.res[5] = len;
  }
  __syncthreads();
  if (!live) return;
  const int len = w.res[5];
  int64_t* orow = tok_out + (int64_t)row * out_width;
  for (int c = lane; c < out_width; c += 64) {
    int64_t tok = pad_id;
    if (!row_bad && c < len) {                               // len <= 255
      const int v = w.out[c];
      tok = v >= 0 ? (int64_t)v : (w.e[-v - 1] & kSubst) ? (int64_t)nh_id : yr[-v - 1];   // -v - 1 < E < g
    } else if (!row_bad && c == len) {
      tok = eos_id;
    }
    orow[c] = tok;
  }
  int32_t* mrow = member_out + (int64_t)row * W;
  for (int c = lane; c < W; c += 64) mrow[c] = c < atoms_in ? (int32_t)w.par[c] : -1;   // atoms_in <= 255
  if (lane == 0) {
    key_out[(int64_t)row * 2] = (int64_t)k_sca, key_out[(int64_t)row * 2 + 1] = (int64_t)k_giv;
    int32_t* o4 = info_out + (int64_t)row * 4;
    o4[0] = row_bad ? -1 : status, o4[1] = st_giv, o4[2] = nK, o4[3] = len;
  }
}

}  // namespace

extern "C" int gct_smiles_scaffold(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                                   const int32_t* table32, const int64_t* label64, const int32_t* ring_ids, int n_rings,
                                   int open_id, int close_id, int pad_id, int eos_id, int sep_id, int n_id, int nh_id,
                                   int64_t* tokens_out, int out_width, int64_t* key_out, int32_t* info_out,
                                   int32_t* member_out, void* stream) {
  GCT_CHECK_ARG(ys && start && table32 && label64 && ring_ids && tokens_out && key_out && info_out && member_out &&
                    n >= 0 && V > 0, "smiles_scaffold: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W && out_width >= 1, "smiles_scaffold: %d token columns in rows of %lld, %d out", W,
                (long long)ld_ys, out_width);
  GCT_CHECK_ARG(n_rings >= 0 && n_rings <= 63, "smiles_scaffold: %d ring numbers (at most 63)", n_rings);
  GCT_CHECK_ARG(open_id >= 0 && open_id < V && close_id >= 0 && close_id < V && pad_id >= 0 && pad_id < V &&
                    eos_id >= 0 && eos_id < V && sep_id >= -1 && sep_id < V && n_id >= -1 && n_id < V && nh_id >= -1 &&
                    nh_id < V, "smiles_scaffold: a token id outside the vocabulary of %d", V);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_scaffold_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys, W,
                     n, start, V, table32, label64, ring_ids, n_rings, open_id, close_id, pad_id, eos_id, sep_id, n_id,
                     nh_id, tokens_out, out_width, key_out, info_out, member_out);
  GCT_LAUNCH_CHECK("smiles_scaffold");
  return GCT_OK;
}
