// SMILES randomisation on the device: gct_smiles_randomize against randomize.py SmilesRandomizer (randomize is the
// statement for one part, randomize_reference the batch rule).  One wave per row, four rows per workgroup, in
// smiles_check_kernel's shape (chem.hip): lane l stages tokens l + 64 t of the row's span in the wave's own LDS and
// the wave finds the first <eos> and the first <sep> in front of it; then, part by part (the scaffold, if any, first):
//   lane 0 parses the part into bonds and per-atom bond lists (rand_parse of smiles_graph.h) and tosses the coin;
//   lane l shuffles the lists of atoms l + 64 t (Philox calls keyed by the INPUT atom: none waits for the walk);
//   lane 0 runs the depth-first search that tells tree edges from ring bonds, and the emission into the LDS row;
// and all lanes write the output row, perm and info.  The walks are one lane's because every step depends on the one
// before; what they leave is indexed dynamically in LDS, never in registers, so nothing spills.  No global atomics.
// An entry of the LDS row is a literal token id (>= 0: ring numbers, parentheses, <sep>, <eos>) or -(j + 1): the token
// at position j of the input span (atoms and bond symbols are carried verbatim, whatever their ids).
// smiles_stage_row is smiles_graph.h's; rand_shuffle_atom and rand_walk are smiles_walk.h's.
#include "smiles_walk.h"

namespace {

struct RandWave : SmilesGraph {                              // (smiles_graph.h: what rand_parse fills; e[i] carries
  int32_t out[256];                                          //  (the token is <sep>) << 24; adj is shuffled in place)
  uint8_t seen[256], pbond[256], left[256];                  // per atom; pbond: the bond the search came by (0xFF: root)
  uint8_t role[256], rnum[256];                              // per bond; role 0 unseen, 1 tree, 2 / 3 ring opened at ba / bb
  uint8_t perm[256];
  int32_t res[4];                                            // randomise this part, its atoms, its bonds
};

__global__ __launch_bounds__(256) void smiles_randomize_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start,
    const int64_t* __restrict__ key, int V, const int32_t* __restrict__ table, const int32_t* __restrict__ ring_ids,
    int n_rings, int open_id, int close_id, int pad_id, int eos_id, int sep_id, GctRng rng, float p,
    int64_t* __restrict__ out, int32_t* __restrict__ info, int32_t* __restrict__ perm, int out_width) {
  __shared__ RandWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  RandWave& w = sh[wave];
  const StagedRow sr = smiles_stage_row(w, ys, ld_ys, W, n, row, start, V, table, eos_id, sep_id, lane,
                                        [](int, int64_t, bool, int word) { return word & 0x1FFFFF; });
  const int t0 = sr.t0, g = sr.g, E = sr.E, S = sr.S;
  const int64_t* yr = sr.yr;
  const bool row_bad = E == kNone;                           // (a dead wave and a row out of range: g = 0, no <eos>)
  const bool two = S != kNone;
  const int total = row_bad ? 0 : min(out_width - t0, 256);  // columns the new span may take: total >= g > E
  const int64_t kw = live ? key[row] : 0;
  const uint32_t klo = (uint32_t)kw, khi = (uint32_t)((uint64_t)kw >> 32);
  int opos = 0, abase = 0, st_mol = GCT_RAND_SYNTAX, st_sca = -1;   // lane 0's: output columns and atoms so far

  for (int it = 0; it < 2; ++it) {
    const int which = 1 - it;                                // the scaffold (part 1) first, then the molecule (part 0)
    const bool active = !row_bad && (which == 0 || two);
    const int lo = which == 1 ? 0 : (two ? S + 1 : 0), hi = which == 1 ? S : E;
    int A = 0, nb = 0, status = GCT_RAND_SYNTAX;
    uint32_t root_word = 0;
    __syncthreads();                                         // the staged row; the last part's lists are done with
    if (active && lane == 0) {
      bool unsup;
      const bool parsed = rand_parse(w, lo, hi, A, nb, unsup);
      status = !parsed ? GCT_RAND_SYNTAX : unsup ? GCT_RAND_UNSUPPORTED : GCT_RAND_KEPT;
      if (status == GCT_RAND_KEPT) {
        const uint4 c = gct_philox(rng, klo, khi, (uint32_t)which, 0u);
        root_word = c.y;
        if (p >= 1.f || c.x < (uint32_t)((double)p * 4294967296.0)) status = GCT_RAND_OK;   // (0 <= p < 1: below 2^32)
      }
      w.res[0] = status == GCT_RAND_OK, w.res[1] = A, w.res[2] = nb;
    } else if (lane == 0) {
      w.res[0] = 0;
    }
    __syncthreads();
    if (w.res[0]) {
      const int nA = w.res[1], nB = w.res[2];
      for (int e = lane; e < nB; e += 64) w.role[e] = 0;
      for (int a = lane; a < nA; a += 64) {
        w.seen[a] = 0, w.left[a] = 0;
        const int d = w.deg[a];
        if (d < 2) continue;
        const uint4 c0 = gct_philox(rng, klo, khi, (uint32_t)which, (uint32_t)(1 + 2 * a));
        uint4 c1 = make_uint4(0, 0, 0, 0);
        if (d > 5) c1 = gct_philox(rng, klo, khi, (uint32_t)which, (uint32_t)(2 + 2 * a));
        rand_shuffle_atom(w, a, d, c0, c1);
      }
    }
    __syncthreads();
    if (active && lane == 0) {
      const int len = hi - lo;
      // room: <eos>, and for the scaffold the <sep> and the molecule's input length, stay inside `total`
      const int room = total - 1 - (which == 1 ? 1 + (E - S - 1) : opos);
      int k = len;
      if (status == GCT_RAND_OK) {
        k = rand_walk(w, A, (int)__umulhi(root_word, (uint32_t)A), opos, room, abase, ring_ids, n_rings, open_id,
                      close_id);
        if (k < 0) status = GCT_RAND_NO_RING;
        else if (k > room) status = GCT_RAND_TOO_LONG;
      }
      if (status != GCT_RAND_OK) {                           // kept: the input tokens, the atoms in their order
        k = len;                                             // (opos + len < total: the input fitted)
        for (int i = 0; i < len; ++i) w.out[opos + i] = -(lo + i + 1);
        for (int a = 0; a < A; ++a) w.perm[abase + a] = (uint8_t)(abase + a);
      }
      w.out[opos + k] = which == 1 ? sep_id : eos_id;
      opos += k + 1;
      abase += A;                                            // (A = 0 for SYNTAX)
      if (which == 1) st_sca = status; else st_mol = status;
    }
  }
  if (lane == 0) w.res[0] = opos, w.res[1] = abase;
  __syncthreads();
  if (!live) return;
  const int outlen = w.res[0], atoms = w.res[1];
  int64_t* orow = out + (int64_t)row * out_width;
  if (row_bad) {
    const int64_t* whole = ys + (int64_t)row * ld_ys;
    for (int c = lane; c < out_width; c += 64) orow[c] = c < W ? whole[c] : (int64_t)pad_id;
  } else {
    const int64_t* whole = yr - t0;
    for (int c = lane; c < out_width; c += 64) {
      int64_t tok = pad_id;
      if (c < t0) {
        tok = whole[c];
      } else if (c - t0 < outlen) {                          // outlen <= total <= 256
        const int v = w.out[c - t0];
        tok = v >= 0 ? (int64_t)v : yr[-v - 1];              // -v - 1 < E < g
      }
      orow[c] = tok;
    }
  }
  if (perm) {
    int32_t* prow = perm + (int64_t)row * out_width;
    for (int c = lane; c < out_width; c += 64) prow[c] = c < atoms ? (int32_t)w.perm[c] : -1;   // atoms <= 255
  }
  if (lane == 0) {
    int32_t* o4 = info + (int64_t)row * 4;
    o4[0] = st_mol, o4[1] = row_bad ? -1 : st_sca, o4[2] = row_bad ? g : outlen, o4[3] = atoms;
  }
}

}  // namespace

extern "C" int gct_smiles_randomize(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start,
                                    const int64_t* key, int V, const int32_t* table, const int32_t* ring_ids, int n_rings,
                                    int open_id, int close_id, int pad_id, int eos_id, int sep_id, uint64_t seed, float p,
                                    int64_t* out, int32_t* info, int32_t* perm, int out_width, void* stream) {
  GCT_CHECK_ARG(ys && start && key && table && ring_ids && out && info && n >= 0 && V > 0, "smiles_randomize: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W && out_width >= W, "smiles_randomize: %d token columns in rows of %lld, %d out", W,
                (long long)ld_ys, out_width);
  GCT_CHECK_ARG(n_rings >= 0 && n_rings <= 63, "smiles_randomize: %d ring numbers (at most 63)", n_rings);
  GCT_CHECK_ARG(open_id >= 0 && open_id < V && close_id >= 0 && close_id < V && pad_id >= 0 && pad_id < V &&
                    eos_id >= 0 && eos_id < V && sep_id >= -1 && sep_id < V,
                "smiles_randomize: a token id outside the vocabulary of %d", V);
  GCT_CHECK_ARG(p >= 0.f && p <= 1.f, "smiles_randomize: p = %g is no probability", (double)p);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_randomize_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys,
                     W, n, start, key, V, table, ring_ids, n_rings, open_id, close_id, pad_id, eos_id, sep_id,
                     gct_rng_make(seed, GCT_SITE_RANDOMIZE), p, out, info, perm, out_width);
  GCT_LAUNCH_CHECK("smiles_randomize");
  return GCT_OK;
}
