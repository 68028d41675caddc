// Molecule identity keys on the device: gct_smiles_key against molkey.py SmilesKeys (key is the statement for one part,
// key_reference the batch rule).  One wave per row, four rows per workgroup, in smiles_randomize_kernel's shape: lane l
// stages tokens l + 64 t of the row's span -- the table word and the token's 64-bit label -- in the wave's own LDS and the
// wave finds the first <eos> and the first <sep> in front of it; then, part by part (the scaffold, if any, first):
//   lane 0 parses the part into bonds and per-atom bond lists (rand_parse of smiles_graph.h);
//   lane l labels bonds l + 64 t and runs the breadth-first searches of atoms l + 64 t on its own: the visited and the
//     frontier sets are four 64-bit words each in registers (a part has at most 255 atoms), every word addressed by a
//     constant, and the bond lists are read from LDS, so no per-lane array is indexed at run time and nothing spills;
//   GCT_KEY_ROUNDS rounds of refinement, one atom per lane and pass, the colours double-buffered in LDS;
//   a butterfly over the wave in a fixed order sums the atoms' colours (the sums wrap, so any order gives the same bits;
//     no atomics).
// A part without a graph (SYNTAX, UNSUPPORTED) gets lane 0's sequential hash of its tokens' labels instead.
// LDS: sizeof(KeyWave) = 13 072 bytes per wave (6 656 the parsed graph, 2 048 the labels, 4 096 the two colour buffers,
// 256 the bond labels, 16 the part's header), 52 288 per workgroup of four rows.
// The prelude is smiles_stage_row (smiles_graph.h); key_part and the per-atom functions under it (key_profile,
// key_refine, ...) are smiles_key.h's, shared with gct_smiles_scaffold.
#include "smiles_key.h"

namespace {

struct KeyWave : SmilesGraph {                               // e[i] also carries, from bit 21: the key's bond label of a
  uint64_t lab[256];                                         //  BOND token (3 bits) or `aromatic` of an ATOM token, and
  uint64_t col[2][256];                                      //  (the token is <sep>) << 24
  uint8_t blab[256];                                         // lab: token position -> label; col: atom -> colour;
  int32_t res[4];                                            // blab: bond -> label; res: graph?, atoms, bonds
};
static_assert(sizeof(KeyWave) * 4 <= 64 * 1024, "four rows per workgroup must fit 64 KB of LDS");

__global__ __launch_bounds__(256) void smiles_key_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start, int V,
    const int32_t* __restrict__ table, const int64_t* __restrict__ label, int eos_id, int sep_id,
    int64_t* __restrict__ key_out, int32_t* __restrict__ info_out) {
  __shared__ KeyWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  KeyWave& w = sh[wave];
  const StagedRow sr = smiles_stage_row(w, ys, ld_ys, W, n, row, start, V, table, eos_id, sep_id, lane,
                                        [&](int j, int64_t tok, bool known, int word) {
                                          w.lab[j] = known ? (uint64_t)label[tok] : key_unknown_label(tok);
                                          return word & 0xFFFFFF;
                                        });
  const int E = sr.E, S = sr.S;
  const bool row_bad = E == kNone;                           // (a dead wave and a row out of range: g = 0, no <eos>)
  const bool two = S != kNone;
  uint64_t k_mol = 0, k_sca = 0;                             // lane 0's
  int st_mol = -1, st_sca = -1, atoms = 0, bonds = 0;

  for (int it = 0; it < 2; ++it) {
    const int which = 1 - it;                                // the scaffold (part 1) first, then the molecule (part 0)
    const bool active = !row_bad && (which == 0 || two);
    const int lo = which == 1 ? 0 : (two ? S + 1 : 0), hi = which == 1 ? S : E;
    int status, nA, nB;
    const uint64_t k = key_part(w, active, lo, hi, lane, status, nA, nB);
    if (active && lane == 0) {
      if (which == 1) {
        k_sca = k, st_sca = status;
      } else {
        k_mol = k, st_mol = status, atoms = nA, bonds = nB;
      }
    }
  }
  if (live && lane == 0) {
    key_out[(int64_t)row * 2] = (int64_t)k_mol, key_out[(int64_t)row * 2 + 1] = (int64_t)k_sca;
    int32_t* o4 = info_out + (int64_t)row * 4;
    o4[0] = st_mol, o4[1] = st_sca, o4[2] = atoms, o4[3] = bonds;
  }
}

}  // namespace

extern "C" int gct_smiles_key(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                              const int32_t* table32, const int64_t* label64, int pad_id, int eos_id, int sep_id,
                              int64_t* key_out, int32_t* info_out, void* stream) {
  GCT_CHECK_ARG(ys && start && table32 && label64 && key_out && info_out && n >= 0 && V > 0, "smiles_key: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W, "smiles_key: %d token columns in rows of %lld", W, (long long)ld_ys);
  GCT_CHECK_ARG(pad_id >= 0 && pad_id < V && eos_id >= 0 && eos_id < V && sep_id >= -1 && sep_id < V,
                "smiles_key: a token id outside the vocabulary of %d", V);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_key_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys, W, n,
                     start, V, table32, label64, eos_id, sep_id, key_out, info_out);
  GCT_LAUNCH_CHECK("smiles_key");
  return GCT_OK;
}
