// The per-atom arithmetic of the molecule identity keys (molkey.py SmilesKeys states the rule), stated once for the
// kernels that key a parsed graph: gct_smiles_key (molkey.hip) and gct_smiles_scaffold (scaffold.hip).  Every function
// is a template over the wave's LDS record Rec, which derives from SmilesGraph (smiles_graph.h) and adds
//   uint64_t lab[256]   token position -> the token's 64-bit label
//   uint8_t blab[256]   bond -> its label o(e)
// (key_graph_sum and key_part also: uint64_t col[2][256], atom -> colour, double-buffered; int32_t res[], three words)
// and whose e[i] carries, from bit 21, the key's label of a BOND token (3 bits) or `aromatic` of an ATOM token.  Plain
// C++ but for the whole-wave functions at the end, host-callable so that a CPU harness can run it under a sanitizer.
#pragma once
#include "smiles_graph.h"

namespace {

constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;            // molkey.py: GOLD, STRING_DOMAIN, UNKNOWN_DOMAIN
constexpr uint64_t kStringDomain = 0xA0761D6478BD642Full;
constexpr uint64_t kUnknownDomain = 0xE7037ED1A0B428DBull;

__host__ __device__ inline uint64_t key_mix(uint64_t x) {    // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// The label of a token the vocabulary does not hold (the part is SYNTAX: it only enters a string key).
__host__ __device__ inline uint64_t key_unknown_label(int64_t tok) { return key_mix((uint64_t)tok ^ kUnknownDomain); }

// The string key of the tokens at [lo, hi): order-dependent, under its own domain constant.
template <class Rec>
__host__ __device__ inline uint64_t key_string(const Rec& w, int lo, int hi) {
  uint64_t h = kStringDomain;
  for (int i = lo; i < hi; ++i) h = key_mix((h + kGold) ^ w.lab[i]);
  return key_mix(h + (uint64_t)(hi - lo));
}

// o(e): the written symbol's label, or without one 5 between two aromatic atom tokens and 1 otherwise.
template <class Rec>
__host__ __device__ inline int key_bond_label(const Rec& w, int e) {
  const int s = w.bsym[e];
  if (s >= 0) return (w.e[s] >> 21) & 7;
  return ((w.e[w.apos[w.ba[e]]] >> 21) & (w.e[w.apos[w.bb[e]]] >> 21) & 1) ? 5 : 1;
}

// c0(a): the distance profile of atom a, by a breadth-first search over the bond lists.  The visited and the frontier
// sets are four 64-bit words each in registers (a part has at most 255 atoms), every word addressed by a constant.
template <class Rec>
__host__ __device__ inline uint64_t key_profile(const Rec& w, int a) {
  uint64_t v0 = 0, v1 = 0, v2 = 0, v3 = 0, f0, f1, f2, f3, n0, n1, n2, n3, sum = 0, md = 0;
  auto mark = [&](int v) {                                   // (v < 256: one of the four words takes the bit)
    const uint64_t bit = 1ull << (v & 63);
    const int q = v >> 6;
    n0 |= q == 0 ? bit : 0, n1 |= q == 1 ? bit : 0, n2 |= q == 2 ? bit : 0, n3 |= q == 3 ? bit : 0;
  };
  auto level = [&](uint64_t f, int base) {
    for (; f; f &= f - 1) {
      const int b = base + __builtin_ctzll(f);               // (a bit is only ever set for an atom of the part)
      sum += key_mix(w.lab[w.apos[b]] ^ md);
      const int d = w.deg[b];
      for (int i = 0; i < d; ++i) {
        const int e = w.adj[b][i];
        mark(w.ba[e] ^ w.bb[e] ^ b);
      }
    }
  };
  n0 = n1 = n2 = n3 = 0;
  mark(a);
  f0 = v0 = n0, f1 = v1 = n1, f2 = v2 = n2, f3 = v3 = n3;
  for (int dist = 1; (f0 | f1 | f2 | f3) != 0; ++dist) {     // (every level takes at least one new atom: <= 255 levels)
    md = key_mix((uint64_t)dist);
    n0 = n1 = n2 = n3 = 0;
    level(f0, 0), level(f1, 64), level(f2, 128), level(f3, 192);
    f0 = n0 & ~v0, f1 = n1 & ~v1, f2 = n2 & ~v2, f3 = n3 & ~v3;
    v0 |= f0, v1 |= f1, v2 |= f2, v3 |= f3;
  }
  return key_mix(w.lab[w.apos[a]] + sum);
}

// One round of bond-labelled refinement for atom a over the colours c.
template <class Rec>
__host__ __device__ inline uint64_t key_refine(const Rec& w, const uint64_t* c, int a) {
  uint64_t s = 3 * c[a];
  const int d = w.deg[a];
  for (int i = 0; i < d; ++i) {
    const int e = w.adj[a][i];
    s += key_mix(c[w.ba[e] ^ w.bb[e] ^ a] ^ key_mix((uint64_t)w.blab[e] + 0x100));
  }
  return key_mix(s);
}

__host__ __device__ inline uint64_t key_combine(uint64_t sum, int atoms, int bonds) {
  return key_mix(sum + (uint64_t)atoms * kGold + (uint64_t)bonds);
}

// A butterfly over the wave in a fixed order (the sums wrap, so any order gives the same bits; no atomics).
__device__ __forceinline__ uint64_t key_wave_sum(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), o, 64);
    x += (uint64_t)lo | ((uint64_t)hi << 32);
  }
  return x;
}

// The whole wave: the wrapping sum of the refined colours of a graph of nA atoms and nB bonds -- lane l labels bonds
// l + 64 t and takes the profiles of atoms l + 64 t, then GCT_KEY_ROUNDS rounds of refinement, one atom per lane and
// pass.  Every wave of the workgroup passes the same 1 + GCT_KEY_ROUNDS barriers, with or without a graph.
template <class Rec>
__device__ __forceinline__ uint64_t key_graph_sum(Rec& w, bool graph, int nA, int nB, int lane) {
  if (graph) {
    for (int e = lane; e < nB; e += 64) w.blab[e] = (uint8_t)key_bond_label(w, e);
    for (int a = lane; a < nA; a += 64) w.col[0][a] = key_profile(w, a);
  }
  __syncthreads();
  for (int r = 0; r < GCT_KEY_ROUNDS; ++r) {
    if (graph)
      for (int a = lane; a < nA; a += 64) w.col[(r + 1) & 1][a] = key_refine(w, w.col[r & 1], a);
    __syncthreads();
  }
  uint64_t sum = 0;
  if (graph)
    for (int a = lane; a < nA; a += 64) sum += key_mix(w.col[GCT_KEY_ROUNDS & 1][a]);
  return key_wave_sum(sum);
}

// The whole wave: the key of the part [lo, hi) of the staged row (an inactive wave only passes the barriers, two more
// than key_graph_sum's): lane 0 parses it, the wave sums a graph's colours, and a part without a graph (SYNTAX,
// UNSUPPORTED) gets lane 0's sequential hash of its tokens' labels instead.  The key and the status are lane 0's.
template <class Rec>
__device__ __forceinline__ uint64_t key_part(Rec& w, bool active, int lo, int hi, int lane, int& status, int& atoms,
                                             int& bonds) {
  status = -1;                                               // (no such part)
  __syncthreads();                                           // the staged row; the last part's lists are done with
  if (lane == 0) {
    int A = 0, nb = 0;
    if (active) {
      bool unsup;
      const bool parsed = rand_parse(w, lo, hi, A, nb, unsup);
      status = !parsed ? GCT_KEY_STRING_SYNTAX : unsup ? GCT_KEY_STRING_UNSUPPORTED : GCT_KEY_GRAPH;
    }
    w.res[0] = active && status == GCT_KEY_GRAPH, w.res[1] = A, w.res[2] = nb;
  }
  __syncthreads();
  const bool graph = w.res[0] != 0;                          // (the same for the whole wave)
  atoms = w.res[1], bonds = w.res[2];
  const uint64_t sum = key_graph_sum(w, graph, atoms, bonds, lane);
  if (!active || lane != 0) return 0;
  return graph ? key_combine(sum, atoms, bonds) : key_string(w, lo, hi);
}

}  // namespace
