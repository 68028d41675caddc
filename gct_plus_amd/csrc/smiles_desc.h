// Ring perception and the per-atom and per-bond arithmetic of the molecular descriptors (descriptor.py states the rule:
// SmilesDescriptors.describe), stated once for gct_smiles_desc (descriptor.hip).  Every function is a template over the
// wave's LDS record Rec, which derives from SmilesGraph (smiles_graph.h) and adds
//   uint16_t dsc[256]    token position -> the token's desc32 word (include/gctplus_hip.h documents the bits)
//   uint8_t rsz[256]     bond -> s(e), the smallest ring through it; 0: no ring bond
//   uint8_t bcls[256]    bond -> its class (kDescSingle ..)
//   uint8_t aflag[256]   atom -> bit 0: it has a TRIPLE bond
// and whose e[i] carries, from bit 21, the key's label of a BOND token (smiles_key.h's table32).  Plain C++,
// host-callable so that a CPU harness can run it under a sanitizer.
#pragma once
#include "smiles_graph.h"

namespace {

enum { kDescSingle = 1, kDescDouble = 2, kDescTriple = 3, kDescQuad = 4, kDescAromatic = 5 };

// desc32: element index + 1 | aromatic << 4 | bracket << 5 | stated H << 6 | (charge + 3) << 10
__host__ __device__ inline int desc_element(int d) { return (d & 15) - 1; }      // -1: UNKNOWN
__host__ __device__ inline bool desc_aromatic(int d) { return (d >> 4) & 1; }
__host__ __device__ inline bool desc_bracket(int d) { return (d >> 5) & 1; }
__host__ __device__ inline int desc_stated_h(int d) { return (d >> 6) & 15; }
__host__ __device__ inline int desc_charge(int d) { return ((d >> 10) & 7) - 3; }

enum { kElB, kElC, kElN, kElO, kElF, kElSi, kElP, kElS, kElCl, kElBr, kElI };

__host__ __device__ inline int desc_mass(int el) {           // mDa; selects, not a table in memory
  switch (el) {
    case kElB: return 10810;
    case kElC: return 12011;
    case kElN: return 14007;
    case kElO: return 15999;
    case kElF: return 18998;
    case kElSi: return 28086;
    case kElP: return 30974;
    case kElS: return 32060;
    case kElCl: return 35450;
    case kElBr: return 79904;
    default: return 126904;
  }
}
constexpr int kDescHydrogenMass = 1008;

// The smallest normal valence >= sigma of a bare atom; -1: none (Si has no list: it cannot be written bare).
__host__ __device__ inline int desc_v0(int el, int sigma) {
  switch (el) {
    case kElB: return sigma <= 3 ? 3 : -1;
    case kElC: return sigma <= 4 ? 4 : -1;
    case kElN:
    case kElP: return sigma <= 3 ? 3 : sigma <= 5 ? 5 : -1;
    case kElO: return sigma <= 2 ? 2 : -1;
    case kElS: return sigma <= 2 ? 2 : sigma <= 4 ? 4 : sigma <= 6 ? 6 : -1;
    case kElF:
    case kElCl:
    case kElBr:
    case kElI: return sigma <= 1 ? 1 : -1;
    default: return -1;
  }
}

// s(e): a breadth-first search from end a of bond e over the bond lists with e excluded, stopped at the level that
// reaches end b; 1 + that level, or 0 when b is not reachable.  The visited and the frontier sets are four 64-bit words
// each in registers (a part has at most 255 atoms), every word addressed by a constant, exactly as key_profile's.
template <class Rec>
__host__ __device__ inline int desc_ring_size(const Rec& w, int e) {
  const int a = w.ba[e], b = w.bb[e];
  uint64_t v0, v1, v2, v3, f0, f1, f2, f3, n0, n1, n2, n3;
  auto mark = [&](int v) {                                   // (v < 256: one of the four words takes the bit)
    const uint64_t bit = 1ull << (v & 63);
    const int q = v >> 6;
    n0 |= q == 0 ? bit : 0, n1 |= q == 1 ? bit : 0, n2 |= q == 2 ? bit : 0, n3 |= q == 3 ? bit : 0;
  };
  auto level = [&](uint64_t f, int base) {
    for (; f; f &= f - 1) {
      const int u = base + __builtin_ctzll(f);               // (a bit is only ever set for an atom of the part)
      const int d = w.deg[u];
      for (int i = 0; i < d; ++i) {
        const int x = w.adj[u][i];
        if (x != e) mark(w.ba[x] ^ w.bb[x] ^ u);
      }
    }
  };
  n0 = n1 = n2 = n3 = 0;
  mark(a);
  f0 = v0 = n0, f1 = v1 = n1, f2 = v2 = n2, f3 = v3 = n3;
  const int qb = b >> 6;
  const uint64_t bbit = 1ull << (b & 63);
  for (int dist = 1; (f0 | f1 | f2 | f3) != 0; ++dist) {     // (every level takes at least one new atom: <= 254 levels)
    n0 = n1 = n2 = n3 = 0;
    level(f0, 0), level(f1, 64), level(f2, 128), level(f3, 192);
    const uint64_t nb = qb == 0 ? n0 : qb == 1 ? n1 : qb == 2 ? n2 : n3;
    if (nb & bbit) return dist + 1;                          // (at most 255: a ring holds at most 255 atoms)
    f0 = n0 & ~v0, f1 = n1 & ~v1, f2 = n2 & ~v2, f3 = n3 & ~v3;
    v0 |= f0, v1 |= f1, v2 |= f2, v3 |= f3;
  }
  return 0;
}

// The class of bond e, s = its ring size: the written symbol's (- and ~ SINGLE, = DOUBLE, # TRIPLE, $ QUAD, :
// AROMATIC); without a symbol AROMATIC between two aromatic atoms when the bond is a ring bond, SINGLE otherwise.
template <class Rec>
__host__ __device__ inline int desc_bond_class(const Rec& w, int e, int s) {
  const int sym = w.bsym[e];
  if (sym >= 0) {
    const int lab = (w.e[sym] >> 21) & 7;                    // (0, a / or \: the part is UNSUPPORTED and never gets here)
    return lab == 6 || lab == 0 ? kDescSingle : lab;
  }
  return s != 0 && desc_aromatic(w.dsc[w.apos[w.ba[e]]]) && desc_aromatic(w.dsc[w.apos[w.bb[e]]]) ? kDescAromatic
                                                                                                 : kDescSingle;
}

// Ertl's contribution of an N (is_n) or O atom in 0.01 A^2: n bonds, h hydrogens, sg / db / tr / ar of them SINGLE /
// DOUBLE / TRIPLE / AROMATIC, charge q, r3 = in a 3-ring.  The lines of descriptor.TPSA_LINES as one switch over the
// packed figures: a line's counts account for all n bonds (a QUAD bond leaves sg + db + tr + ar < n: the fallback).
constexpr int desc_tpsa_key(int is_n, int n, int h, int sg, int db, int tr, int ar, int q) {
  return is_n | n << 1 | h << 5 | sg << 9 | db << 13 | tr << 17 | ar << 21 | (q + 3) << 25;
}

__host__ __device__ inline int desc_tpsa(bool is_n, int n, int h, int sg, int db, int tr, int ar, int q, bool r3) {
  if (sg + db + tr + ar == n) {
    switch (desc_tpsa_key(is_n, n, h, sg, db, tr, ar, q)) {
      case desc_tpsa_key(1, 1, 0, 0, 0, 1, 0, 0): return 2379;
      case desc_tpsa_key(1, 1, 1, 0, 1, 0, 0, 0): return 2385;
      case desc_tpsa_key(1, 1, 2, 1, 0, 0, 0, 0): return 2602;
      case desc_tpsa_key(1, 1, 2, 0, 1, 0, 0, 1): return 2559;
      case desc_tpsa_key(1, 1, 3, 1, 0, 0, 0, 1): return 2764;
      case desc_tpsa_key(1, 2, 0, 1, 1, 0, 0, 0): return 1236;
      case desc_tpsa_key(1, 2, 0, 0, 1, 1, 0, 0): return 1360;
      case desc_tpsa_key(1, 2, 1, 2, 0, 0, 0, 0): return r3 ? 2194 : 1203;
      case desc_tpsa_key(1, 2, 0, 1, 0, 1, 0, 1): return 436;
      case desc_tpsa_key(1, 2, 1, 1, 1, 0, 0, 1): return 1397;
      case desc_tpsa_key(1, 2, 2, 2, 0, 0, 0, 1): return 1661;
      case desc_tpsa_key(1, 2, 0, 0, 0, 0, 2, 0): return 1289;
      case desc_tpsa_key(1, 2, 1, 0, 0, 0, 2, 0): return 1579;
      case desc_tpsa_key(1, 2, 1, 0, 0, 0, 2, 1): return 1414;
      case desc_tpsa_key(1, 3, 0, 3, 0, 0, 0, 0): return r3 ? 301 : 324;
      case desc_tpsa_key(1, 3, 0, 1, 2, 0, 0, 0): return 1168;
      case desc_tpsa_key(1, 3, 0, 2, 1, 0, 0, 1): return 301;
      case desc_tpsa_key(1, 3, 1, 3, 0, 0, 0, 1): return 444;
      case desc_tpsa_key(1, 3, 0, 0, 0, 0, 3, 0): return 441;
      case desc_tpsa_key(1, 3, 0, 1, 0, 0, 2, 0): return 493;
      case desc_tpsa_key(1, 3, 0, 0, 1, 0, 2, 0): return 410;
      case desc_tpsa_key(1, 3, 0, 0, 0, 0, 3, 1): return 410;
      case desc_tpsa_key(1, 3, 0, 1, 0, 0, 2, 1): return 388;
      case desc_tpsa_key(1, 4, 0, 4, 0, 0, 0, 1): return 0;
      case desc_tpsa_key(0, 1, 0, 0, 1, 0, 0, 0): return 1707;
      case desc_tpsa_key(0, 1, 1, 1, 0, 0, 0, 0): return 2023;
      case desc_tpsa_key(0, 1, 0, 1, 0, 0, 0, -1): return 2306;
      case desc_tpsa_key(0, 2, 0, 2, 0, 0, 0, 0): return r3 ? 1253 : 923;
      case desc_tpsa_key(0, 2, 0, 0, 0, 0, 2, 0): return 1314;
      default: break;
    }
  }
  const int v = is_n ? 3050 - 820 * n + 150 * h : 2850 - 860 * n + 150 * h;
  return v > 0 ? v : 0;
}

// What atom a adds to the row's sums; rsz and bcls of its bonds are final.
struct DescAtom {
  int unknown, hydrogens, mass, charge, hbd, hba, tpsa, touched, triple;
};

template <class Rec>
__host__ __device__ inline DescAtom desc_atom(const Rec& w, int a) {
  DescAtom r = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int d = w.dsc[w.apos[a]], el = desc_element(d);
  if (el < 0) {
    r.unknown = 1;
    return r;
  }
  const int n = w.deg[a];
  int sigma = 0, sg = 0, db = 0, tr = 0, ar = 0;
  bool r3 = false;
  for (int i = 0; i < n; ++i) {
    const int x = w.adj[a][i], c = w.bcls[x];
    sigma += c == kDescAromatic ? 1 : c;
    sg += c == kDescSingle, db += c == kDescDouble, tr += c == kDescTriple, ar += c == kDescAromatic;
    r3 |= w.rsz[x] == 3;
    r.touched |= c == kDescAromatic && w.rsz[x] != 0;
  }
  int h;
  if (desc_bracket(d)) {
    h = desc_stated_h(d);
  } else {
    const int v0 = desc_v0(el, sigma);
    h = v0 < 0 ? 0 : desc_aromatic(d) ? (v0 - sigma - 1 > 0 ? v0 - sigma - 1 : 0) : v0 - sigma;
  }
  r.hydrogens = h;
  r.mass = desc_mass(el) + kDescHydrogenMass * h;
  r.charge = desc_charge(d);
  r.triple = tr != 0;
  if (el == kElN || el == kElO) {
    r.hba = 1;
    r.hbd = h >= 1;
    r.tpsa = desc_tpsa(el == kElN, n, h, sg, db, tr, ar, r.charge, r3);
  }
  return r;
}

// The lowest atom that a reaches over the AROMATIC ring bonds (a itself without one): the representative of a's
// component of that subgraph.  The search is desc_ring_size's, over those bonds only and to exhaustion.
template <class Rec>
__host__ __device__ inline int desc_component(const Rec& w, int a) {
  uint64_t v0, v1, v2, v3, f0, f1, f2, f3, n0, n1, n2, n3;
  auto mark = [&](int v) {
    const uint64_t bit = 1ull << (v & 63);
    const int q = v >> 6;
    n0 |= q == 0 ? bit : 0, n1 |= q == 1 ? bit : 0, n2 |= q == 2 ? bit : 0, n3 |= q == 3 ? bit : 0;
  };
  auto level = [&](uint64_t f, int base) {
    for (; f; f &= f - 1) {
      const int u = base + __builtin_ctzll(f);
      const int d = w.deg[u];
      for (int i = 0; i < d; ++i) {
        const int x = w.adj[u][i];
        if (w.bcls[x] == kDescAromatic && w.rsz[x] != 0) mark(w.ba[x] ^ w.bb[x] ^ u);
      }
    }
  };
  n0 = n1 = n2 = n3 = 0;
  mark(a);
  f0 = v0 = n0, f1 = v1 = n1, f2 = v2 = n2, f3 = v3 = n3;
  while ((f0 | f1 | f2 | f3) != 0) {                         // (every level takes at least one new atom)
    n0 = n1 = n2 = n3 = 0;
    level(f0, 0), level(f1, 64), level(f2, 128), level(f3, 192);
    f0 = n0 & ~v0, f1 = n1 & ~v1, f2 = n2 & ~v2, f3 = n3 & ~v3;
    v0 |= f0, v1 |= f1, v2 |= f2, v3 |= f3;
  }
  return v0 ? __builtin_ctzll(v0) : v1 ? 64 + __builtin_ctzll(v1) : v2 ? 128 + __builtin_ctzll(v2) : 192 + __builtin_ctzll(v3);
}

// Bond e is rotatable: SINGLE, no ring bond, both ends of degree >= 2, neither end with a TRIPLE bond (aflag is final).
template <class Rec>
__host__ __device__ inline bool desc_rotatable(const Rec& w, int e) {
  const int a = w.ba[e], b = w.bb[e];
  return w.bcls[e] == kDescSingle && w.rsz[e] == 0 && w.deg[a] >= 2 && w.deg[b] >= 2 && !((w.aflag[a] | w.aflag[b]) & 1);
}

}  // namespace
