// The per-atom arithmetic of the circular fingerprints and the per-pair arithmetic of the Tanimoto aggregates
// (fingerprint.py states the rules: SmilesFingerprints.fingerprint and tanimoto_reference), stated once for the two
// kernels of fingerprint.hip.  The fingerprint functions are templates over the wave's LDS record Rec, which derives
// from SmilesGraph (smiles_graph.h) and adds
//   uint64_t col[2][256]  atom -> identifier, double-buffered; col[1][j] first holds the label of the token at j
//   uint8_t blab[256]     bond -> its label o(e)
//   uint32_t bits[32]     the row's GCT_FP_BITS bits: word k >> 5, bit k & 31
// and whose e[i] carries the key's bits from bit 21 (smiles_key.h).  key_mix, key_bond_label and key_refine are
// smiles_key.h's, unchanged.  Plain C++ but for fp_mark's LDS OR, host-callable so that a CPU harness can run it under a
// sanitizer.
#pragma once
#include "smiles_key.h"

namespace {

static_assert(GCT_FP_BITS == 1024, "a fingerprint is 16 64-bit words: the records and kernels below count on it");
constexpr int kFpWords = GCT_FP_BITS / 32;                   // 32-bit words of a fingerprint

// id_0(a) = mix(L(a) ^ mix(0x200 + deg(a))): the label of the atom's token and the number of its bonds.
template <class Rec>
__host__ __device__ inline uint64_t fp_id0(const Rec& w, int a) {
  return key_mix(w.col[1][w.apos[a]] ^ key_mix(0x200ull + (uint64_t)w.deg[a]));
}

// Set bit id mod GCT_FP_BITS of the row.  OR commutes, so the lanes of a wave may set their bits in any order: an LDS
// OR on the device (no global atomic), a plain one on the host.
template <class Rec>
__host__ __device__ inline void fp_mark(Rec& w, uint64_t id) {
  const uint32_t k = (uint32_t)(id & (uint64_t)(GCT_FP_BITS - 1));
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(&w.bits[k >> 5], 1u << (k & 31));
#else
  w.bits[k >> 5] |= 1u << (k & 31);
#endif
}

// ---- Tanimoto.  A pair is (c, u) = (popcount(a & b), cnt_a + cnt_b - c); T = (float)c / (float)u, correctly rounded.

// popcount(x) + c: on the device the one instruction that does both (left to itself the compiler counts into fresh
// registers and adds them up afterwards, 2.5 instructions per word instead of 2).
__host__ __device__ inline int tani_count(uint32_t x, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
  int r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(c));
  return r;
#else
  return __builtin_popcount(x) + c;
#endif
}

// The product of two figures of at most 2 * GCT_FP_BITS in absolute value: a full-rate 24-bit multiply on the device.
__host__ __device__ inline int tani_mul(int x, int y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(x, y);
#else
  return x * y;
#endif
}

// c over the kFpWords 32-bit words of two fingerprints, on two chains.
__host__ __device__ inline int tani_common(const uint32_t* a, const uint32_t* b) {
  int c0 = 0, c1 = 0;
#pragma unroll
  for (int k = 0; k < kFpWords; k += 2) c0 = tani_count(a[k] & b[k], c0), c1 = tani_count(a[k + 1] & b[k + 1], c1);
  return c0 + c1;
}

// The running best of one row of a: (c, u, j), (-1, 1, -1) before the first present row of b.  c / u > bc / bu by cross
// multiplication (every figure is at most GCT_FP_BITS, u and bu are positive): exact, so ties keep the earlier j.
struct TaniBest {
  int c, u, j;
};

__host__ __device__ inline TaniBest tani_none() { return TaniBest{-1, 1, -1}; }

__host__ __device__ inline bool tani_better(int c, int u, const TaniBest& b) {
  return tani_mul(c, b.u) > tani_mul(b.c, u);
}

// The term a present pair adds to `total`: T for P = 1, the fp64 product of the fp32 T with itself for P = 2 (exact).
template <int P>
__host__ __device__ inline double tani_term(int c, int u) {
  const float t = (float)c / (float)u;
  return P == 2 ? (double)t * (double)t : (double)t;
}

// One row of a (its words and count ca) against rows [j0, j1) of b in ascending order: b's words at bw + 32 (j - jb),
// its counts at bcnt + (j - jb).  A row of b with count 0 is absent: it adds nothing and never wins (by selects, not a
// branch, so that the count's read does not stand in front of the pair's; u = 0 can only meet an absent row of b, whose
// quotient is dropped).
template <int P>
__host__ __device__ inline void tani_tile(const uint32_t* a, int ca, const uint32_t* bw, const int32_t* bcnt, int jb,
                                          int j0, int j1, TaniBest& best, double& total) {
  for (int j = j0; j < j1; ++j) {
    const int cb = bcnt[j - jb];
    const bool present = cb != 0;
    const int c = tani_common(a, bw + (size_t)(j - jb) * kFpWords), u = ca + cb - c;
    total += present ? tani_term<P>(c, u) : 0.0;
    if (present && tani_better(c, u, best)) best = TaniBest{c, u, j};
  }
}

// The fold of one row's per-split partials, in split order: the earlier split wins a tie (its rows of b are lower), the
// totals are added in split order.  An absent row of a (ca == 0) and a row that met no present row of b: (0, -1, 0).
__host__ __device__ inline void tani_fold(const int32_t* pc, const int32_t* pu, const int32_t* pj, const double* pt,
                                          size_t stride, int splits, int ca, float& best, int32_t& arg, double& total) {
  TaniBest b = tani_none();
  double t = 0.0;
  for (int s = 0; s < splits; ++s) {
    const size_t at = (size_t)s * stride;
    if (pj[at] >= 0 && tani_better(pc[at], pu[at], b)) b = TaniBest{pc[at], pu[at], pj[at]};
    t += pt[at];
  }
  const bool none = ca == 0 || b.j < 0;
  best = none ? 0.0f : (float)b.c / (float)b.u;
  arg = none ? -1 : b.j;
  total = none ? 0.0 : t;
}

}  // namespace
