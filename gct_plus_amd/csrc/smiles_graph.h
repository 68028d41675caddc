// The labelled graph of one SMILES part as SmilesRandomizer.parse (randomize.py) reads it, stated once for the kernels
// that work on it: gct_smiles_randomize (randomize.hip), gct_smiles_key (molkey.hip) and gct_smiles_scaffold
// (scaffold.hip; smiles_key.h and smiles_walk.h hold what those share beyond the parse).  SmilesGraph is the part of a
// wave's LDS record that the parse fills -- each kernel's record derives from it and adds its own fields -- and
// rand_parse / rand_link are plain C++ over it, host-callable so that a CPU harness can run them under a sanitizer;
// smiles_stage_row is the row prelude of the randomize and key kernels: the staged span, its first <eos> and the first
// <sep> before it (the scaffold kernel keeps its own copy of the prelude and of key_part: on the shared ones it measured
// 0.7 % slower, 626.4 against 621.9 us at 32 768 rows, with 32 more instructions of 5 623 and the same barriers).
// An entry e[i] is the token's table word (class | ring number << 8 | bond order << 16 | unsupported << 20; a kernel may
// keep bits of its own from bit 21 up, the parse does not look at them).
#pragma once
#include "common.h"
#include "smiles_grammar.h"

namespace {

constexpr int kMaxDeg = 8;                                   // randomize.MAX_DEGREE

struct SmilesGraph {
  int32_t e[256];                                            // table word | the kernel's own bits
  uint32_t ring[GCT_GRAMMAR_MAX_RINGS];                      // open occurrence: atom | order << 8 | (symbol pos + 1) << 12
  int16_t bsym[256];                                         // bond -> position of its BOND token, -1: none
  int16_t par[256];                                          // atom -> chain parent (-1: none)
  uint16_t apos[256], stk[256], stamp[256];                  // stamp[a] = b + 1: a ring bond a-b was added at newest atom b
  uint8_t adj[256][kMaxDeg];                                 // atom -> its bonds, parse order
  uint8_t ba[256], bb[256];                                  // bond -> its ends, ba < bb
  uint8_t deg[256];                                          // per atom
};

__host__ __device__ inline void rand_link(SmilesGraph& w, int a, int b, int sym, int& nb, bool& unsup) {
  if (w.deg[a] >= kMaxDeg || w.deg[b] >= kMaxDeg) {
    unsup = true;
    return;
  }
  const int e = nb++;                                        // (a link takes an ATOM or a closing RING token: nb <= 254)
  w.ba[e] = (uint8_t)a, w.bb[e] = (uint8_t)b;
  w.bsym[e] = (int16_t)sym;
  w.adj[a][w.deg[a]++] = (uint8_t)e;
  w.adj[b][w.deg[b]++] = (uint8_t)e;
}

// Lane 0: the part e[lo, hi) parsed as decode.py smiles_walk reads it (the statement; chem_walk of chem.hip is the same
// walk over a whole row, kept apart because the check kernel is measurably slower on a shared template).  Returns false
// for SYNTAX.
__host__ __device__ inline bool rand_parse(SmilesGraph& w, int lo, int hi, int& atoms, int& bonds, bool& unsup) {
  int prev = GP_START, depth = 0, cur = -1, pend = 0, pendpos = -1, A = 0, nb = 0, sp = 0;
  uint64_t open = 0, here = 0;
  unsup = false;
  atoms = bonds = 0;
  for (int i = lo; i < hi; ++i) {
    const int ent = w.e[i], cls = ent & 0xFF;
    const bool ar = prev == GP_ATOM || prev == GP_RING, arc = ar || prev == GP_CLOSE;
    bool ok;
    if ((ent >> 20) & 1) unsup = true;
    switch (cls) {
      case GCT_GRAMMAR_ATOM: {
        ok = true;
        prev = GP_ATOM;
        here = 0;
        const int a = A++;                                   // (A <= hi - lo <= 255)
        w.apos[a] = (uint16_t)i;
        w.deg[a] = 0;
        w.par[a] = (int16_t)cur;
        w.stamp[a] = 0;
        if (cur >= 0) rand_link(w, cur, a, pendpos, nb, unsup);
        cur = a;
        pend = 0, pendpos = -1;
        break;
      }
      case GCT_GRAMMAR_BOND:
        ok = ar || prev == GP_OPEN || prev == GP_CLOSE;
        prev = ar ? GP_BOND_A : GP_BOND_B;
        pend = (ent >> 16) & 7, pendpos = i;
        break;
      case GCT_GRAMMAR_OPEN:
        ok = arc;
        prev = GP_OPEN;
        ++depth;
        if (ok) w.stk[sp++] = (uint16_t)cur;                 // (sp <= #OPEN tokens <= 255)
        break;
      case GCT_GRAMMAR_CLOSE:
        ok = arc && depth > 0;
        prev = GP_CLOSE;
        --depth;
        if (ok) cur = w.stk[--sp];
        pend = 0, pendpos = -1;
        break;
      case GCT_GRAMMAR_RING: {
        ok = ar || prev == GP_BOND_A;
        const int r = (ent >> 8) & 63;
        const uint64_t bit = 1ull << r;
        if (ok && (open & bit)) {
          if (here & bit) {
            ok = false;                                      // a ring does not close on the atom that opened it
          } else {
            open ^= bit;
            const uint32_t rec = w.ring[r];
            const int a = (int)(rec & 0xFFu), o = (int)((rec >> 8) & 7u), osym = (int)(rec >> 12) - 1;
            if ((o && pend && o != pend) || w.par[cur] == a || w.stamp[a] == cur + 1) {
              unsup = true;                                  // `check` reports RING_BOND
            } else {
              rand_link(w, a, cur, pendpos >= 0 ? pendpos : osym, nb, unsup);
              w.stamp[a] = (uint16_t)(cur + 1);
            }
          }
        } else if (ok) {
          open |= bit;
          here |= bit;
          w.ring[r] = (uint32_t)cur | ((uint32_t)pend << 8) | ((uint32_t)(pendpos + 1) << 12);
        }
        prev = GP_RING;
        pend = 0, pendpos = -1;
        break;
      }
      case GCT_GRAMMAR_DOT:
        ok = arc && depth == 0;
        prev = GP_DOT;
        unsup = true;
        cur = -1;
        pend = 0, pendpos = -1;
        break;
      default:                                               // <eos> cannot be here; <pad>, <sep> and banned tokens
        ok = false;
        break;
    }
    if (!ok) return false;
  }
  const bool arc = prev == GP_ATOM || prev == GP_RING || prev == GP_CLOSE;
  if (!(arc && depth == 0 && open == 0)) return false;       // the <eos> behind the part
  atoms = A, bonds = nb;
  return true;
}

struct StagedRow {
  const int64_t* yr;                                         // the span's first token (read only under j < g)
  int t0, g;                                                 // ys[row][t0, t0 + g): 0 <= g <= 256; out of range: 0, 0
  int E, S;                                                  // first <eos>; first <sep> in front of it (kNone: none)
};

// The whole wave: lane l stages tokens l + 64 t of the row's span ys[row][start[row], W) in w.e -- word(j, tok, known,
// table word or GCT_GRAMMAR_BANNED) is the kernel's own entry for the token at j, which gets (the token is <sep>) << 24
// on top -- and two butterflies find E and S.  A dead wave and a row whose start is out of range have g = 0, so no <eos>.
template <class Rec, class Word>
__device__ __forceinline__ StagedRow smiles_stage_row(Rec& w, const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n,
                                                      int row, const int32_t* __restrict__ start, int V,
                                                      const int32_t* __restrict__ table, int eos_id, int sep_id,
                                                      int lane, Word&& word) {
  const int t0 = row < n ? start[row] : W;
  const bool in_range = row < n && t0 >= 0 && t0 <= W && W - t0 <= 256;
  StagedRow r;
  r.t0 = in_range ? t0 : 0;
  r.g = in_range ? W - t0 : 0;
  r.yr = ys + (int64_t)row * ld_ys + r.t0;
  r.E = r.S = kNone;
  int sep_at = 0;                                            // bit t: token lane + 64 t is <sep>
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = lane + 64 * t;
    if (j < r.g) {
      const int64_t tok = r.yr[j];
      const bool known = tok >= 0 && tok < V;
      int x = word(j, tok, known, known ? table[tok] : GCT_GRAMMAR_BANNED);
      if (tok == sep_id) x |= 1 << 24, sep_at |= 1 << t;     // (sep_id -1: none)
      w.e[j] = x;
      if (tok == eos_id) r.E = min(r.E, j);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r.E = min(r.E, __shfl_xor(r.E, o, 64));
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (((sep_at >> t) & 1) && lane + 64 * t < r.E) r.S = min(r.S, lane + 64 * t);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r.S = min(r.S, __shfl_xor(r.S, o, 64));
  return r;
}

}  // namespace
