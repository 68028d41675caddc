// The randomiser's write-out (randomize.py SmilesRandomizer.write_out: passes 1 and 2 of `randomize`), stated once for
// the kernels that spell a parsed graph: gct_smiles_randomize (randomize.hip) and gct_smiles_scaffold (scaffold.hip).
// rand_walk is a template over the wave's LDS record Rec, which derives from SmilesGraph (smiles_graph.h) and adds
//   int32_t out[256]                            the new row: a literal token id (>= 0) or -(j + 1), the token at position j
//   uint8_t seen[256], pbond[256], left[256]    per atom; pbond: the bond the search came by (0xFF: root)
//   uint8_t role[256], rnum[256]                per bond; role 0 unseen, 1 tree, 2 / 3 ring opened at ba / bb
//   uint8_t perm[256]                           the input atom of the k-th output atom
// Plain C++, host-callable so that a CPU harness can run it under a sanitizer.
#pragma once
#include "smiles_graph.h"

namespace {

// A lane's atom a: the Fisher-Yates shuffle of its bond list adj[a] of d >= 2 entries, back to front.  Step i swaps
// entry i with entry floor(x (i + 1) / 2^32), x being word i - 1 of c0 and, from the fifth step on, word i - 5 of c1 (the
// atom's two Philox results; c1 is not looked at for d <= 5).  The words are picked by constants: no per-lane array.
template <class Rec>
__host__ __device__ inline void rand_shuffle_atom(Rec& w, int a, int d, uint4 c0, uint4 c1) {
  for (int i = d - 1; i >= 1; --i) {
    const uint4 c = i - 1 < 4 ? c0 : c1;
    const int k = (i - 1) & 3;
    const uint32_t x = k == 0 ? c.x : (k == 1 ? c.y : (k == 2 ? c.z : c.w));
    const int j = (int)(((uint64_t)x * (uint32_t)(i + 1)) >> 32);
    const uint8_t ti = w.adj[a][i], tj = w.adj[a][j];
    w.adj[a][i] = tj, w.adj[a][j] = ti;
  }
}

// Lane 0: passes 1 and 2 of the statement for a part of A atoms rooted at `root`, into w.out[opos, opos + room) and
// w.perm[abase, abase + A).  seen / left / role of the part are cleared by the caller.  Returns the length of the new
// spelling (it may exceed room: nothing is written past it), or -1 when no ring number was free.
template <class Rec>
__host__ __device__ int rand_walk(Rec& w, int A, int root, int opos, int room, int abase,
                                  const int32_t* __restrict__ ring_ids, int n_rings, int open_id, int close_id) {
  // pass 1
  int sp = 0;
  w.seen[root] = 1;
  w.pbond[root] = 0xFF;
  w.stk[sp++] = (uint16_t)root;                              // atom | next list index << 8; sp <= A <= 255
  while (sp > 0) {
    const int f = w.stk[sp - 1], u = f & 0xFF, i = f >> 8;
    if (i == w.deg[u]) {
      --sp;
      continue;
    }
    w.stk[sp - 1] = (uint16_t)(u | ((i + 1) << 8));
    const int e = w.adj[u][i];
    if (e == w.pbond[u] || w.role[e] != 0) continue;
    const int v = w.ba[e] ^ w.bb[e] ^ u;
    if (w.seen[v]) {
      w.role[e] = v == w.ba[e] ? 2 : 3;                      // v is an ancestor: the opening end
    } else {
      w.seen[v] = 1;
      w.pbond[v] = (uint8_t)e;
      w.role[e] = 1;
      ++w.left[u];
      w.stk[sp++] = (uint16_t)v;
    }
  }
  // pass 2
  uint64_t free_ = (1ull << n_rings) - 1;                    // (n_rings <= 63) bit k: ring_ids[k] is free
  int k = 0, pk = 0;
  bool no_ring = false;
  auto emit = [&](int v) {
    if (k < room) w.out[opos + k] = v;
    ++k;
  };
  auto emit_atom = [&](int u) {
    emit(-((int)w.apos[u] + 1));
    w.perm[abase + pk++] = (uint8_t)(abase + u);             // (every atom is emitted once: pk <= A)
    uint64_t closed = 0;
    const int d = w.deg[u];
    for (int i = 0; i < d; ++i) {
      const int e = w.adj[u][i], r = w.role[e];
      if (r < 2) continue;
      if ((r == 2 ? w.ba[e] : w.bb[e]) == u) {
        if (w.bsym[e] >= 0) emit(-((int)w.bsym[e] + 1));
        if (!free_) {
          no_ring = true;
          return;
        }
        const int idx = __builtin_ctzll(free_);
        free_ &= free_ - 1;
        w.rnum[e] = (uint8_t)idx;
        emit(ring_ids[idx]);
      } else {
        const int idx = w.rnum[e];
        emit(ring_ids[idx]);
        closed |= 1ull << idx;
      }
    }
    free_ |= closed;                                         // free again from the next atom on
  };
  emit_atom(root);
  sp = 0;
  w.stk[sp++] = (uint16_t)root;                              // atom | next list index << 8 | inside parentheses << 12
  while (sp > 0 && !no_ring) {
    const int f = w.stk[sp - 1], u = f & 0xFF, paren = (f >> 12) & 1, d = w.deg[u];
    int i = (f >> 8) & 15;
    while (i < d && !(w.role[w.adj[u][i]] == 1 && w.adj[u][i] != w.pbond[u])) ++i;
    if (i == d) {
      --sp;
      if (paren) emit(close_id);
      continue;
    }
    const int e = w.adj[u][i], v = w.ba[e] ^ w.bb[e] ^ u;
    w.stk[sp - 1] = (uint16_t)(u | ((i + 1) << 8) | (paren << 12));
    const int branch = --w.left[u] > 0;
    if (branch) emit(open_id);
    if (w.bsym[e] >= 0) emit(-((int)w.bsym[e] + 1));
    emit_atom(v);
    w.stk[sp++] = (uint16_t)(v | (branch << 12));
  }
  return no_ring ? -1 : k;
}

}  // namespace
