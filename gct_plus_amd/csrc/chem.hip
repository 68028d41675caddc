// The chemical validity check of finished rows: gct_smiles_check against decode.py SmilesChemistry.check (the
// statement).  It takes no part in the decode loop.  One wave per row, four rows per workgroup.  Lane l stages tokens
// l + 64 t of the row's span ys[r][start_r, W) in the wave's own LDS as (class | ring << 8 | chem << 16); lane 0 then
// walks the staged row once -- chem_walk: grammar_step's transitions for the first token without one,
// and the molecular graph with the branch stack, the per-atom sums and the open rings in LDS; after that lane l judges
// atoms l + 64 t and the wave reduces the finding with the smallest position.
// The walk is one lane's because every step of it depends on the one before (the chain atom after a CLOSE is whatever
// the stack holds); what it leaves in LDS is indexed dynamically there, never in registers, so nothing spills.  The walk
// and the per-atom verdict are plain C++, host-callable so that a CPU harness can run them under a sanitizer.
#include "common.h"
#include "smiles_grammar.h"

namespace {

struct ChemWave {
  int32_t e[256];
  uint32_t acc[256];                                         // atom -> sigma (bits 0..11) | largest order (12..14) |
  uint32_t ring[GCT_GRAMMAR_MAX_RINGS];                      //  aromatic neighbours (16..24)
  int16_t par[256];
  uint16_t apos[256], stk[256], stamp[256];
  int32_t res[4];                                            // syntax position (-1: none), atoms, ring bonds, ring finding
};
static_assert(sizeof(ChemWave) == 4368, "17 472 bytes of LDS per workgroup of four rows");

__host__ __device__ inline void chem_link(ChemWave& w, int a, int b, int order) {
  const bool ar_a = (w.e[w.apos[a]] >> 24) & 1, ar_b = (w.e[w.apos[b]] >> 24) & 1;
  uint32_t x = w.acc[a], y = w.acc[b];
  x += (uint32_t)order + (ar_b ? 1u << 16 : 0u);
  y += (uint32_t)order + (ar_a ? 1u << 16 : 0u);
  if (((x >> 12) & 7u) < (uint32_t)order) x = (x & ~(7u << 12)) | ((uint32_t)order << 12);
  if (((y >> 12) & 7u) < (uint32_t)order) y = (y & ~(7u << 12)) | ((uint32_t)order << 12);
  w.acc[a] = x;
  w.acc[b] = y;
}

// Lane 0: the staged span e[0, g) walked once, as decode.py smiles_walk reads a whole row (the statement; rand_parse of
// smiles_graph.h is the same walk over a part): <eos> goes to END and then only <pad> may follow.  Returns the first
// token without a transition, g for a span without <eos>, or -1, and the atoms, the ring closures and the first
// RING_BOND position (kNone: none).  ring[r]: atom | order << 16 of the open occurrence; par[a]: a's chain parent (-1: none);
// stamp[a] = b + 1 after a ring bond a-b was added while b was the newest atom: rings close on the newest atom only (no
// RING follows a CLOSE), so "a and b are bonded already" is par[b] == a || stamp[a] == b + 1.
__host__ __device__ __forceinline__ int chem_walk(ChemWave& w, int g, int& n_atoms, int& n_rings, int& first_clash) {
  int prev = GP_START, depth = 0, bad = -1;
  uint64_t open = 0, here = 0;
  int cur = -1, pend = 0, atoms = 0, rings = 0, sp = 0, ring_find = kNone;
  for (int i = 0; i < g; ++i) {
    const int ent = w.e[i], cls = ent & 0xFF;
    const bool ar = prev == GP_ATOM || prev == GP_RING, arc = ar || prev == GP_CLOSE;
    bool ok;
    if (prev == GP_END) {
      ok = cls == GCT_GRAMMAR_PAD;
    } else {
      switch (cls) {
        case GCT_GRAMMAR_ATOM: {
          ok = true;
          prev = GP_ATOM;
          here = 0;
          const int a = atoms++;
          w.apos[a] = (uint16_t)i;
          w.acc[a] = 0;
          w.par[a] = (int16_t)cur;
          w.stamp[a] = 0;
          if (cur >= 0) chem_link(w, cur, a, pend ? pend : 1);
          cur = a;
          pend = 0;
          break;
        }
        case GCT_GRAMMAR_BOND:
          ok = ar || prev == GP_OPEN || prev == GP_CLOSE;
          prev = ar ? GP_BOND_A : GP_BOND_B;
          pend = (ent >> 28) & 7;
          break;
        case GCT_GRAMMAR_OPEN:
          ok = arc;
          prev = GP_OPEN;
          ++depth;
          if (ok) w.stk[sp++] = (uint16_t)cur;             // (arc: an atom stands there; sp <= #tokens <= 256)
          break;
        case GCT_GRAMMAR_CLOSE:
          ok = arc && depth > 0;
          prev = GP_CLOSE;
          --depth;
          if (ok) cur = w.stk[--sp];
          pend = 0;
          break;
        case GCT_GRAMMAR_RING: {
          ok = ar || prev == GP_BOND_A;
          const int r = (ent >> 8) & 63;
          const uint64_t bit = 1ull << r;
          if (ok && (open & bit)) {
            if (here & bit) {
              ok = false;                                  // a ring does not close on the atom that opened it
            } else {
              open ^= bit;
              const int a = (int)(w.ring[r] & 0xFFFFu), o = (int)(w.ring[r] >> 16);
              ++rings;
              if ((o && pend && o != pend) || w.par[cur] == a || w.stamp[a] == cur + 1) {
                if (ring_find == kNone) ring_find = i;
              } else {
                chem_link(w, a, cur, pend ? pend : (o ? o : 1));
                w.stamp[a] = (uint16_t)(cur + 1);
              }
            }
          } else if (ok) {
            open |= bit;
            here |= bit;
            w.ring[r] = (uint32_t)cur | ((uint32_t)pend << 16);
          }
          prev = GP_RING;
          pend = 0;
          break;
        }
        case GCT_GRAMMAR_DOT:
          ok = arc && depth == 0;
          prev = GP_DOT;
          cur = -1;
          pend = 0;
          break;
        case GCT_GRAMMAR_EOS:
          ok = arc && depth == 0 && open == 0;
          prev = GP_END;
          break;
        default:
          ok = false;
          break;
      }
    }
    if (!ok) {
      bad = i;
      break;
    }
  }
  if (bad < 0 && prev != GP_END) bad = g;                    // no <eos> (an empty span: position 0)
  n_atoms = atoms, n_rings = rings, first_clash = ring_find;
  return bad;
}

// An atom's staged word and sums: GCT_CHEM_VALENCE, GCT_CHEM_AROMATIC or GCT_CHEM_OK.
__host__ __device__ inline int chem_verdict(int word, uint32_t x) {
  const int c = word >> 16;
  const int cap = c & 15, H = (c >> 4) & 15, mo = (int)((x >> 12) & 7u), anb = (int)((x >> 16) & 0x1FFu);
  const bool arom = (c >> 8) & 1, clike = (c >> 9) & 1;
  const int used = (int)(x & 0xFFFu) + H + (arom && clike && mo < 2 ? 1 : 0);
  if (cap != GCT_CHEM_NO_CAP && used > cap) return GCT_CHEM_VALENCE;
  return arom && anb < 2 ? GCT_CHEM_AROMATIC : GCT_CHEM_OK;
}

__global__ __launch_bounds__(256) void smiles_check_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start, int V,
    const int32_t* __restrict__ table, const int32_t* __restrict__ chem, int32_t* __restrict__ out) {
  __shared__ ChemWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  ChemWave& w = sh[wave];
  int t0 = live ? start[row] : W;
  const bool in_range = t0 >= 0 && t0 <= W && W - t0 <= 256;  // (ops.smiles_check checks; anything else: SYNTAX at 0)
  if (!in_range) t0 = W;
  const int g = W - t0;                                      // 0 <= g <= 256 tokens in the span
  if (live) {
    const int64_t* yr = ys + (int64_t)row * ld_ys + t0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = lane + 64 * t;
      if (j < g) {
        const int64_t tok = yr[j];
        w.e[j] = tok >= 0 && tok < V ? (table[tok] & 0xFFFF) | (chem[tok] << 16)
                                     : GCT_GRAMMAR_BANNED | (GCT_CHEM_NO_CAP << 16);
      }
    }
  }
  __syncthreads();
  if (live && lane == 0) {
    int atoms, rings, ring_find;
    w.res[0] = chem_walk(w, g, atoms, rings, ring_find);
    w.res[1] = atoms, w.res[2] = rings, w.res[3] = ring_find;
  }
  __syncthreads();
  if (!live) return;
  const int bad = w.res[0], atoms = w.res[1], rings = w.res[2];
  int key = kNone;                                           // position << 3 | status of the first finding
  if (bad < 0) {
    if (w.res[3] != kNone) key = (w.res[3] << 3) | GCT_CHEM_RING_BOND;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int a = lane + 64 * t;
      if (a < atoms) {
        const int p = w.apos[a], v = chem_verdict(w.e[p], w.acc[a]);
        if (v != GCT_CHEM_OK) key = min(key, (p << 3) | v);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
  }
  if (lane == 0) {
    int32_t* o4 = out + (int64_t)row * 4;
    if (bad >= 0) {
      o4[0] = GCT_CHEM_SYNTAX, o4[1] = bad, o4[2] = 0, o4[3] = 0;
    } else {
      o4[0] = key == kNone ? GCT_CHEM_OK : key & 7;
      o4[1] = key == kNone ? -1 : key >> 3;
      o4[2] = atoms, o4[3] = rings;
    }
  }
}

}  // namespace

extern "C" int gct_smiles_check(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                                const int32_t* table, const int32_t* chem, int32_t* out, void* stream) {
  GCT_CHECK_ARG(ys && start && table && chem && out && n >= 0 && V > 0, "smiles_check: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W, "smiles_check: %d token columns in rows of %lld", W, (long long)ld_ys);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_check_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys, W,
                     n, start, V, table, chem, out);
  GCT_LAUNCH_CHECK("smiles_check");
  return GCT_OK;
}
