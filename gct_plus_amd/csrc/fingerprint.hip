// Circular fingerprints and Tanimoto aggregates on the device: gct_smiles_fp and gct_fp_tanimoto against
// fingerprint.py (SmilesFingerprints.fingerprint is the statement for one part, fp_reference the batch rule,
// tanimoto_reference the rule of the aggregates).  The per-atom and per-pair arithmetic is smiles_fp.h's.
//
// gct_smiles_fp: one wave per row, four rows per workgroup, in smiles_key_kernel's shape.  Lane l stages tokens l + 64 t
// of the row's span -- the table word, and the token's 64-bit label in col[1], which nothing else needs until the first
// round of refinement overwrites it -- and the wave finds the first <eos> and the first <sep> in front of it; lane 0
// parses the molecule part (rand_parse of smiles_graph.h); lane l labels bonds l + 64 t and takes id_0 of atoms l + 64 t;
// GCT_FP_RADIUS rounds of key_refine follow, one atom per lane and pass, double-buffered in LDS; every generation's
// bits are OR-ed into the row's 32 LDS words (OR commutes: any order gives the same bits; no global atomics).
// LDS: sizeof(FpWave) = 11 152 bytes per wave (6 656 the parsed graph, 4 096 the two identifier buffers, 256 the bond
// labels, 128 the bits, 16 the part's header), 44 608 per workgroup of four rows -- less than the key kernel's 52 288:
// there is no label array of its own.
//
// gct_fp_tanimoto: a workgroup of 256 threads holds one row of `a` per thread in registers (32 VGPRs) and walks its
// split of `b` tile by tile: kTileB rows and their counts are staged in LDS, every lane reads the same word of b (a
// broadcast: one address per read, no bank conflict), and a pair costs 32 x (AND, popcount-accumulate), one division, one
// fp64 add and one integer compare.  The grid is (row tiles of a) x (splits of b); with more than one split the partials
// go to the workspace and tani_fold_kernel folds them in split order.  No atomics; the split count is a function of
// (n, m) alone (tani_plan), so the bits of `total` do not depend on the device.
#include "smiles_fp.h"

namespace {

struct FpWave : SmilesGraph {                                // e[i] also carries the key's bits from bit 21 (smiles_key.h)
  uint64_t col[2][256];                                      // atom -> identifier; col[1][j] first: label of token j
  uint8_t blab[256];                                         // bond -> label
  uint32_t bits[kFpWords];                                   // the row's bits
  int32_t res[4];                                            // graph?, atoms, bonds, status
};
static_assert(sizeof(FpWave) * 4 <= 64 * 1024, "four rows per workgroup must fit 64 KB of LDS");
static_assert(sizeof(FpWave) <= sizeof(SmilesGraph) + 2048 + 4096 + 256 + 16, "no larger than the key kernel's record");

__global__ __launch_bounds__(256) void smiles_fp_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start, int V,
    const int32_t* __restrict__ table, const int64_t* __restrict__ label, int eos_id, int sep_id,
    int64_t* __restrict__ bits_out, int32_t* __restrict__ info_out) {
  __shared__ FpWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  FpWave& w = sh[wave];
  if (lane < kFpWords) w.bits[lane] = 0;
  const StagedRow sr = smiles_stage_row(w, ys, ld_ys, W, n, row, start, V, table, eos_id, sep_id, lane,
                                        [&](int j, int64_t tok, bool known, int word) {
                                          w.col[1][j] = known ? (uint64_t)label[tok] : key_unknown_label(tok);
                                          return word & 0xFFFFFF;
                                        });
  const bool active = sr.E != kNone;                         // (a dead wave and a row out of range: g = 0, no <eos>)
  const int lo = sr.S != kNone ? sr.S + 1 : 0, hi = sr.E;    // the molecule: behind the first <sep>, or all of it
  __syncthreads();                                           // the staged row and the cleared bits
  if (lane == 0) {
    int A = 0, nb = 0, status = -1;
    if (active) {
      bool unsup;
      const bool parsed = rand_parse(w, lo, hi, A, nb, unsup);
      status = !parsed ? GCT_FP_SYNTAX : unsup ? GCT_FP_UNSUPPORTED : GCT_FP_GRAPH;
    }
    w.res[0] = active && status == GCT_FP_GRAPH, w.res[1] = A, w.res[2] = nb, w.res[3] = status;
  }
  __syncthreads();
  const bool graph = w.res[0] != 0;                          // (the same for the whole wave)
  const int nA = w.res[1], nB = w.res[2];
  if (graph) {
    for (int e = lane; e < nB; e += 64) w.blab[e] = (uint8_t)key_bond_label(w, e);
    for (int a = lane; a < nA; a += 64) {
      const uint64_t id = fp_id0(w, a);
      w.col[0][a] = id;
      fp_mark(w, id);
    }
  }
  __syncthreads();                                           // every label is read: col[1] is free
  for (int r = 0; r < GCT_FP_RADIUS; ++r) {
    if (graph)
      for (int a = lane; a < nA; a += 64) {
        const uint64_t id = key_refine(w, w.col[r & 1], a);
        w.col[(r + 1) & 1][a] = id;
        fp_mark(w, id);
      }
    __syncthreads();
  }
  uint32_t mine = lane < kFpWords ? w.bits[lane] : 0u;
  int pop = __builtin_popcount(mine);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pop += __shfl_xor(pop, o, 64);
  const uint32_t next = (uint32_t)__shfl_down((int)mine, 1, 64);
  if (live && lane < kFpWords && !(lane & 1))
    bits_out[(int64_t)row * (GCT_FP_BITS / 64) + (lane >> 1)] = (int64_t)((uint64_t)mine | ((uint64_t)next << 32));
  if (live && lane == 0) {
    int32_t* o4 = info_out + (int64_t)row * 4;
    o4[0] = w.res[3], o4[1] = pop, o4[2] = nA, o4[3] = nB;
  }
}

// ------------------------------------------------------------------------------------------------- Tanimoto
constexpr int kTileA = 256;                                  // rows of a per workgroup, one per thread
constexpr int kTileB = 128;                                  // rows of b per LDS tile: 16 KB of words, 512 B of counts
constexpr int kTargetGroups = 1024;                          // four workgroups on each of 256 CUs, whatever the device has
constexpr int kMaxSplits = 256;

struct TaniPlan {
  int row_tiles, splits, tiles_per_split;
};

// (n, m) -> the grid.  Enough splits of b to reach kTargetGroups workgroups, never more than tiles of b, and every
// split holds at least one tile.  A function of the shapes alone.
TaniPlan tani_plan(int n, int m) {
  TaniPlan p;
  p.row_tiles = (n + kTileA - 1) / kTileA;
  const int tiles = (m + kTileB - 1) / kTileB;
  int want = p.row_tiles > 0 ? (kTargetGroups + p.row_tiles - 1) / p.row_tiles : 1;
  want = want < 1 ? 1 : want > kMaxSplits ? kMaxSplits : want;
  want = want > tiles ? (tiles > 0 ? tiles : 1) : want;
  p.tiles_per_split = tiles > 0 ? (tiles + want - 1) / want : 1;
  p.splits = tiles > 0 ? (tiles + p.tiles_per_split - 1) / p.tiles_per_split : 1;
  return p;
}

// The workspace of `splits` > 1: four arrays [splits][n] -- c, u, j (int32) and the total (fp64, first: 8-byte aligned).
struct TaniWs {
  double* t;
  int32_t *c, *u, *j;
};

TaniWs tani_ws(void* ws, int n, int splits) {
  const size_t k = (size_t)n * (size_t)splits;
  TaniWs r;
  r.t = (double*)ws;
  r.c = (int32_t*)(r.t + k);
  r.u = r.c + k;
  r.j = r.u + k;
  return r;
}

__global__ __launch_bounds__(kTileA) void tani_kernel(
    const int64_t* __restrict__ a, int64_t lda, const int32_t* __restrict__ cnt_a, int n, const int64_t* __restrict__ b,
    int64_t ldb, const int32_t* __restrict__ cnt_b, int m, int p, int tiles_per_split, int splits, TaniWs ws,
    float* __restrict__ best_out, int32_t* __restrict__ arg_out, double* __restrict__ total_out) {
  __shared__ __attribute__((aligned(16))) uint32_t sb[kTileB * kFpWords];
  __shared__ int32_t sc[kTileB];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kTileA + tid;
  const bool live = i < n;
  uint32_t av[kFpWords];
  {
    const int64_t* ar = a + (int64_t)(live ? i : 0) * lda;   // (a dead thread reads row 0 and writes nothing; n >= 1)
#pragma unroll
    for (int k = 0; k < kFpWords / 2; ++k) {
      const uint64_t x = (uint64_t)ar[k];
      av[2 * k] = (uint32_t)x, av[2 * k + 1] = (uint32_t)(x >> 32);
    }
  }
  const int ca = cnt_a[live ? i : 0];
  const int split = blockIdx.y;
  const int64_t first = (int64_t)split * tiles_per_split * kTileB;
  const int j_end = (int)min((int64_t)m, first + (int64_t)tiles_per_split * kTileB);
  TaniBest best = tani_none();
  double total = 0.0;
  for (int jb = (int)first; jb < j_end; jb += kTileB) {      // (first < m: every split holds a tile)
    const int rows = min(kTileB, j_end - jb);
    __syncthreads();                                         // the last tile is read
    for (int q = tid; q < rows * (kFpWords / 2); q += kTileA) {
      const int r = q >> 4, k = q & 15;                      // 16 64-bit words per row of b
      const uint64_t x = (uint64_t)b[(int64_t)(jb + r) * ldb + k];
      sb[r * kFpWords + 2 * k] = (uint32_t)x, sb[r * kFpWords + 2 * k + 1] = (uint32_t)(x >> 32);
    }
    if (tid < rows) sc[tid] = cnt_b[jb + tid];
    __syncthreads();
    if (p == 2)
      tani_tile<2>(av, ca, sb, sc, jb, jb, jb + rows, best, total);
    else
      tani_tile<1>(av, ca, sb, sc, jb, jb, jb + rows, best, total);
  }
  if (!live) return;
  if (splits == 1) {
    const bool none = ca == 0 || best.j < 0;
    best_out[i] = none ? 0.0f : (float)best.c / (float)best.u;
    arg_out[i] = none ? -1 : best.j;
    total_out[i] = none ? 0.0 : total;
  } else {
    const size_t at = (size_t)split * (size_t)n + (size_t)i;
    ws.c[at] = best.c, ws.u[at] = best.u, ws.j[at] = best.j, ws.t[at] = total;
  }
}

__global__ __launch_bounds__(256) void tani_fold_kernel(TaniWs ws, const int32_t* __restrict__ cnt_a, int n, int splits,
                                                        float* __restrict__ best_out, int32_t* __restrict__ arg_out,
                                                        double* __restrict__ total_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float best;
  int32_t arg;
  double total;
  tani_fold(ws.c + i, ws.u + i, ws.j + i, ws.t + i, (size_t)n, splits, cnt_a[i], best, arg, total);
  best_out[i] = best, arg_out[i] = arg, total_out[i] = total;
}

__global__ void tani_empty_kernel(int n, float* __restrict__ best_out, int32_t* __restrict__ arg_out,
                                  double* __restrict__ total_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) best_out[i] = 0.0f, arg_out[i] = -1, total_out[i] = 0.0;
}

}  // namespace

extern "C" int gct_smiles_fp(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                             const int32_t* table32, const int64_t* label64, int pad_id, int eos_id, int sep_id,
                             int64_t* bits_out, int32_t* info_out, void* stream) {
  GCT_CHECK_ARG(ys && start && table32 && label64 && bits_out && info_out && n >= 0 && V > 0, "smiles_fp: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W, "smiles_fp: %d token columns in rows of %lld", W, (long long)ld_ys);
  GCT_CHECK_ARG(pad_id >= 0 && pad_id < V && eos_id >= 0 && eos_id < V && sep_id >= -1 && sep_id < V,
                "smiles_fp: a token id outside the vocabulary of %d", V);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_fp_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys, W, n,
                     start, V, table32, label64, eos_id, sep_id, bits_out, info_out);
  GCT_LAUNCH_CHECK("smiles_fp");
  return GCT_OK;
}

extern "C" int gct_fp_tanimoto_tile_b(void) { return kTileB; }

extern "C" int gct_fp_tanimoto_splits(int n, int m) { return n < 0 || m < 0 ? 0 : tani_plan(n, m).splits; }

extern "C" int64_t gct_fp_tanimoto_ws_bytes(int n, int m) {
  if (n < 0 || m < 0) return 0;
  const int splits = tani_plan(n, m).splits;
  return splits > 1 ? (int64_t)n * splits * (int64_t)(sizeof(double) + 3 * sizeof(int32_t)) : 0;
}

extern "C" int gct_fp_tanimoto(const int64_t* a, int64_t lda, const int32_t* cnt_a, int n, const int64_t* b, int64_t ldb,
                               const int32_t* cnt_b, int m, int p, void* ws, int64_t ws_bytes, float* best_out,
                               int32_t* arg_out, double* total_out, void* stream) {
  GCT_CHECK_ARG(n >= 0 && m >= 0 && (n == 0 || (a && cnt_a && best_out && arg_out && total_out)) &&
                    (m == 0 || (b && cnt_b)), "fp_tanimoto: bad args");
  GCT_CHECK_ARG(lda >= GCT_FP_BITS / 64 && ldb >= GCT_FP_BITS / 64, "fp_tanimoto: rows of %lld and %lld words, a "
                "fingerprint has %d", (long long)lda, (long long)ldb, GCT_FP_BITS / 64);
  GCT_CHECK_ARG(p == 1 || p == 2, "fp_tanimoto: p = %d, must be 1 or 2", p);
  GCT_CHECK_ARG(m <= (1 << 30), "fp_tanimoto: %d rows of b, at most 2^30", m);
  if (n == 0) return GCT_OK;
  if (m == 0) {
    hipLaunchKernelGGL(tani_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       best_out, arg_out, total_out);
    GCT_LAUNCH_CHECK("fp_tanimoto");
    return GCT_OK;
  }
  const TaniPlan plan = tani_plan(n, m);
  const int64_t need = gct_fp_tanimoto_ws_bytes(n, m);
  GCT_CHECK_ARG(need == 0 || (ws && ws_bytes >= need && ((uintptr_t)ws & 7) == 0),
                "fp_tanimoto: %d splits need an 8-byte aligned workspace of %lld bytes, got %lld", plan.splits,
                (long long)need, (long long)ws_bytes);
  const TaniWs w = plan.splits > 1 ? tani_ws(ws, n, plan.splits) : TaniWs{nullptr, nullptr, nullptr, nullptr};
  hipLaunchKernelGGL(tani_kernel, dim3((unsigned)plan.row_tiles, (unsigned)plan.splits), dim3(kTileA), 0,
                     (hipStream_t)stream, a, lda, cnt_a, n, b, ldb, cnt_b, m, p, plan.tiles_per_split, plan.splits, w,
                     best_out, arg_out, total_out);
  GCT_LAUNCH_CHECK("fp_tanimoto");
  if (plan.splits > 1) {
    hipLaunchKernelGGL(tani_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, cnt_a,
                       n, plan.splits, best_out, arg_out, total_out);
    GCT_LAUNCH_CHECK("fp_tanimoto fold");
  }
  return GCT_OK;
}
