// Molecular descriptors on the device: gct_smiles_desc against descriptor.py (SmilesDescriptors.describe is the
// statement for one part, desc_reference the batch rule).  Ring perception and the per-atom and per-bond arithmetic
// are smiles_desc.h's.
//
// One wave per row, four rows per workgroup, in smiles_key_kernel's shape.  Lane l stages tokens l + 64 t of the row's
// span -- the table word and the token's desc32 word -- and the wave finds the first <eos> and the first <sep> in front
// of it; lane 0 parses the molecule part (rand_parse of smiles_graph.h); then, for a part with a graph,
//   lane l takes bonds l + 64 t: one breadth-first search per bond from one end with the bond excluded (visited and
//     frontier sets in four 64-bit registers each, the bond lists read from LDS) gives s(e), and with it the bond's class;
//   lane l takes atoms l + 64 t: sigma, the bond-class counts, hydrogens, the TPSA line, the mass, whether the atom is
//     UNKNOWN, and the lowest atom reached over AROMATIC ring bonds (the representative of the atom's component of that
//     subgraph: a second search of the same kind, over those bonds only);
//   lane l takes bonds l + 64 t again for the rotatable bonds, which need both ends' TRIPLE flags;
//   butterflies over the wave sum the integers (no atomics), and lane 0 writes the row's twelve words.
// LDS: sizeof(DescWave) = 7 952 bytes per wave (6 656 the parsed graph, 512 the desc32 words, 3 x 256 ring sizes, bond
// classes and atom flags, 16 the part's header), 31 808 per workgroup of four rows -- less than the key kernel's 13 072
// per wave: there are no labels and no colours.
#include "smiles_desc.h"

namespace {

struct DescWave : SmilesGraph {                              // e[i] also carries the key's bits from bit 21 (smiles_key.h)
  uint16_t dsc[256];                                         // token position -> desc32 word
  uint8_t rsz[256];                                          // bond -> s(e), 0: no ring bond
  uint8_t bcls[256];                                         // bond -> class
  uint8_t aflag[256];                                        // atom -> bit 0: has a TRIPLE bond
  int32_t res[4];                                            // status, atoms, bonds
};
static_assert(sizeof(DescWave) * 4 <= 64 * 1024, "four rows per workgroup must fit 64 KB of LDS");
static_assert(sizeof(DescWave) <= 13072, "no larger than the key kernel's record");

__device__ __forceinline__ int desc_wave_sum(int x) {        // a butterfly in a fixed order; integers: any order agrees
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__global__ __launch_bounds__(256) void smiles_desc_kernel(
    const int64_t* __restrict__ ys, int64_t ld_ys, int W, int n, const int32_t* __restrict__ start, int V,
    const int32_t* __restrict__ table, const int32_t* __restrict__ desc, int eos_id, int sep_id,
    int32_t* __restrict__ values_out) {
  __shared__ DescWave sh[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  const bool live = row < n;
  DescWave& w = sh[wave];
  const StagedRow sr = smiles_stage_row(w, ys, ld_ys, W, n, row, start, V, table, eos_id, sep_id, lane,
                                        [&](int j, int64_t tok, bool known, int word) {
                                          w.dsc[j] = (uint16_t)(known ? desc[tok] : 0);
                                          return word & 0xFFFFFF;
                                        });
  const bool active = sr.E != kNone;                         // (a dead wave and a row out of range: g = 0, no <eos>)
  const int lo = sr.S != kNone ? sr.S + 1 : 0, hi = sr.E;    // the molecule: behind the first <sep>, or all of it
  __syncthreads();                                           // the staged row
  if (lane == 0) {
    int A = 0, nb = 0, status = -1;
    if (active) {
      bool unsup;
      const bool parsed = rand_parse(w, lo, hi, A, nb, unsup);
      status = !parsed ? GCT_DESC_SYNTAX : unsup ? GCT_DESC_UNSUPPORTED : GCT_DESC_OK;
    }
    w.res[0] = status, w.res[1] = A, w.res[2] = nb;
  }
  __syncthreads();
  const int parsed_status = w.res[0];                        // (the same for the whole wave)
  const bool graph = parsed_status == GCT_DESC_OK;
  const int nA = w.res[1], nB = w.res[2];
  int ring_bonds = 0, arom_bonds = 0;
  if (graph)
    for (int e = lane; e < nB; e += 64) {
      const int s = desc_ring_size(w, e), c = desc_bond_class(w, e, s);
      w.rsz[e] = (uint8_t)s, w.bcls[e] = (uint8_t)c;
      ring_bonds += s != 0;
      arom_bonds += s != 0 && c == kDescAromatic;
    }
  __syncthreads();                                           // every bond's ring size and class
  int unknown = 0, hyd = 0, mass = 0, charge = 0, hbd = 0, hba = 0, tpsa = 0, touched = 0, comps = 0;
  if (graph)
    for (int a = lane; a < nA; a += 64) {
      const DescAtom r = desc_atom(w, a);
      w.aflag[a] = (uint8_t)r.triple;
      unknown += r.unknown, hyd += r.hydrogens, mass += r.mass, charge += r.charge, hbd += r.hbd, hba += r.hba;
      tpsa += r.tpsa, touched += r.touched;
      if (r.touched) comps += desc_component(w, a) == a;
    }
  __syncthreads();                                           // every atom's flag
  int rot = 0;
  if (graph)
    for (int e = lane; e < nB; e += 64) rot += desc_rotatable(w, e);
  unknown = desc_wave_sum(unknown), hyd = desc_wave_sum(hyd), mass = desc_wave_sum(mass);
  charge = desc_wave_sum(charge), hbd = desc_wave_sum(hbd), hba = desc_wave_sum(hba), tpsa = desc_wave_sum(tpsa);
  touched = desc_wave_sum(touched), comps = desc_wave_sum(comps), rot = desc_wave_sum(rot);
  ring_bonds = desc_wave_sum(ring_bonds), arom_bonds = desc_wave_sum(arom_bonds);
  if (live && lane == 0) {
    int32_t* o = values_out + (int64_t)row * GCT_DESC_COLUMNS;
    const bool ok = graph && unknown == 0;
    o[0] = graph && unknown ? GCT_DESC_UNKNOWN_ATOM : parsed_status;
    o[1] = nA;                                               // (0 unless the part parsed)
    o[2] = ok ? hyd : 0, o[3] = ok ? mass : 0, o[4] = ok ? charge : 0, o[5] = ok ? hbd : 0, o[6] = ok ? hba : 0;
    o[7] = ok ? rot : 0, o[8] = ok ? nB - nA + 1 : 0, o[9] = ok ? arom_bonds - touched + comps : 0;
    o[10] = ok ? tpsa : 0, o[11] = ok ? ring_bonds : 0;
  }
}

}  // namespace

extern "C" int gct_smiles_desc(const int64_t* ys, int64_t ld_ys, int W, int n, const int32_t* start, int V,
                               const int32_t* table32, const int32_t* desc32, int pad_id, int eos_id, int sep_id,
                               int32_t* values_out, void* stream) {
  GCT_CHECK_ARG(ys && start && table32 && desc32 && values_out && n >= 0 && V > 0, "smiles_desc: bad args");
  GCT_CHECK_ARG(W >= 0 && ld_ys >= W, "smiles_desc: %d token columns in rows of %lld", W, (long long)ld_ys);
  GCT_CHECK_ARG(pad_id >= 0 && pad_id < V && eos_id >= 0 && eos_id < V && sep_id >= -1 && sep_id < V,
                "smiles_desc: a token id outside the vocabulary of %d", V);
  if (n == 0) return GCT_OK;
  hipLaunchKernelGGL(smiles_desc_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ys, ld_ys, W, n,
                     start, V, table32, desc32, eos_id, sep_id, values_out);
  GCT_LAUNCH_CHECK("smiles_desc");
  return GCT_OK;
}
