// CPU harness of the host-callable parts of the SMILES kernels (tools/smiles_walk_check.py builds and drives it):
// rand_parse of csrc/smiles_graph.h, the check's walk and verdict (csrc/chem.hip), rand_shuffle_atom and
// rand_walk (csrc/smiles_walk.h), the per-atom key functions (csrc/smiles_key.h), sca_peel / sca_shell / sca_nh /
// sca_compact (csrc/scaffold.hip), the fingerprint and Tanimoto functions (csrc/smiles_fp.h) and the ring perception and
// per-atom descriptor functions (csrc/smiles_desc.h) run on the HOST over one
// LDS record per case, bond by bond and atom by atom as the kernels' lanes do, so that AddressSanitizer and UBSan see
// every index they form -- the scaffold's aliased walk buffers, the fingerprint's labels in its second identifier buffer
// and reused parse fields included.  No GPU is touched.  Usage: smiles_walk_host MODE FILE; the file holds the count and
// then per case, by mode,
//   check      L / L staged words
//   randomize  L calls n_rings open_id close_id room / L table words / 4 * calls stream words / n_rings ring ids
//   key        L / L table words / L token labels (unsigned 64-bit)
//   scaffold   L n_rings open_id close_id room nh_id nh_word / nh_label / L table words (| 1 << 25 on `n`) / L token
//              labels / n_rings ring ids
//   fingerprint L / L table words / L token labels (unsigned 64-bit)
//   tanimoto   na nb p tile tiles_per_split / na + nb rows: count and 32 words of 32 bits
//   descriptor L / L table words / L desc32 words
// and one line goes out per case:
//   check      status position atoms ring_bonds
//   randomize  status, and for a rewritten part the length, the row's LDS entries | perm
//   key        status key (unsigned) atoms bonds
//   scaffold   status key atoms-kept length | the row's entries | member per input atom
//   fingerprint status atoms bonds and the 16 words (unsigned 64-bit)
//   tanimoto   per row of a: best (the fp32's bits) arg total (the fp64's bits)
//   descriptor the row's twelve integers
// (an entry is a literal id, or -(j + 1) for the token at position j).
#include "../gct_plus_amd/csrc/chem.hip"
#include "../gct_plus_amd/csrc/randomize.hip"
#include "../gct_plus_amd/csrc/molkey.hip"
#include "../gct_plus_amd/csrc/scaffold.hip"
#include "../gct_plus_amd/csrc/fingerprint.hip"
#include "../gct_plus_amd/csrc/descriptor.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

void gct_set_error(const char*, ...) {}

static FILE* f;

static long long rd() {                                      // the next number; a short file ends the run
  long long x;
  if (fscanf(f, "%lld", &x) != 1) exit(2);
  return x;
}

static uint64_t rdu() {
  unsigned long long u;
  if (fscanf(f, "%llu", &u) != 1) exit(2);
  return (uint64_t)u;
}

static int rd_in(int lo, int hi) {
  const long long x = rd();
  if (x < lo || x > hi) exit(2);
  return (int)x;
}

template <class Rec>
static void fresh(Rec* w, int L) {                           // nothing may rely on a cleared record
  memset((void*)w, 0xAB, sizeof(*w));
  for (int i = 0; i < L; ++i) w->e[i] = (int32_t)rd();
}

template <class Rec>
static uint64_t graph_key(Rec* w, int A, int nb) {           // key_graph_sum, atom by atom
  for (int e = 0; e < nb; ++e) w->blab[e] = (uint8_t)key_bond_label(*w, e);
  for (int a = 0; a < A; ++a) w->col[0][a] = key_profile(*w, a);
  for (int r = 0; r < GCT_KEY_ROUNDS; ++r)
    for (int a = 0; a < A; ++a) w->col[(r + 1) & 1][a] = key_refine(*w, w->col[r & 1], a);
  uint64_t sum = 0;
  for (int a = 0; a < A; ++a) sum += key_mix(w->col[GCT_KEY_ROUNDS & 1][a]);
  return key_combine(sum, A, nb);
}

static void run_check(ChemWave* w) {
  const int g = rd_in(0, 256);
  fresh(w, g);
  int atoms, rings, ring_find;
  const int bad = chem_walk(*w, g, atoms, rings, ring_find);
  if (bad >= 0) {
    printf("%d %d 0 0\n", GCT_CHEM_SYNTAX, bad);
    return;
  }
  int key = ring_find == kNone ? kNone : (ring_find << 3) | GCT_CHEM_RING_BOND;
  for (int a = 0; a < atoms; ++a) {
    const int p = w->apos[a], v = chem_verdict(w->e[p], w->acc[a]);
    if (v != GCT_CHEM_OK && ((p << 3) | v) < key) key = (p << 3) | v;
  }
  printf("%d %d %d %d\n", key == kNone ? GCT_CHEM_OK : key & 7, key == kNone ? -1 : key >> 3, atoms, rings);
}

static void run_randomize(RandWave* w) {
  const int L = rd_in(0, 255), calls = rd_in(1 + 2 * L, 1 << 20), nr = rd_in(0, 63);
  const int open_id = (int)rd(), close_id = (int)rd(), room = rd_in(0, 256);
  fresh(w, L);
  std::vector<uint4> words((size_t)calls);
  std::vector<int32_t> rid(64, -1);
  for (uint4& c : words) c.x = (uint32_t)rd(), c.y = (uint32_t)rd(), c.z = (uint32_t)rd(), c.w = (uint32_t)rd();
  for (int i = 0; i < nr; ++i) rid[i] = (int32_t)rd();
  int A, nb;
  bool unsup;
  if (!rand_parse(*w, 0, L, A, nb, unsup)) {
    printf("%d\n", GCT_RAND_SYNTAX);
    return;
  }
  if (unsup) {
    printf("%d\n", GCT_RAND_UNSUPPORTED);
    return;
  }
  for (int e = 0; e < nb; ++e) w->role[e] = 0;
  for (int a = 0; a < A; ++a) {
    w->seen[a] = 0, w->left[a] = 0;
    if (w->deg[a] >= 2) rand_shuffle_atom(*w, a, w->deg[a], words[1 + 2 * a], words[2 + 2 * a]);
  }
  const int root = (int)(((uint64_t)words[0].y * (uint32_t)A) >> 32);
  const int k = rand_walk(*w, A, root, 0, room, 0, rid.data(), nr, open_id, close_id);
  if (k < 0) {
    printf("%d\n", GCT_RAND_NO_RING);
  } else if (k > room) {
    printf("%d %d\n", GCT_RAND_TOO_LONG, k);
  } else {
    printf("%d %d", GCT_RAND_OK, k);
    for (int i = 0; i < k; ++i) printf(" %d", w->out[i]);
    printf(" |");
    for (int a = 0; a < A; ++a) printf(" %d", (int)w->perm[a]);
    printf("\n");
  }
}

static void run_key(KeyWave* w) {
  const int L = rd_in(0, 255);
  fresh(w, L);
  for (int i = 0; i < L; ++i) w->lab[i] = rdu();
  int A, nb;
  bool unsup;
  const bool parsed = rand_parse(*w, 0, L, A, nb, unsup);
  if (!parsed || unsup)
    printf("%d %llu %d %d\n", parsed ? GCT_KEY_STRING_UNSUPPORTED : GCT_KEY_STRING_SYNTAX,
           (unsigned long long)key_string(*w, 0, L), A, nb);
  else
    printf("%d %llu %d %d\n", GCT_KEY_GRAPH, (unsigned long long)graph_key(w, A, nb), A, nb);
}

static void run_scaffold(ScaWave* w) {
  const int L = rd_in(0, 255), nr = rd_in(0, 63), open_id = (int)rd(), close_id = (int)rd(), room = rd_in(0, 255);
  const int nh_id = (int)rd(), nh_word = (int)rd();
  const uint64_t nh_label = rdu();
  fresh(w, L);
  for (int i = 0; i < L; ++i) w->lab[i] = rdu();
  std::vector<int32_t> rid(64, -1);
  for (int i = 0; i < nr; ++i) rid[i] = (int32_t)rd();
  int A, nb;
  bool unsup;
  const bool parsed = rand_parse(*w, 0, L, A, nb, unsup);
  if (!parsed || unsup) {
    printf("%d 0 0 0 | |\n", parsed ? GCT_SCA_UNSUPPORTED : GCT_SCA_SYNTAX);
    return;
  }
  for (int e = 0; e < nb; ++e) w->blab[e] = (uint8_t)key_bond_label(*w, e);
  for (int a = 0; a < A; ++a) w->par[a] = 1, w->stamp[a] = w->deg[a];
  const int core = sca_peel(*w, A);
  int status = GCT_SCA_OK, nK = 0, nBk = 0, len = 0;
  uint64_t key = 0;
  std::vector<int> member(A, 0);
  if (core == 0) {
    status = GCT_SCA_ACYCLIC;
  } else {
    bool missing = false;
    for (int e = 0; e < nb; ++e) sca_shell(*w, e);
    for (int a = 0; a < A; ++a) missing |= sca_nh(*w, a, nh_id, nh_word, nh_label);
    sca_compact(*w, A, nb, nK, nBk);
    for (int a = 0; a < A; ++a) member[a] = w->par[a];
    if (missing) {
      status = GCT_SCA_NO_TOKEN;
    } else {
      key = graph_key(w, nK, nBk);
      memset((void*)w->col, 0xCD, sizeof(w->col));           // the walk's buffers alias it
      for (int e = 0; e < nBk; ++e) w->role[e] = 0;
      for (int a = 0; a < nK; ++a) w->seen[a] = 0, w->left[a] = 0;
      len = rand_walk(*w, nK, 0, 0, room, 0, rid.data(), nr, open_id, close_id);
      if (len < 0) status = GCT_SCA_NO_RING;
      else if (len > room) status = GCT_SCA_TOO_LONG;
      if (status != GCT_SCA_OK) len = 0;
    }
  }
  printf("%d %llu %d %d |", status, (unsigned long long)key, nK, len);
  for (int i = 0; i < len; ++i) {
    const int v = w->out[i];
    printf(" %d", v >= 0 ? v : (w->e[-v - 1] & kSubst) ? nh_id : v);
  }
  printf(" |");
  for (int a = 0; a < A; ++a) printf(" %d", member[a]);
  printf("\n");
}

static void run_fingerprint(FpWave* w) {                     // smiles_fp_kernel, atom by atom
  const int L = rd_in(0, 255);
  fresh(w, L);
  for (int i = 0; i < L; ++i) w->col[1][i] = rdu();
  for (int k = 0; k < kFpWords; ++k) w->bits[k] = 0;         // (the kernel clears them in front of the staging)
  int A, nb;
  bool unsup;
  const bool parsed = rand_parse(*w, 0, L, A, nb, unsup);
  const int status = !parsed ? GCT_FP_SYNTAX : unsup ? GCT_FP_UNSUPPORTED : GCT_FP_GRAPH;
  if (status == GCT_FP_GRAPH) {
    for (int e = 0; e < nb; ++e) w->blab[e] = (uint8_t)key_bond_label(*w, e);
    for (int a = 0; a < A; ++a) {
      const uint64_t id = fp_id0(*w, a);
      w->col[0][a] = id;
      fp_mark(*w, id);
    }
    memset((void*)w->col[1], 0xCD, sizeof(w->col[1]));       // every label is read: the first round overwrites them
    for (int r = 0; r < GCT_FP_RADIUS; ++r)
      for (int a = 0; a < A; ++a) {
        const uint64_t id = key_refine(*w, w->col[r & 1], a);
        w->col[(r + 1) & 1][a] = id;
        fp_mark(*w, id);
      }
  }
  printf("%d %d %d", status, A, nb);
  for (int k = 0; k < kFpWords; k += 2)
    printf(" %llu", (unsigned long long)((uint64_t)w->bits[k] | ((uint64_t)w->bits[k + 1] << 32)));
  printf("\n");
}

struct TaniCase {};                                          // (no record: the vectors below are the case's memory)

static void run_tanimoto(TaniCase*) {                        // tani_kernel's walk of one row of a, and tani_fold
  const int na = rd_in(0, 4096), nb = rd_in(0, 4096), p = rd_in(1, 2), tile = rd_in(1, 4096), tps = rd_in(1, 4096);
  std::vector<int32_t> ca((size_t)na), cb((size_t)nb);
  std::vector<uint32_t> wa((size_t)na * kFpWords), wb((size_t)nb * kFpWords);
  for (int i = 0; i < na; ++i) {
    ca[i] = rd_in(0, GCT_FP_BITS);
    for (int k = 0; k < kFpWords; ++k) wa[(size_t)i * kFpWords + k] = (uint32_t)rdu();
  }
  for (int j = 0; j < nb; ++j) {
    cb[j] = rd_in(0, GCT_FP_BITS);
    for (int k = 0; k < kFpWords; ++k) wb[(size_t)j * kFpWords + k] = (uint32_t)rdu();
  }
  const int tiles = (nb + tile - 1) / tile, splits = tiles ? (tiles + tps - 1) / tps : 1;
  std::vector<int32_t> pc((size_t)splits), pu((size_t)splits), pj((size_t)splits);
  std::vector<double> pt((size_t)splits);
  for (int i = 0; i < na; ++i) {
    for (int s = 0; s < splits; ++s) {
      TaniBest best = tani_none();
      double total = 0.0;
      const int first = s * tps * tile, end = std::min(nb, first + tps * tile);
      for (int jb = first; jb < end; jb += tile) {           // a tile as the kernel stages it: its own copy, exactly as long
        const int rows = std::min(tile, end - jb);
        std::vector<uint32_t> sb(wb.begin() + (size_t)jb * kFpWords, wb.begin() + (size_t)(jb + rows) * kFpWords);
        std::vector<int32_t> sc(cb.begin() + jb, cb.begin() + jb + rows);
        if (p == 2)
          tani_tile<2>(&wa[(size_t)i * kFpWords], ca[i], sb.data(), sc.data(), jb, jb, jb + rows, best, total);
        else
          tani_tile<1>(&wa[(size_t)i * kFpWords], ca[i], sb.data(), sc.data(), jb, jb, jb + rows, best, total);
      }
      pc[s] = best.c, pu[s] = best.u, pj[s] = best.j, pt[s] = total;
    }
    float best;
    int32_t arg;
    double total;
    tani_fold(pc.data(), pu.data(), pj.data(), pt.data(), 1, splits, ca[i], best, arg, total);
    uint32_t fb;
    uint64_t tb;
    memcpy(&fb, &best, 4), memcpy(&tb, &total, 8);
    printf("%u %d %llu ", fb, (int)arg, (unsigned long long)tb);
  }
  printf("\n");
}

static void run_descriptor(DescWave* w) {                    // smiles_desc_kernel, bond by bond and atom by atom
  const int L = rd_in(0, 255);
  fresh(w, L);
  for (int i = 0; i < L; ++i) w->dsc[i] = (uint16_t)rd_in(0, 0xFFFF);
  int A, nb;
  bool unsup;
  const bool parsed = rand_parse(*w, 0, L, A, nb, unsup);
  if (!parsed || unsup) {
    printf("%d %d 0 0 0 0 0 0 0 0 0 0\n", parsed ? GCT_DESC_UNSUPPORTED : GCT_DESC_SYNTAX, parsed ? A : 0);
    return;
  }
  int ring_bonds = 0, arom_bonds = 0, rot = 0;
  for (int e = 0; e < nb; ++e) {
    const int s = desc_ring_size(*w, e), c = desc_bond_class(*w, e, s);
    w->rsz[e] = (uint8_t)s, w->bcls[e] = (uint8_t)c;
    ring_bonds += s != 0, arom_bonds += s != 0 && c == kDescAromatic;
  }
  DescAtom t = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int comps = 0;
  for (int a = 0; a < A; ++a) {
    const DescAtom r = desc_atom(*w, a);
    w->aflag[a] = (uint8_t)r.triple;
    t.unknown += r.unknown, t.hydrogens += r.hydrogens, t.mass += r.mass, t.charge += r.charge, t.hbd += r.hbd;
    t.hba += r.hba, t.tpsa += r.tpsa, t.touched += r.touched;
    if (r.touched) comps += desc_component(*w, a) == a;
  }
  for (int e = 0; e < nb; ++e) rot += desc_rotatable(*w, e);
  if (t.unknown)
    printf("%d %d 0 0 0 0 0 0 0 0 0 0\n", GCT_DESC_UNKNOWN_ATOM, A);
  else
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", GCT_DESC_OK, A, t.hydrogens, t.mass, t.charge, t.hbd, t.hba, rot,
           nb - A + 1, arom_bonds - t.touched + comps, t.tpsa, ring_bonds);
}

template <class Rec>
static int run(void (*one)(Rec*)) {
  std::vector<Rec> record(1);                                // on the heap, where ASan guards both ends
  for (long long n = rd(); n > 0; --n) one(record.data());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3 || !(f = fopen(argv[2], "r"))) return 2;
  const char* mode = argv[1];
  if (!strcmp(mode, "check")) return run(run_check);
  if (!strcmp(mode, "randomize")) return run(run_randomize);
  if (!strcmp(mode, "key")) return run(run_key);
  if (!strcmp(mode, "scaffold")) return run(run_scaffold);
  if (!strcmp(mode, "fingerprint")) return run(run_fingerprint);
  if (!strcmp(mode, "tanimoto")) return run(run_tanimoto);
  if (!strcmp(mode, "descriptor")) return run(run_descriptor);
  return 2;
}
