// CPU harness of gct_smiles_key's host-callable parts (tools/molkey_walk_check.py builds and drives it): rand_parse of
// csrc/smiles_graph.h and key_bond_label / key_profile / key_refine / key_combine / key_string of csrc/molkey.hip run on
// the HOST over one KeyWave record per case, atom by atom as the kernel's lanes do, so that AddressSanitizer and UBSan
// see every index they form.  No GPU is touched.  Cases come from a text file -- the count, then per case
//   L / L table words / L token labels (unsigned 64-bit)
// -- and one line goes out per case: status, key (unsigned), atoms, bonds.
#include "../gct_plus_amd/csrc/molkey.hip"

#include <cstdio>
#include <vector>

void gct_set_error(const char*, ...) {}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  long long ncases = 0, x = 0;
  unsigned long long u = 0;
  if (!f || fscanf(f, "%lld", &ncases) != 1) return 2;
  std::vector<KeyWave> record(1);
  KeyWave* w = record.data();
  for (long long cs = 0; cs < ncases; ++cs) {
    long long L = 0;
    if (fscanf(f, "%lld", &L) != 1 || L < 0 || L > 255) return 2;
    for (size_t q = 0; q < sizeof(*w); ++q) ((unsigned char*)w)[q] = 0xAB;   // nothing may rely on a cleared record
    for (int i = 0; i < (int)L; ++i) {
      if (fscanf(f, "%lld", &x) != 1) return 2;
      w->e[i] = (int32_t)x & 0xFFFFFF;
    }
    for (int i = 0; i < (int)L; ++i) {
      if (fscanf(f, "%llu", &u) != 1) return 2;
      w->lab[i] = (uint64_t)u;
    }
    int A, nb;
    bool unsup;
    const bool parsed = rand_parse(*w, 0, (int)L, A, nb, unsup);
    if (!parsed || unsup) {
      printf("%d %llu %d %d\n", parsed ? GCT_KEY_STRING_UNSUPPORTED : GCT_KEY_STRING_SYNTAX,
             (unsigned long long)key_string(*w, 0, (int)L), A, nb);
      continue;
    }
    for (int e = 0; e < nb; ++e) w->blab[e] = (uint8_t)key_bond_label(*w, e);
    for (int a = 0; a < A; ++a) w->col[0][a] = key_profile(*w, a);
    for (int r = 0; r < GCT_KEY_ROUNDS; ++r)
      for (int a = 0; a < A; ++a) w->col[(r + 1) & 1][a] = key_refine(*w, w->col[r & 1], a);
    uint64_t sum = 0;
    for (int a = 0; a < A; ++a) sum += key_mix(w->col[GCT_KEY_ROUNDS & 1][a]);
    printf("%d %llu %d %d\n", GCT_KEY_GRAPH, (unsigned long long)key_combine(sum, A, nb), A, nb);
  }
  fclose(f);
  return 0;
}
