// CPU harness of gct_smiles_scaffold's host-callable parts (tools/scaffold_walk_check.py builds and drives it): rand_parse
// of csrc/smiles_graph.h, sca_peel / sca_shell / sca_nh / sca_compact of csrc/scaffold.hip, the per-atom key functions of
// csrc/smiles_key.h and rand_walk of csrc/smiles_walk.h run on the HOST over one ScaWave record per case, bond by bond and
// atom by atom as the kernel's lanes do, so that AddressSanitizer and UBSan see every index they form -- the aliased walk
// buffers and the reused parse fields included.  No GPU is touched.  Cases come from a text file -- the count, then per case
//   L n_rings open_id close_id room nh_id nh_word / nh_label / L table words (| 1 << 25 on `n`) / L token labels /
//   n_rings ring ids
// -- and one line goes out per case: status, key (unsigned), atoms kept, length | the row's entries (a literal id, or
// -(j + 1) for the token at position j) | member per input atom.
#include "../gct_plus_amd/csrc/scaffold.hip"

#include <cstdio>
#include <vector>

void gct_set_error(const char*, ...) {}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  long long ncases = 0, x = 0;
  unsigned long long u = 0;
  if (!f || fscanf(f, "%lld", &ncases) != 1) return 2;
  std::vector<ScaWave> record(1);
  ScaWave* w = record.data();
  for (long long cs = 0; cs < ncases; ++cs) {
    long long head[7];
    for (long long& h : head)
      if (fscanf(f, "%lld", &h) != 1) return 2;
    const int L = (int)head[0], nr = (int)head[1], open_id = (int)head[2], close_id = (int)head[3], room = (int)head[4];
    const int nh_id = (int)head[5], nh_word = (int)head[6];
    if (L < 0 || L > 255 || nr < 0 || nr > 63 || room < 0 || room > 255) return 2;
    if (fscanf(f, "%llu", &u) != 1) return 2;
    const uint64_t nh_label = (uint64_t)u;
    std::vector<int32_t> rid(64, -1);
    for (size_t q = 0; q < sizeof(*w); ++q) ((unsigned char*)w)[q] = 0xAB;   // nothing may rely on a cleared record
    for (int i = 0; i < L; ++i) {
      if (fscanf(f, "%lld", &x) != 1) return 2;
      w->e[i] = (int32_t)x;
    }
    for (int i = 0; i < L; ++i) {
      if (fscanf(f, "%llu", &u) != 1) return 2;
      w->lab[i] = (uint64_t)u;
    }
    for (int i = 0; i < nr; ++i) {
      if (fscanf(f, "%lld", &x) != 1) return 2;
      rid[i] = (int32_t)x;
    }
    int A, nb;
    bool unsup;
    const bool parsed = rand_parse(*w, 0, L, A, nb, unsup);
    if (!parsed || unsup) {
      printf("%d 0 0 0 | |\n", parsed ? GCT_SCA_UNSUPPORTED : GCT_SCA_SYNTAX);
      continue;
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
        for (int e = 0; e < nBk; ++e) w->blab[e] = (uint8_t)key_bond_label(*w, e);
        for (int a = 0; a < nK; ++a) w->col[0][a] = key_profile(*w, a);
        for (int r = 0; r < GCT_KEY_ROUNDS; ++r)
          for (int a = 0; a < nK; ++a) w->col[(r + 1) & 1][a] = key_refine(*w, w->col[r & 1], a);
        uint64_t sum = 0;
        for (int a = 0; a < nK; ++a) sum += key_mix(w->col[GCT_KEY_ROUNDS & 1][a]);
        key = key_combine(sum, nK, nBk);
        for (size_t q = 0; q < sizeof(w->col); ++q) ((unsigned char*)w->col)[q] = 0xCD;   // the walk's buffers alias it
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
  fclose(f);
  return 0;
}
