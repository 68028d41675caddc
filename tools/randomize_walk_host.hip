// CPU harness of gct_smiles_randomize's sequential walks (tools/randomize_walk_check.py builds and drives it): rand_parse,
// the list shuffle as the kernel's lanes do it, and rand_walk of csrc/randomize.hip run on the HOST over one RandWave
// record per case, so that AddressSanitizer and UBSan see every index the walks form.  No GPU is touched.  Cases come
// from a text file -- the count, then per case
//   L calls n_rings open_id close_id room / L table words / 4 * calls stream words / n_rings ring ids
// -- and one line goes out per case: the status, and for a rewritten part the row's LDS entries and perm.
#include "../gct_plus_amd/csrc/randomize.hip"

#include <cstdio>
#include <vector>

void gct_set_error(const char*, ...) {}

static bool read_int(FILE* f, long long& x) { return fscanf(f, "%lld", &x) == 1; }

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
  long long ncases = 0, x = 0;
  if (!f || !read_int(f, ncases)) return 2;
  std::vector<RandWave> record(1);
  RandWave* w = record.data();
  for (long long cs = 0; cs < ncases; ++cs) {
    long long head[6];
    for (long long& h : head)
      if (!read_int(f, h)) return 2;
    const int L = (int)head[0], calls = (int)head[1], nr = (int)head[2], open_id = (int)head[3], close_id = (int)head[4];
    const int room = (int)head[5];
    if (L < 0 || L > 255 || calls < 1 + 2 * L || nr < 0 || nr > 63 || room < 0 || room > 256) return 2;
    std::vector<uint32_t> words(4 * (size_t)calls);
    std::vector<int32_t> rid(64, -1);
    for (size_t q = 0; q < sizeof(*w); ++q) ((unsigned char*)w)[q] = 0xAB;   // nothing may rely on a cleared record
    for (int i = 0; i < L; ++i) {
      if (!read_int(f, x)) return 2;
      w->e[i] = (int32_t)x;
    }
    for (uint32_t& word : words) {
      if (!read_int(f, x)) return 2;
      word = (uint32_t)x;
    }
    for (int i = 0; i < nr; ++i) {
      if (!read_int(f, x)) return 2;
      rid[i] = (int32_t)x;
    }
    int A, nb;
    bool unsup;
    if (!rand_parse(*w, 0, L, A, nb, unsup)) {
      printf("%d\n", GCT_RAND_SYNTAX);
      continue;
    }
    if (unsup) {
      printf("%d\n", GCT_RAND_UNSUPPORTED);
      continue;
    }
    for (int e = 0; e < nb; ++e) w->role[e] = 0;                              // the lanes' part, atom by atom
    for (int a = 0; a < A; ++a) {
      w->seen[a] = 0, w->left[a] = 0;
      const int d = w->deg[a];
      for (int i = d - 1; i >= 1; --i) {
        const uint32_t word = words[4 * (size_t)(1 + 2 * a + (i - 1) / 4) + (i - 1) % 4];
        const int j = (int)(((uint64_t)word * (uint32_t)(i + 1)) >> 32);
        const uint8_t ti = w->adj[a][i], tj = w->adj[a][j];
        w->adj[a][i] = tj, w->adj[a][j] = ti;
      }
    }
    const int root = (int)(((uint64_t)words[1] * (uint32_t)A) >> 32);
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
  fclose(f);
  return 0;
}
