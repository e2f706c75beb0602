// Stand-alone driver for a sanitizer run of mvae_smiles_scaffold_smiles_host (host code only; nothing here touches a device).
//   python tests/sanitize/rewrite_host_dump.py rows.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude tests/sanitize/scaffold_smiles_host_main.cpp molecular-vae_amd/csrc/scaffold_smiles.hip \
//         -o scaffold_smiles_host_asan
//   ./scaffold_smiles_host_asan rows.bin
// rows.bin is the rewrite driver's file (its seed and draws are not used): int32 B, T, V, bos, eos, pad, seed, reps; int64 x [B, T];
// int32 tok_info [V], chem_info [V], emit [48]; uint32 draw [B].
// Every buffer is allocated at its exact size, so a read or write one element past any of them is reported.  The run repeats with
// max_content = 127, 20 and 1, with T_out = max_content + 2 and T_out = 2, and without info.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mvae.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short file\n"); exit(2); }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s rows.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const std::vector<int32_t> h = take<int32_t>(f, 8);
  const int B = h[0], T = h[1], V = h[2], bos = h[3], eos = h[4], pad = h[5];
  const std::vector<int64_t> x = take<int64_t>(f, (size_t)B * T);
  const std::vector<int32_t> tok = take<int32_t>(f, V), chem = take<int32_t>(f, V), emit = take<int32_t>(f, MVAE_REWRITE_EMIT);
  fclose(f);
  long hist[16] = {0};
  unsigned long long sum = 0;
  const int mcs[3] = {127, 20, 1};
  for (int mc : mcs)
    for (int pass = 0; pass < 3; ++pass) {
      const int T_out = pass == 1 ? 2 : mc + 2;
      std::vector<int64_t> out((size_t)B * T_out);
      std::vector<int32_t> out_len(B), status(B), info((size_t)B * MVAE_SCAFFOLD_SMILES_INFO);
      const int rc = mvae_smiles_scaffold_smiles_host(B, T, V, x.data(), T, tok.data(), chem.data(), emit.data(), bos, eos, pad, mc, T_out,
                                                      out.data(), out_len.data(), status.data(), pass == 2 ? nullptr : info.data());
      if (rc != MVAE_OK) { fprintf(stderr, "entry returned %d\n", rc); return 1; }
      for (int b = 0; b < B; ++b) { ++hist[status[b] & 15]; sum += (unsigned long long)out_len[b]; }
      for (int64_t v : out) sum += (unsigned long long)v;
      if (pass != 2)
        for (int32_t v : info) sum += (unsigned long long)v;
    }
  printf("rows %d x 9 runs, checksum %llu, statuses:", B, sum);
  for (int s = 0; s < 16; ++s) printf(" %ld", hist[s]);
  printf("\n");
  return 0;
}
