// Stand-alone driver for a sanitizer run of mvae_smiles_fragment_host and mvae_smiles_fragment_smiles_host (host code only; nothing
// here touches a device).
//   python tests/sanitize/rewrite_host_dump.py rows.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude tests/sanitize/fragment_host_main.cpp molecular-vae_amd/csrc/fragment.hip molecular-vae_amd/csrc/fragment_smiles.hip \
//         -o fragment_host_asan
//   ./fragment_host_asan rows.bin
// rows.bin is the rewrite driver's file (its seed and draws are not used): int32 B, T, V, bos, eos, pad, seed, reps; int64 x [B, T];
// int32 tok_info [V], chem_info [V], emit [48]; uint32 draw [B].
// Every buffer is allocated at its exact size, so a read or write one element past any of them is reported.  The keys entry runs with
// and without the mask; the string entry runs for frag = 0, 1, 2, 15, 16 and 126, with max_content = 127 and 3, with T_out =
// max_content + 2 and T_out = 2, and without info.
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
  long hist[MVAE_FRAGMENT_SMILES_COUNTS] = {0};
  unsigned long long sum = 0;
  int runs = 0;
  for (int pass = 0; pass < 2; ++pass, ++runs) {
    std::vector<int32_t> status(B), desc((size_t)B * MVAE_FRAGMENT_DESC);
    std::vector<int64_t> mask((size_t)B * MVAE_FRAGMENT_MAX * 2), key((size_t)B * MVAE_FRAGMENT_MAX);
    const int rc = mvae_smiles_fragment_host(B, T, V, x.data(), T, tok.data(), chem.data(), eos, status.data(), pass ? nullptr : mask.data(),
                                             desc.data(), key.data());
    if (rc != MVAE_OK) { fprintf(stderr, "keys entry returned %d\n", rc); return 1; }
    for (int b = 0; b < B; ++b) ++hist[status[b] & 31];
    for (int32_t v : desc) sum += (unsigned long long)v;
    for (int64_t v : key) sum += (unsigned long long)v;
    if (!pass)
      for (int64_t v : mask) sum += (unsigned long long)v;
  }
  const int frags[6] = {0, 1, 2, 15, 16, 126}, mcs[2] = {127, 3};
  for (int frag : frags)
    for (int mc : mcs)
      for (int pass = 0; pass < 3; ++pass, ++runs) {
        const int T_out = pass == 1 ? 2 : mc + 2;
        std::vector<int64_t> out((size_t)B * T_out);
        std::vector<int32_t> out_len(B), status(B), info((size_t)B * MVAE_FRAGMENT_SMILES_INFO);
        const int rc = mvae_smiles_fragment_smiles_host(B, T, V, x.data(), T, tok.data(), chem.data(), emit.data(), bos, eos, pad, mc, T_out,
                                                        out.data(), out_len.data(), status.data(), frag, pass == 2 ? nullptr : info.data());
        if (rc != MVAE_OK) { fprintf(stderr, "string entry returned %d\n", rc); return 1; }
        for (int b = 0; b < B; ++b) { ++hist[status[b] & 31]; sum += (unsigned long long)out_len[b]; }
        for (int64_t v : out) sum += (unsigned long long)v;
        if (pass != 2)
          for (int32_t v : info) sum += (unsigned long long)v;
      }
  printf("rows %d x %d runs, checksum %llu, statuses:", B, runs, sum);
  for (int s = 0; s < 17; ++s) printf(" %ld", hist[s]);
  printf("\n");
  return 0;
}
