// Stand-alone driver for a sanitizer run of mvae_smiles_substruct_compile_host and mvae_smiles_substruct_host (host code only; nothing
// here touches a device).
//   python tests/sanitize/rewrite_host_dump.py rows.bin
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude tests/sanitize/substruct_host_main.cpp molecular-vae_amd/csrc/smiles_substruct.hip -o substruct_host_asan
//   ./substruct_host_asan rows.bin
// rows.bin is the rewrite driver's file (its seed and draws are not used): int32 B, T, V, bos, eos, pad, seed, reps; int64 x [B, T];
// int32 tok_info [V], chem_info [V], emit [48]; uint32 draw [B].
// The queries are the file's own rows: every slice of 64 rows goes through the compile entry (most are refused: too many atoms, stereo,
// the corpus' broken rows), and every eighth slice is searched for in the first 700 rows at three budgets, with and without map, steps
// and counts.  One more search runs with a table of random words, which the entry has to survive: it masks every index.
// Every buffer is allocated at its exact size, so a read or write one element past any of them is reported.
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
  const int B = h[0], T = h[1], V = h[2], eos = h[4];
  const std::vector<int64_t> x = take<int64_t>(f, (size_t)B * T);
  const std::vector<int32_t> tok = take<int32_t>(f, V), chem = take<int32_t>(f, V), emit = take<int32_t>(f, MVAE_REWRITE_EMIT);
  fclose(f);
  const uint32_t stereo_lo = (uint32_t)emit[43], stereo_hi = (uint32_t)emit[44];
  unsigned long long sum = 0;
  long accepted = 0, refused[16] = {0}, searched = 0;
  const int rows = B < 700 ? B : 700;
  for (int q0 = 0, slice = 0; q0 < B; q0 += MVAE_SUBSTRUCT_QUERIES, ++slice) {
    const int Q = B - q0 < MVAE_SUBSTRUCT_QUERIES ? B - q0 : MVAE_SUBSTRUCT_QUERIES;
    std::vector<int32_t> table((size_t)Q * MVAE_SUBSTRUCT_WORDS), qstatus(Q);
    int rc = mvae_smiles_substruct_compile_host(Q, T, V, x.data() + (size_t)q0 * T, T, tok.data(), chem.data(), stereo_lo, stereo_hi, eos,
                                                table.data(), qstatus.data());
    if (rc != MVAE_OK) { fprintf(stderr, "compile returned %d\n", rc); return 1; }
    int ok = 0;
    for (int q = 0; q < Q; ++q) { ok += qstatus[q] == 0; ++refused[qstatus[q] & 15]; }
    accepted += ok;
    for (int32_t v : table) sum += (unsigned long long)(uint32_t)v;
    if (slice % 8) continue;
    const int budgets[3] = {65536, 300, 1};
    for (int pass = 0; pass < 3; ++pass) {
      const bool bare = pass == 2;
      std::vector<int32_t> status(rows), steps((size_t)rows * Q), counts((size_t)Q * 2);
      std::vector<int64_t> hit(rows), undecided(rows);
      std::vector<uint8_t> map((size_t)rows * MVAE_SUBSTRUCT_QATOMS);
      rc = mvae_smiles_substruct_host(rows, T, V, x.data(), T, tok.data(), chem.data(), eos, Q, table.data(), budgets[pass], Q - 1, status.data(),
                                      hit.data(), undecided.data(), bare ? nullptr : map.data(), bare ? nullptr : steps.data(),
                                      bare ? nullptr : counts.data());
      if (rc != MVAE_OK) { fprintf(stderr, "search returned %d\n", rc); return 1; }
      ++searched;
      for (int b = 0; b < rows; ++b) sum += (unsigned long long)status[b] + (unsigned long long)hit[b] + 3ull * (unsigned long long)undecided[b];
      if (!bare) {
        for (int32_t v : steps) sum += (unsigned long long)v;
        for (int32_t v : counts) sum += (unsigned long long)v;
        for (uint8_t v : map) sum += v;
      }
    }
  }
  // a table the compile entry did not write
  {
    const int Q = 16;
    std::vector<int32_t> table((size_t)Q * MVAE_SUBSTRUCT_WORDS), status(rows), steps((size_t)rows * Q);
    uint32_t s = 12345;
    for (int32_t& v : table) { s = s * 1664525u + 1013904223u; v = (int32_t)s; }
    for (int q = 0; q < Q; ++q) {
      table[(size_t)q * MVAE_SUBSTRUCT_WORDS] = q * 3 - 2;             // -2 .. 43 atoms
      for (int k = 1; k <= 3; ++k) table[(size_t)q * MVAE_SUBSTRUCT_WORDS + k] = 0;
    }
    std::vector<int64_t> hit(rows), undecided(rows);
    std::vector<uint8_t> map((size_t)rows * MVAE_SUBSTRUCT_QATOMS);
    const int rc = mvae_smiles_substruct_host(rows, T, V, x.data(), T, tok.data(), chem.data(), eos, Q, table.data(), 2000, 7, status.data(),
                                              hit.data(), undecided.data(), map.data(), steps.data(), nullptr);
    if (rc != MVAE_OK) { fprintf(stderr, "search returned %d\n", rc); return 1; }
    for (int32_t v : steps) sum += (unsigned long long)v;
  }
  printf("rows %d, queries accepted %ld, searches %ld, checksum %llu, query statuses:", B, accepted, searched, sum);
  for (int s = 0; s < 16; ++s) printf(" %ld", refused[s]);
  printf("\n");
  return 0;
}
