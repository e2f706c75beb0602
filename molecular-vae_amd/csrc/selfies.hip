// SELFIES on the device (gfx950): mvae_selfies_decode_rows / _corpus / _host and mvae_selfies_encode_rows / _corpus / _host.
// include/mvae.h ("SELFIES") states the definition; NOT the selfies package's derivation, agreement with it is neither tested nor claimed.
//
// Two more families of the writer driver (smiles_writer.hpp).  The driver's block bodies (block_rows, block_corpus) and its host loop
// (host_rows) are used as they are: to them V, tok_info, chem_info and emit are whatever the family's row() reads, and bos_id, eos_id,
// pad_id are the output's.  What the driver cannot state for a family whose input and output vocabularies differ are the argument checks
// of its entries (it wants eos_id < V and both SMILES tables), so the checks and the three launches stand here, and nothing else does.
//   decode   sf::derive            the derivation into the walk's arrays: atom words, deferred ring bonds (selfies.hpp)
//            sf::apply_rings       the ring bonds in order, clamped by what both ends can still take; a second bond raises the first
//            sf::reparent          a ring bond of order >= 2 becomes a tree bond, the single tree bond it displaces the closure
//            rew::adjacency, can::ranks, rew::write(can::RankOrder)      unchanged: the canonical Kekule spelling in the SMILES vocabulary
//   encode   rew::read             the walk and the stereo test
//            sf::kekulise          the matching of kekule.hpp on lent arrays, made explicit as double bonds
//            sf::sizes             the capacity test, the last child and the subtree size of every atom
//            sf::emit_row          the symbols in atom order, staged in the half-edge array and moved to O when C is dead
// One thread per row, 64-thread blocks, the rewrite's 80 KiB of LDS per block (rew::Lds) with nothing added.  A row that is not written
// gives the empty row, never a copy of its source, which is in another language.
#include "common.hpp"
#include "selfies.hpp"
#include "smiles_canon.hpp"
#include "smiles_writer.hpp"

namespace sf {

struct Info {
  int32_t* info;
  SMI_HD void put(long b, int a, int c, int d, int e) const {
    if (!info) return;
    info[4 * b] = a; info[4 * b + 1] = c; info[4 * b + 2] = d; info[4 * b + 3] = e;
  }
};

// SELFIES tokens in, SMILES tokens out.  To the driver: V and tok_info are the SELFIES vocabulary's size and info table, chem_info is
// unused, emit is the SMILES emit table.  info = atoms, ring bonds, ring bonds re-parented, the column of a token that is no symbol.
struct Decode {
  struct Args { int32_t* info; };

  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool, int V, const int32_t* sinfo, const int32_t*, const int32_t* emit, int,
                        int max_content, long b, const Args& a, int* len) {
    *len = 0;
    const Info info{a.info};
    const Derived d = derive(s.W, s.C, s.S, s.D, s.P, src, first, end, V, sinfo);
    if (d.status != smg::OK) { info.put(b, 0, 0, 0, d.col); return d.status; }
    const int kept = apply_rings(s.W, s.C, d.nring);
    const int moved = reparent(s.W, s.C, kept);
    info.put(b, d.n, kept, moved < 0 ? 0 : moved, -1);
    if (moved < 0) return rew::RING_MULTI;
    finish_words(s.W, d.n);
    rew::adjacency(s.W, s.C, s.A, s.S, s.D, s.P, d.n, kept);
    int unused[4];
    can::ranks(s.W, s.A, s.S, s.O, s.D, s.P, d.n, unused);
    const int st = rew::write(can::RankOrder<decltype(s.O)>{s.O}, s.W, s.O, s.A, s.S, s.D, s.P, d.n, emit, max_content, len);
    if (st != smg::OK) *len = 0;
    return st;
  }

  static SMI_HD void skipped(long b, const Args& a) { Info{a.info}.put(b, 0, 0, 0, -1); }
};

// SMILES tokens in, SELFIES tokens out.  To the driver: V, tok_info, chem_info and emit are the SMILES vocabulary's.  semit: the SELFIES
// emit table; eos_in: the <eos> of the SMILES rows.  info = atoms, branch symbols, ring symbols, the atom over its capacity.
struct Encode {
  struct Args {
    const int32_t* semit;
    int eos_in;
    int32_t* info;
  };

  template <class S, class Src>
  static SMI_HD int row(S& s, const Src& src, int first, int end, bool end_is_eos, int V, const int32_t* tok_info, const int32_t* chem_info,
                        const int32_t* emit, int, int max_content, long b, const Args& a, int* len) {
    *len = 0;
    const Info info{a.info};
    info.put(b, 0, 0, 0, -1);
    fpr::Rec<decltype(s.C)> rec(s.C);
    const int st = rew::read(s.W, rec, src, first, end, end_is_eos, V, tok_info, chem_info, emit, end_is_eos ? -1 : a.eos_in);
    if (st != smg::OK) return st;
    const int n = rec.n, nclos = rec.nclos < fpr::CLOSURES ? rec.nclos : fpr::CLOSURES;
    if (!kekulise(s.W, s.C, s.A, s.S, s.D, n, nclos)) return kek::KEKULE;
    const int over = sizes(s.W, s.C, s.S, s.D, s.P, n, nclos);
    if (over != NONE) { info.put(b, n, 0, 0, over); return CAPACITY; }
    HalfView<decltype(s.A), 0> stage{s.A};
    rew::Writer<decltype(stage)> out{stage, a.semit, max_content};
    int branches, rings;
    const int wst = emit_row(s.W, s.C, s.S, s.D, s.P, n, nclos, out, &branches, &rings);
    info.put(b, n, branches, rings, -1);
    if (wst != smg::OK) return wst;
    for (int t = 0; t < out.len; ++t) s.O.set(t, (uint8_t)stage.get(t));
    *len = out.len;
    return smg::OK;
  }

  static SMI_HD void skipped(long b, const Args& a) { Info{a.info}.put(b, 0, 0, 0, -1); }
};

inline bool id_ok(int id) { return id >= 0 && id <= 255; }

// what every entry refuses: the output ids are bytes of the staged row
inline int common_check(int V, const void* table_a, const void* table_b, const void* table_c, int max_content, const void* status) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;
  if (V < 1 || !table_a || !table_b || !table_c || !status || max_content < 1 || max_content > smg::CONTENT_MAX) return MVAE_ERR_INVALID;
  return MVAE_OK;
}
inline int rows_check(int B, int T, const int64_t* x, int64_t x_ld, int bos_id, int eos_id, int pad_id, int T_out, const void* out,
                      const void* out_len) {
  return x && out && out_len && B >= 1 && T >= 1 && x_ld >= T && id_ok(bos_id) && id_ok(eos_id) && id_ok(pad_id) && T_out >= 2 ? MVAE_OK
                                                                                                                                : MVAE_ERR_INVALID;
}
inline int corpus_check(const void* tokens, const void* offsets, int64_t N, const void* rows, int B, int max_content, int stride,
                        const void* tokens_out, const void* offsets_out) {
  return tokens && offsets && rows && tokens_out && offsets_out && N >= 1 && B >= 1 && stride >= max_content ? MVAE_OK : MVAE_ERR_INVALID;
}

}  // namespace sf

namespace {

static_assert(sizeof(rew::Lds) == MVAE_SELFIES_LDS_BYTES, "include/mvae.h states the LDS per block");
static_assert(MVAE_SELFIES_LDS_BYTES <= 80 * 1024, "two blocks per CU");

__global__ __launch_bounds__(64) void selfies_decode_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                 const int32_t* __restrict__ sinfo, const int32_t* __restrict__ emit, int bos_id,
                                                                 int eos_id, int pad_id, int max_content, int T_out, int64_t* __restrict__ out,
                                                                 int32_t* __restrict__ out_len, int32_t* __restrict__ status,
                                                                 int32_t* __restrict__ counts, int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_rows<sf::Decode>(lds, B, T, V, x, x_ld, sinfo, nullptr, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                              counts, info);
}

__global__ __launch_bounds__(64) void selfies_decode_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                   const int64_t* __restrict__ rows, int B, int V,
                                                                   const int32_t* __restrict__ sinfo, const int32_t* __restrict__ emit,
                                                                   int max_content, int stride, uint8_t* __restrict__ tokens_out,
                                                                   int64_t* __restrict__ offsets_out, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ err,
                                                                   int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_corpus<sf::Decode>(lds, tokens, offsets, N, rows, B, V, sinfo, nullptr, emit, max_content, stride, tokens_out, offsets_out, status,
                                counts, err, info);
}

__global__ __launch_bounds__(64) void selfies_encode_rows_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                 const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                 const int32_t* __restrict__ emit, int eos_in, const int32_t* __restrict__ semit,
                                                                 int bos_id, int eos_id, int pad_id, int max_content, int T_out,
                                                                 int64_t* __restrict__ out, int32_t* __restrict__ out_len,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_rows<sf::Encode>(lds, B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                              counts, semit, eos_in, info);
}

__global__ __launch_bounds__(64) void selfies_encode_corpus_kernel(const uint8_t* __restrict__ tokens, const int64_t* __restrict__ offsets, long N,
                                                                   const int64_t* __restrict__ rows, int B, int V,
                                                                   const int32_t* __restrict__ tok_info, const int32_t* __restrict__ chem_info,
                                                                   const int32_t* __restrict__ emit, const int32_t* __restrict__ semit,
                                                                   int max_content, int stride, uint8_t* __restrict__ tokens_out,
                                                                   int64_t* __restrict__ offsets_out, int32_t* __restrict__ status,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ err,
                                                                   int32_t* __restrict__ info) {
  __shared__ rew::Lds lds;
  rew::block_corpus<sf::Encode>(lds, tokens, offsets, N, rows, B, V, tok_info, chem_info, emit, max_content, stride, tokens_out, offsets_out,
                                status, counts, err, semit, -1, info);
}

}  // namespace

extern "C" {

int mvae_selfies_decode_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* sinfo, const int32_t* emit, int bos_id,
                             int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len, int32_t* status,
                             int32_t* counts, int32_t* info, void* stream) {
  if (const int rc = sf::common_check(V, sinfo, emit, emit, max_content, status)) return rc;
  if (const int rc = sf::rows_check(B, T, x, x_ld, bos_id, eos_id, pad_id, T_out, out, out_len)) return rc;
  hipLaunchKernelGGL(selfies_decode_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, sinfo, emit,
                     bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status, counts, info);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_selfies_decode_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V, const int32_t* sinfo,
                               const int32_t* emit, int max_content, int stride, uint8_t* tokens_out, int64_t* offsets_out, int32_t* status,
                               int32_t* counts, int32_t* err, int32_t* info, void* stream) {
  if (const int rc = sf::common_check(V, sinfo, emit, emit, max_content, status)) return rc;
  if (const int rc = sf::corpus_check(tokens, offsets, N, rows, B, max_content, stride, tokens_out, offsets_out)) return rc;
  hipLaunchKernelGGL(selfies_decode_corpus_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, rows, B, V,
                     sinfo, emit, max_content, stride, tokens_out, offsets_out, status, counts, err, info);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_selfies_decode_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* sinfo, const int32_t* emit, int bos_id,
                             int eos_id, int pad_id, int max_content, int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* info) {
  if (const int rc = sf::common_check(V, sinfo, emit, emit, max_content, status)) return rc;
  if (const int rc = sf::rows_check(B, T, x, x_ld, bos_id, eos_id, pad_id, T_out, out, out_len)) return rc;
  return rew::host_rows<sf::Decode>(B, T, V, x, x_ld, sinfo, nullptr, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status,
                                    info);
}

int mvae_selfies_encode_rows(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int eos_in, const int32_t* semit, int bos_id, int eos_id, int pad_id, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* counts, int32_t* info, void* stream) {
  if (const int rc = sf::common_check(V, tok_info, chem_info, emit, max_content, status)) return rc;
  if (const int rc = sf::rows_check(B, T, x, x_ld, bos_id, eos_id, pad_id, T_out, out, out_len)) return rc;
  if (!semit || eos_in < 0 || eos_in >= V) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(selfies_encode_rows_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info,
                     chem_info, emit, eos_in, semit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len, status, counts, info);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_selfies_encode_corpus(const uint8_t* tokens, const int64_t* offsets, int64_t N, const int64_t* rows, int B, int V,
                               const int32_t* tok_info, const int32_t* chem_info, const int32_t* emit, const int32_t* semit, int max_content,
                               int stride, uint8_t* tokens_out, int64_t* offsets_out, int32_t* status, int32_t* counts, int32_t* err,
                               int32_t* info, void* stream) {
  if (const int rc = sf::common_check(V, tok_info, chem_info, emit, max_content, status)) return rc;
  if (const int rc = sf::corpus_check(tokens, offsets, N, rows, B, max_content, stride, tokens_out, offsets_out)) return rc;
  if (!semit) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(selfies_encode_corpus_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, tokens, offsets, (long)N, rows, B, V,
                     tok_info, chem_info, emit, semit, max_content, stride, tokens_out, offsets_out, status, counts, err, info);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_selfies_encode_host(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, const int32_t* chem_info,
                             const int32_t* emit, int eos_in, const int32_t* semit, int bos_id, int eos_id, int pad_id, int max_content,
                             int T_out, int64_t* out, int32_t* out_len, int32_t* status, int32_t* info) {
  if (const int rc = sf::common_check(V, tok_info, chem_info, emit, max_content, status)) return rc;
  if (const int rc = sf::rows_check(B, T, x, x_ld, bos_id, eos_id, pad_id, T_out, out, out_len)) return rc;
  if (!semit || eos_in < 0 || eos_in >= V) return MVAE_ERR_INVALID;
  return rew::host_rows<sf::Encode>(B, T, V, x, x_ld, tok_info, chem_info, emit, bos_id, eos_id, pad_id, max_content, T_out, out, out_len,
                                    status, semit, eos_in, info);
}

}  // extern "C"
