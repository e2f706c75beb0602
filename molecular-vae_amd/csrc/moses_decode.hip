// Autoregressive decoding back end of mosesvae.VAE (gfx950): the sampling step and its filtered / syntax-constrained / prefix-forced
// siblings, the beam-search step and its finalize, and the two SMILES-automaton kernels.  Every launch handles everything behind the GRU
// step of one generated token.  The pieces the kernels share (head staging and GEMV, wave scan, next-input row, automaton advance, token
// commit) are written once below: the suite requires the siblings to be bit-identical where their inputs coincide.
#include <atomic>
#include "common.hpp"
#include "kernels.hpp"
#include "smiles_syntax.hpp"

// ------------------------------------------------------------------------------------------- shared pieces
// the V x H head (decoder_fc) into LDS, once per workgroup
template <typename T>
__device__ __forceinline__ void stage_head(T* ws, const T* __restrict__ wfc, long ldw, int V, int H) {
  for (int i = threadIdx.x; i < V * H; i += 256) ws[i] = wfc[(long)(i / H) * ldw + (i % H)];
  __syncthreads();
}

// logit of one row: lane k-strided partial dot products, wave reduction per class (V <= 64 classes: class v ends up in lane v, lanes >= V
// hold -inf).  `scale` is the samplers' 1 / temp, applied where the value is selected -- (a + bias) * scale, rounded on its own: applied to
// the returned value it would be contracted with the subtraction of the max into one fma -- and 1 for the beam kernel (folded away).
template <typename T>
__device__ __forceinline__ float head_logit(const T* __restrict__ hrow, const T* ws, const float* __restrict__ bias, float scale, int V, int H,
                                            int lane) {
  float mine = -INFINITY;
  for (int v = 0; v < V; ++v) {
    float a = 0.f;
    for (int k = lane; k < H; k += 64) a += TT<T>::ld(hrow + k) * TT<T>::ld(ws + (long)v * H + k);
    a = wave_sum(a);
    if (lane == v) mine = (a + (bias ? bias[v] : 0.f)) * scale;
  }
  return mine;
}

// inclusive prefix sum over the 64 lanes (fixed order); *tot = the sum of all of them
__device__ __forceinline__ float wave_scan(float c, int lane, float* tot) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float up = __shfl_up(c, o, 64); if (lane >= o) c += up; }
  *tot = __shfl(c, 63, 64);
  return c;
}

// next step's layer-0 addend row  add_out[row] = table[tok] + base[row]  (the embedding folded into the input projection), one wave
__device__ __forceinline__ void write_next_input(const float* __restrict__ table, const float* __restrict__ base, float* __restrict__ add_out,
                                                 long row, int tok, int W, int lane) {
  const float* trow = table + (long)tok * W;
  const float* brow = base + row * W;
  float* orow = add_out + row * W;
  for (int cidx = lane * 4; cidx < W; cidx += 256) {
    const float4 tv = *reinterpret_cast<const float4*>(trow + cidx), bv = *reinterpret_cast<const float4*>(brow + cidx);
    *reinterpret_cast<float4*>(orow + cidx) = make_float4(tv.x + bv.x, tv.y + bv.y, tv.z + bv.z, tv.w + bv.w);
  }
}

// out[0..1] = the packed automaton state after `tok` from the packed state (g0, g1): mode ERROR, the other fields kept, when the automaton
// refuses the token or `refuse` is set (the sampler's empty allowed set); `keep` carries the state unchanged (the beam kernel's finished parent)
__device__ __forceinline__ void smi_advance(int32_t g0, int32_t g1, int tok, const int32_t* __restrict__ tok_info, int32_t* out,
                                            bool refuse = false, bool keep = false) {
  const smi::State os = smi::unpack(g0, g1);
  smi::State nx = os;
  if (!keep && (refuse || !smi::step(os, tok, tok_info[tok], &nx))) { nx = os; nx.mode = smi::ERROR; }
  out[0] = smi::pack0(nx);
  out[1] = smi::pack1(nx);
}

// lane 0 of a sampler row commits token w of this step: a row that had not ended writes x, end_pads / eos_mask at <eos> and folds w into its
// FNV-1a hash (hash may be NULL); w_out is written either way.  Returns whether the row had not ended: the caller's logq and automaton
// updates hang on it.
__device__ __forceinline__ bool commit_token(long b, int w, int step, int eos_id, int64_t* __restrict__ xrow, int64_t* __restrict__ end_pads,
                                             uint8_t* __restrict__ eos_mask, int64_t* __restrict__ hash, int64_t* __restrict__ w_out) {
  const bool open = eos_mask[b] == 0;
  if (open) {
    xrow[step] = w;
    if (w == eos_id) { end_pads[b] = step + 1; eos_mask[b] = 1; }
    if (hash) hash[b] = (int64_t)(((uint64_t)hash[b] ^ (uint64_t)w) * 0x100000001b3ULL);
  }
  w_out[b] = w;
  return open;
}

// the launch statement given, once for either compute dtype (the callers have refused every other value): inside it `T` is the element type
#define DECODE_BY_DTYPE(dtype, ...) do { if ((dtype) == MVAE_BF16) { using T = bf16_t; __VA_ARGS__; } else { using T = float; __VA_ARGS__; } } while (0)
static size_t head_lds_bytes(int dtype, int V, int H) { return (size_t)V * H * (dtype == MVAE_BF16 ? 2 : 4); }

// ------------------------------------------------------------------------------------------- autoregressive sampling step (mosesvae.py:236-253)
// ONE launch per generated token for everything behind the GRU step:  y = decoder_fc(h_top);  p = softmax(y / temp);  w ~ multinomial(p, 1);
// x[~eos, i] = w[~eos];  end_pads[new eos] = i + 1;  eos |= (w == eos)  -- and the NEXT step's layer-0 addend row  add[b] = table[w_b] + base[b]
// (the embedding folded into the input projection, mosesvae.py:239-240).  One wave per batch row; the V x H head sits in LDS once per workgroup.
// Explicit randomness, no hidden state: u(b, i) = hash(seed, i * B + b) / 2^32 (the same counter hash as mvae_dropout_keep); the sampled
// index is the first k with  cumsum_k(p) > u * sum(p)  in the fixed order k = 0 .. V - 1.
template <typename T>
__global__ __launch_bounds__(256) void moses_sample_step_kernel(int B, int V, int H, const T* __restrict__ h, long ldh, const T* __restrict__ wfc, long ldw,
                                                                const float* __restrict__ bias, float inv_temp, uint32_t seed, int step, int eos_id,
                                                                const float* __restrict__ table, int W, const float* __restrict__ base,
                                                                float* __restrict__ add_out, int64_t* __restrict__ x, long x_ld,
                                                                int64_t* __restrict__ end_pads, uint8_t* __restrict__ eos_mask, int64_t* __restrict__ w_out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* ws = reinterpret_cast<T*>(smem_raw);                    // [V][H]
  stage_head(ws, wfc, ldw, V, H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
    const float mine = head_logit(h + (long)b * ldh, ws, bias, inv_temp, V, H, lane);
    const float mx = wave_max(mine);
    const float e = (lane < V) ? __expf(mine - mx) : 0.f;
    float tot;
    const float c = wave_scan(e, lane, &tot);
    const uint32_t hsh = drop_hash_u32(seed, (uint32_t)((long)step * B + b));
    const float u = (float)hsh * (1.0f / 4294967296.0f) * tot;
    const unsigned long long above = __ballot(lane < V && c > u);
    const int w = above ? (int)__builtin_ctzll(above) : V - 1;   // (u rounds up to tot for hsh near 2^32: take the last class)
    if (lane == 0) commit_token(b, w, step, eos_id, x + (long)b * x_ld, end_pads, eos_mask, nullptr, w_out);
    // (the finished rows keep being fed their sampled token, as the reference does)
    write_next_input(table, base, add_out, b, w, W, lane);
  }
}

// The filtered sibling of moses_sample_step_kernel (top-k / nucleus truncation, the sample's log-probability, a running FNV-1a hash of the
// row's tokens; no reference counterpart).  Same shape, and the same fp32 arithmetic in the same order up to the prefix sum of e (the shared
// pieces above).  Class v lives in lane v, so its rank in the order (p desc, id asc) and the mass ranked before it come out of one pass over
// u = 0 .. V-1 of "read lane u (uniform index), compare, add".  keep = (rank < top_k, 0: off) and (before < top_p * sum(p) or rank 0;
// top_p >= 1: off), both on the unfiltered p;  q = keep ? e : 0;  the draw is the first KEPT class with cumsum(q) > u * sum(q).  With both
// filters off q == e and the draw is the existing one.  A row that had not ended before this step adds log(q_w / sum q) to logq[b] and folds
// w into hash[b].
//
// SYNTAX (mvae_moses_sample_syntax_step; the other instantiation compiles none of it): a row that had not ended carries a SMILES automaton
// state gstate[b] (smiles_syntax.hpp).  Lane v decides whether class v is allowed -- the automaton takes it AND the string can still be
// finished in the max_len - 1 - step tokens left after it -- before the softmax: the stabilising max runs over the allowed classes only (a
// dominant illegal logit would underflow every legal one), e = 0 for the others, and the filters rank the legal classes among
// themselves.  The drawn token then advances gstate[b].  Ended rows are neither masked nor advanced.
//
// FORCED (mvae_moses_sample_forced_step; the other instantiations compile none of it): forced[b, step] >= 0 names the token row b writes at
// this step instead of drawing one.  The value is read once per row, wave-uniform.  A forced row skips the head, the softmax, the mask and
// the filter ranking; its token goes through the bookkeeping of a drawn one (x, end_pads / eos_mask, hash, gstate -- ERROR if the
// automaton refuses it --, w_out, the next input row) and adds nothing to logq.  A free row (-1, or a value outside [0, V)) runs the code
// of the other instantiations unchanged.
template <typename T, bool SYNTAX, bool FORCED = false>
__global__ __launch_bounds__(256) void moses_sample_filtered_step_kernel(int B, int V, int H, const T* __restrict__ h, long ldh, const T* __restrict__ wfc,
                                                                         long ldw, const float* __restrict__ bias, float inv_temp, int top_k, float top_p,
                                                                         uint32_t seed, int step, int eos_id, const float* __restrict__ table, int W,
                                                                         const float* __restrict__ base, float* __restrict__ add_out,
                                                                         int64_t* __restrict__ x, long x_ld, int64_t* __restrict__ end_pads,
                                                                         uint8_t* __restrict__ eos_mask, int64_t* __restrict__ w_out,
                                                                         float* __restrict__ logq, int64_t* __restrict__ hash,
                                                                         const int32_t* __restrict__ tok_info, int32_t* __restrict__ gstate, int max_len,
                                                                         const int32_t* __restrict__ forced, long forced_ld) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* ws = reinterpret_cast<T*>(smem_raw);                    // [V][H]
  stage_head(ws, wfc, ldw, V, H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool filtered = top_k > 0 || top_p < 1.f;            // kernel-uniform
  int32_t my_info = 0;
  if constexpr (SYNTAX) my_info = lane < V ? tok_info[lane] : 0;
  for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
    if constexpr (FORCED) {
      const int fw = __builtin_amdgcn_readfirstlane(forced[(long)b * forced_ld + step]);
      if (fw >= 0 && fw < V) {                               // wave-uniform: the whole row is forced
        if (lane == 0) {
          const bool open = commit_token(b, fw, step, eos_id, x + (long)b * x_ld, end_pads, eos_mask, hash, w_out);
          if constexpr (SYNTAX) if (open) smi_advance(gstate[2 * (long)b], gstate[2 * (long)b + 1], fw, tok_info, gstate + 2 * (long)b);
        }
        write_next_input(table, base, add_out, b, fw, W, lane);
        continue;
      }
    }
    const float mine = head_logit(h + (long)b * ldh, ws, bias, inv_temp, V, H, lane);
    bool allowed = lane < V;
    bool live = false;                                       // SYNTAX: the row had not ended before this step (wave-uniform)
    int32_t g0 = 0, g1 = 0;
    if constexpr (SYNTAX) {
      live = eos_mask[b] == 0;
      if (live) {
        g0 = gstate[2 * (long)b];
        g1 = gstate[2 * (long)b + 1];
        smi::State nx;
        allowed = allowed && smi::step(smi::unpack(g0, g1), lane, my_info, &nx) && smi::need(nx) <= max_len - 1 - step;
      }
    }
    const unsigned long long amask = SYNTAX ? __ballot(allowed) : 0ull;
    const float mx = SYNTAX ? wave_max(allowed ? mine : -INFINITY) : wave_max(mine);
    const float e = SYNTAX ? (allowed ? __expf(mine - mx) : 0.f) : ((lane < V) ? __expf(mine - mx) : 0.f);
    float tot;
    float c = wave_scan(e, lane, &tot);
    bool keep = allowed;
    float q = e;
    if (filtered) {
      int rank = 0;
      float before = 0.f;
      for (int u = 0; u < V; ++u) {                          // uniform index: a lane read, not a permute
        const float eu = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), u));
        if (SYNTAX && !((amask >> u) & 1ull)) continue;      // the legal classes are ranked among themselves
        if (eu > e || (eu == e && u < lane)) { ++rank; before += eu; }
      }
      keep = keep && (top_k == 0 || rank < top_k) && (!(top_p < 1.f) || rank == 0 || before < top_p * tot);
      q = keep ? e : 0.f;
      c = wave_scan(q, lane, &tot);
    }
    const uint32_t hsh = drop_hash_u32(seed, (uint32_t)((long)step * B + b));
    const float u = (float)hsh * (1.0f / 4294967296.0f) * tot;
    const unsigned long long kept = __ballot(keep);          // never empty: the rank-0 class is kept
    const unsigned long long above = __ballot(keep && c > u);
    int w = above ? (int)__builtin_ctzll(above) : (kept ? 63 - (int)__builtin_clzll(kept) : V - 1);   // (u rounds up to tot: the last kept class)
    const bool stuck = SYNTAX && live && amask == 0ull;      // an empty allowed set (the feasibility rule excludes it): <eos>, state ERROR
    if (stuck) w = eos_id;
    const float qw = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(q), w));
    if (lane == 0) {
      const bool open = commit_token(b, w, step, eos_id, x + (long)b * x_ld, end_pads, eos_mask, hash, w_out);
      if (open && logq && !stuck) logq[b] += logf(qw / tot);
      if constexpr (SYNTAX) if (open) smi_advance(g0, g1, w, tok_info, gstate + 2 * (long)b, /*refuse=*/stuck);
    }
    write_next_input(table, base, add_out, b, w, W, lane);
  }
}

// The automaton over finished token rows: one thread per row runs smi::step over x[b, 1:] until it reaches END (the <eos> token taken in a
// state that may end).  valid[b] = 1 iff it does; bad_pos[b] = the index of the first refused token (an id outside [0, V) is one), T when
// the row ran out without <eos>, -1 when the row is valid.  eos_id is the only token that ends a row: it counts as EOS whatever the
// table says of it, and another id the table calls EOS is refused.
__global__ __launch_bounds__(64) void smiles_syntax_check_kernel(int B, int T, int V, const int64_t* __restrict__ x, long x_ld,
                                                                 const int32_t* __restrict__ tok_info, int eos_id,
                                                                 uint8_t* __restrict__ valid, int32_t* __restrict__ bad_pos) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  smi::State s{smi::START, 0, smi::NO_PREV, 0, 0};
  int bad = T;
  for (int t = 1; t < T; ++t) {
    const int64_t tok = x[(long)b * x_ld + t];
    smi::State nx;
    if (tok < 0 || tok >= V) { bad = t; break; }
    int32_t info = tok_info[tok];
    if (tok == eos_id) info = smi::C_EOS;
    else if ((info & 0xFF) == smi::C_EOS) info = smi::C_OTHER;
    if (!smi::step(s, (int)tok, info, &nx)) { bad = t; break; }
    s = nx;
    if (s.mode == smi::END) { bad = -1; break; }
  }
  valid[b] = bad < 0 ? 1 : 0;
  if (bad_pos) bad_pos[b] = bad;
}

// The automaton over prefixes (smi::walk): one thread per row walks ids[b, 0 : len_b] from the initial state and writes the packed state it
// reached, smi::need of it and the index of the first refused token (-1: none; the state is then in ERROR and need 0).
__global__ __launch_bounds__(64) void smiles_prefix_state_kernel(int B, int P, int V, const int32_t* __restrict__ ids, long ids_ld,
                                                                 const int32_t* __restrict__ lens, const int32_t* __restrict__ tok_info,
                                                                 int32_t* __restrict__ state, int32_t* __restrict__ need, int32_t* __restrict__ bad_pos) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int n = lens[b];
  n = n < 0 ? 0 : (n > P ? P : n);
  smi::State s;
  const int bad = smi::walk(ids + (long)b * ids_ld, n, V, tok_info, &s);
  state[2 * (long)b] = smi::pack0(s);
  state[2 * (long)b + 1] = smi::pack1(s);
  need[b] = smi::need(s);
  bad_pos[b] = bad;
}

// ------------------------------------------------------------------------------------------- beam-search decoding step (no reference counterpart)
// ONE launch per generated token for everything behind the GRU step, for R = B * K rows (molecule m owns rows m*K .. m*K + K-1, beam k of it
// being row m*K + k):  logp = log_softmax(decoder_fc(h_top));  an active beam r proposes its own top-K tokens at score[r] + logp, a finished
// beam proposes itself once (token pad, score unchanged);  per molecule the best K of those candidates survive, in the total order
// (score desc, parent beam asc, token asc) -- so the K beams of a molecule stay sorted by score.  A NaN candidate counts as -inf.
// A workgroup owns whole molecules (G = max(1, 4 / K) of them per pass, one wave per row), striding over them as the sampler strides over
// rows, so the V x H head is loaded into LDS once per workgroup and each merge stays in LDS.  The launch then writes, per new beam, the
// backpointer record (token, parent) of this step, the new score / finished flag / end (end = step + 1 at the first <eos>, unchanged
// otherwise), the next step's layer-0 addend row table[token] + base[r], and reorders the recurrent state: for every layer, the parent's row
// of the state the GRU step just wrote (half 1 of `state`) is copied into row r of half 0, which that step has already consumed and which
// the next step reads as its h0.  Parents are rows of the same molecule, so a workgroup touches only its own rows.
//
// SYNTAX (mvae_moses_beam_syntax_step; the other instantiation compiles none of it): every row carries a SMILES automaton state gstate[r]
// (smiles_syntax.hpp).  Lane v of an active row decides whether class v may be proposed -- the automaton takes it AND the string can still
// be finished in the max_len - 1 - step tokens left after it, the rule of the sampling launch -- and the row proposes its best
// min(K, allowed) classes.  logp stays the log-softmax over ALL classes: the mask removes candidates, it does not renormalise, so a score is
// still log p(tokens | z).  A molecule may be left with fewer than K candidates: a slot without one gets (-inf, parent 0, pad), its pad
// token puts its automaton in ERROR, which allows nothing, so it stays dead.  Phase 1 reads the pass's old states into LDS, phase 3 writes
// row r's new one: the parent's old state if the parent was finished, else step(parent's old state, token).
//
// FORCED (mvae_moses_beam_forced_step; the other instantiations compile none of it): forced[m, step] >= 0 names the token every hypothesis
// of molecule m takes at this step.  The value is read once per row, wave-uniform.  An active row of such a molecule proposes exactly one
// candidate, the forced token at score + logp[forced] -- unmasked under SYNTAX: the state advances with it in phase 3 and a refused token
// puts it in ERROR --, so the beams that were dead (-inf) stay dead through the forced steps and come alive at the first free one, as they
// do at step 1.  A molecule with -1 (or a value outside [0, V)) runs the code of the other instantiations unchanged.
constexpr int BEAM_KMAX = 16;
template <typename T, bool SYNTAX, bool FORCED = false>
__global__ __launch_bounds__(256) void moses_beam_step_kernel(int B, int K, int V, int H, int NL, T* __restrict__ state, long layer_stride,
                                                              long half_stride, long ldh, const T* __restrict__ wfc, long ldw,
                                                              const float* __restrict__ bias, int step, int eos_id, int pad_id,
                                                              const float* __restrict__ table, int W, const float* __restrict__ base,
                                                              float* __restrict__ add_out, float* __restrict__ score, uint8_t* __restrict__ fin,
                                                              int64_t* __restrict__ ends, int32_t* __restrict__ hist_tok, int32_t* __restrict__ hist_par,
                                                              const int32_t* __restrict__ tok_info, int32_t* __restrict__ gstate, int max_len,
                                                              const int32_t* __restrict__ forced, long forced_ld) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  T* ws = reinterpret_cast<T*>(smem_raw);                    // [V][H]
  __shared__ int32_t old_g[SYNTAX ? 2 * BEAM_KMAX : 1];      // SYNTAX: the automaton states the pass started from
  __shared__ float cand_s[BEAM_KMAX * BEAM_KMAX];            // [row of the pass][rank within the row]
  __shared__ int cand_t[BEAM_KMAX * BEAM_KMAX];
  __shared__ int cand_n[BEAM_KMAX];
  __shared__ float old_s[BEAM_KMAX];
  __shared__ int old_f[BEAM_KMAX];
  __shared__ long old_e[BEAM_KMAX];
  __shared__ float sel_s[BEAM_KMAX];
  __shared__ int sel_p[BEAM_KMAX], sel_t[BEAM_KMAX];
  stage_head(ws, wfc, ldw, V, H);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = K >= 4 ? 1 : 4 / K;                         // molecules per pass: G * K <= 16 rows
  const long R = (long)B * K;
  const T* htop = state + (long)(NL - 1) * layer_stride + half_stride;
  int32_t my_info = 0;
  if constexpr (SYNTAX) my_info = lane < V ? tok_info[lane] : 0;
  for (int m0 = blockIdx.x * G; m0 < B; m0 += gridDim.x * G) {
    const int nm = (B - m0 < G) ? B - m0 : G, nr = nm * K;
    const long r0 = (long)m0 * K;
    // 1. each row's candidates, sorted by (score desc, token asc)
    for (int lr = wave; lr < nr; lr += 4) {
      const long r = r0 + lr;
      float s = score[r];
      if (s != s) s = -INFINITY;
      const bool done = fin[r] != 0;
      if (lane == 0) { old_s[lr] = s; old_f[lr] = done; old_e[lr] = (long)ends[r]; }
      smi::State gs{};
      if constexpr (SYNTAX) {
        const int32_t g0 = gstate[2 * r], g1 = gstate[2 * r + 1];
        if (lane == 0) { old_g[2 * lr] = g0; old_g[2 * lr + 1] = g1; }
        gs = smi::unpack(g0, g1);
      }
      if (done) {
        if (lane == 0) { cand_s[lr * K] = s; cand_t[lr * K] = pad_id; cand_n[lr] = 1; }
        continue;                                            // wave-uniform
      }
      const float mine = head_logit(htop + r * ldh, ws, bias, 1.f, V, H, lane);
      const float mx = wave_max(mine);
      const float se = wave_sum(lane < V ? expf(mine - mx) : 0.f);
      float c = s + (mine - (mx + logf(se)));
      if (c != c) c = -INFINITY;
      if constexpr (FORCED) {
        const int fw = __builtin_amdgcn_readfirstlane(forced[(long)(m0 + lr / K) * forced_ld + step]);
        if (fw >= 0 && fw < V) {                             // wave-uniform: the one candidate of a forced row
          const float cf = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), fw));
          if (lane == 0) { cand_s[lr * K] = cf; cand_t[lr * K] = fw; cand_n[lr] = 1; }
          continue;
        }
      }
      bool avail = lane < V;
      int nc = K;                                            // K <= V: an available class is always left
      if constexpr (SYNTAX) {
        smi::State nx;
        avail = avail && smi::step(gs, lane, my_info, &nx) && smi::need(nx) <= max_len - 1 - step;
        const int na = (int)__builtin_popcountll(__ballot(avail));
        nc = na < K ? na : K;                                // wave-uniform; 0 for a row in ERROR (a dead slot)
      }
      for (int j = 0; j < nc; ++j) {
        const float best = wave_max(avail ? c : -INFINITY);
        const unsigned long long hit = __ballot(avail && c == best);
        const int v = hit ? (int)__builtin_ctzll(hit) : 0;
        if (lane == v) avail = false;
        if (lane == 0) { cand_s[lr * K + j] = best; cand_t[lr * K + j] = v; }
      }
      if (lane == 0) cand_n[lr] = nc;
    }
    __syncthreads();
    // 2. per molecule, a K-way merge of its K sorted candidate lists (lane p = the head of parent p's list): the best K survive
    if (wave < nm) {
      const int g = wave;
      int ptr = 0;
      for (int j = 0; j < K; ++j) {
        const bool valid = lane < K && ptr < cand_n[g * K + lane];
        const int ci = (g * K + (lane < K ? lane : 0)) * K + (ptr < K ? ptr : 0);
        const float key = valid ? cand_s[ci] : -INFINITY;
        const int tk = valid ? cand_t[ci] : pad_id;
        const float best = wave_max(key);
        const unsigned long long hit = __ballot(valid && key == best);   // empty only under SYNTAX: a slot left without a candidate
        const int p = hit ? (int)__builtin_ctzll(hit) : 0;
        const int tok = __shfl(tk, p, 64);
        if (lane == p) ++ptr;
        if (lane == 0) { sel_s[g * K + j] = best; sel_p[g * K + j] = p; sel_t[g * K + j] = hit ? tok : pad_id; }
      }
    }
    __syncthreads();
    // 3. the new beams: bookkeeping, backpointers, next input rows, recurrent state reordered from the parents
    for (int lr = wave; lr < nr; lr += 4) {
      const long r = r0 + lr;
      const int p = sel_p[lr], lp = (lr / K) * K + p;
      const bool pdone = old_f[lp] != 0;
      const int tok = pdone ? pad_id : sel_t[lr];
      if (lane == 0) {
        score[r] = sel_s[lr];
        fin[r] = (pdone || tok == eos_id) ? 1 : 0;
        ends[r] = (!pdone && tok == eos_id) ? (int64_t)(step + 1) : (int64_t)old_e[lp];
        hist_tok[(long)step * R + r] = tok;
        hist_par[(long)step * R + r] = p;
        if constexpr (SYNTAX)                                // (a finished parent's state is carried unchanged)
          smi_advance(old_g[2 * lp], old_g[2 * lp + 1], tok, tok_info, gstate + 2 * r, /*refuse=*/false, /*keep=*/pdone);
      }
      write_next_input(table, base, add_out, r, tok, W, lane);
      const long src_row = r0 + lp;
      for (int l = 0; l < NL; ++l) {
        const T* src = state + (long)l * layer_stride + half_stride + src_row * ldh;
        T* dst = state + (long)l * layer_stride + r * ldh;
        if (((H * (int)sizeof(T)) & 15) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
          const int n16 = H * (int)sizeof(T) / 16;
          for (int i = lane; i < n16; i += 64) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        } else {
          for (int i = lane; i < H; i += 64) dst[i] = src[i];
        }
      }
    }
    __syncthreads();                                         // LDS is reused by the next pass
  }
}
// The K hypotheses of every molecule from the backpointer record, already in score order: ids [B, K, max_len] int64 (bos first, the
// chosen tokens after it -- pad after each end, as finished beams only ever append pad).  One thread per (molecule, beam).
__global__ __launch_bounds__(256) void moses_beam_finalize_kernel(int B, int K, int max_len, int bos_id, const int32_t* __restrict__ hist_tok,
                                                                  const int32_t* __restrict__ hist_par, const int64_t* __restrict__ ends,
                                                                  const float* __restrict__ score, int64_t* __restrict__ ids,
                                                                  int64_t* __restrict__ ends_out, float* __restrict__ score_out) {
  const long R = (long)B * K;
  for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
    const long m0 = (r / K) * K;
    int k = (int)(r - m0);
    int64_t* out = ids + r * max_len;
    for (int t = max_len - 1; t >= 1; --t) {
      const long i = (long)t * R + m0 + k;
      out[t] = hist_tok[i];
      k = hist_par[i];
    }
    out[0] = bos_id;
    if (ends_out) ends_out[r] = ends[r];
    if (score_out) score_out[r] = score[r];
  }
}

// ------------------------------------------------------------------------------------------- launchers
// what the four sampling entries refuse (MVAE_ERR_INVALID); mvae_moses_sample_step has no filters and passes top_k = 0, top_p = 1
static bool sample_filtered_args_ok(int dtype, int B, int V, int H, const void* h_top, const void* w_fc, float temp, int top_k, float top_p, int step,
                                    const float* table, int W, const float* base, float* add_out, int64_t* x, int64_t* end_pads, uint8_t* eos_mask,
                                    int64_t* w_out) {
  if (!h_top || !w_fc || !table || !base || !add_out || !x || !end_pads || !eos_mask || !w_out) return false;
  if (dtype != MVAE_F32 && dtype != MVAE_BF16) return false;
  if (B < 1 || V < 1 || V > 64 || H < 1 || (W & 3) || W < 4 || !(temp > 0.f) || step < 0) return false;
  if (top_k < 0 || top_k > V || !(top_p > 0.f)) return false;                 // (a NaN top_p fails the comparison)
  return true;
}

// the launch behind mvae_moses_sample_filtered_step (SYNTAX = false), mvae_moses_sample_syntax_step (true) and, with FORCED and either
// SYNTAX, mvae_moses_sample_forced_step; the callers have checked
template <bool SYNTAX, bool FORCED = false>
static int sample_filtered_launch(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                  float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                  const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                  int64_t* w_out, float* logq, int64_t* hash, const int32_t* tok_info, int32_t* gstate, int max_len, void* stream,
                                  const int32_t* forced = nullptr, int64_t forced_ld = 0) {
  const size_t lds = head_lds_bytes(dtype, V, H);
  if (lds > 160 * 1024) return MVAE_ERR_UNSUPPORTED;                 // the head must fit the CU's LDS, as in mvae_moses_sample_step
  // a head above the default 64 KB dynamic-LDS limit: both dtypes of the kernel are opted in
  if (lds > 64 * 1024)
    MVAE_CHECK_HIP((lds_opt_in<moses_sample_filtered_step_kernel<float, SYNTAX, FORCED>, moses_sample_filtered_step_kernel<bf16_t, SYNTAX, FORCED>>(160 * 1024)));
  if (top_p > 1.f) top_p = 1.f;                                       // larger values mean off
  int blocks = (B + 3) / 4; if (blocks > 1024) blocks = 1024;
  DECODE_BY_DTYPE(dtype, hipLaunchKernelGGL((moses_sample_filtered_step_kernel<T, SYNTAX, FORCED>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, B, V, H,
                                     (const T*)h_top, (long)ldh, (const T*)w_fc, (long)ldw, bias, 1.f / temp, top_k, top_p, seed, step, eos_id, table,
                                     W, base, add_out, x, (long)x_ld, end_pads, eos_mask, w_out, logq, hash, tok_info, gstate, max_len, forced,
                                     (long)forced_ld));
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

// what mvae_moses_beam_step refuses (MVAE_ERR_INVALID), shared with the syntax and forced entries
static bool beam_step_args_ok(int dtype, int B, int K, int V, int H, int layers, const void* state, int64_t ldh, const void* w_fc, int64_t ldw, int step,
                              int eos_id, int pad_id, const float* table, int W, const float* base, const float* add_out, const float* score,
                              const uint8_t* fin, const int64_t* ends, const int32_t* hist_tok, const int32_t* hist_par) {
  if (!state || !w_fc || !table || !base || !add_out || !score || !fin || !ends || !hist_tok || !hist_par) return false;
  if (dtype != MVAE_F32 && dtype != MVAE_BF16) return false;
  if (B < 1 || V < 1 || H < 1 || layers < 1 || layers > MVAE_MAX_LAYERS || ldh < H || ldw < H || (W & 3) || W < 4 || step < 1) return false;
  if (K < 1 || K > BEAM_KMAX || K > V) return false;
  if (eos_id < 0 || eos_id >= V || pad_id < 0 || pad_id >= V) return false;
  if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(add_out)) & 15) return false;
  return true;
}

// the launch behind mvae_moses_beam_step (SYNTAX = false), mvae_moses_beam_syntax_step (true) and, with FORCED and either SYNTAX,
// mvae_moses_beam_forced_step; the callers have checked
template <bool SYNTAX, bool FORCED = false>
static int beam_step_launch(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride, int64_t ldh,
                            const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table, int W,
                            const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok, int32_t* hist_par,
                            const int32_t* tok_info, int32_t* gstate, int max_len, void* stream, const int32_t* forced = nullptr,
                            int64_t forced_ld = 0) {
  if (V > 64) return MVAE_ERR_UNSUPPORTED;                           // one class per lane
  const size_t lds = head_lds_bytes(dtype, V, H);
  constexpr size_t lds_cap = 156 * 1024;                             // the CU's 160 KB less the kernel's static candidate arrays
  if (lds > lds_cap) return MVAE_ERR_UNSUPPORTED;
  if (lds > 64 * 1024)
    MVAE_CHECK_HIP((lds_opt_in<moses_beam_step_kernel<float, SYNTAX, FORCED>, moses_beam_step_kernel<bf16_t, SYNTAX, FORCED>>((int)lds_cap)));
  const int G = K >= 4 ? 1 : 4 / K;
  int blocks = (B + G - 1) / G; if (blocks > 1024) blocks = 1024;
  DECODE_BY_DTYPE(dtype, hipLaunchKernelGGL((moses_beam_step_kernel<T, SYNTAX, FORCED>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, B, K, V, H, layers,
                                     (T*)state, (long)layer_stride, (long)half_stride, (long)ldh, (const T*)w_fc, (long)ldw, bias, step, eos_id, pad_id,
                                     table, W, base, add_out, score, fin, ends, hist_tok, hist_par, tok_info, gstate, max_len, forced,
                                     (long)forced_ld));
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

// ------------------------------------------------------------------------------------------- extern "C" surface
extern "C" {

int mvae_moses_sample_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, float temp,
                           uint32_t seed, int step, int eos_id, const float* table, int W, const float* base, float* add_out, int64_t* x, int64_t x_ld,
                           int64_t* end_pads, uint8_t* eos_mask, int64_t* w_out, void* stream) {
  if (!sample_filtered_args_ok(dtype, B, V, H, h_top, w_fc, temp, 0, 1.f, step, table, W, base, add_out, x, end_pads, eos_mask, w_out))
    return MVAE_ERR_INVALID;
  const size_t lds = head_lds_bytes(dtype, V, H);
  if (lds > 160 * 1024) return MVAE_ERR_UNSUPPORTED;                 // the head must fit the CU's LDS (fp32, H = 512: V <= 80; bf16: V <= 64 by the check above)
  if (lds > 64 * 1024) MVAE_CHECK_HIP((lds_opt_in<moses_sample_step_kernel<float>, moses_sample_step_kernel<bf16_t>>(160 * 1024)));
  int blocks = (B + 3) / 4; if (blocks > 1024) blocks = 1024;
  DECODE_BY_DTYPE(dtype, hipLaunchKernelGGL((moses_sample_step_kernel<T>), dim3(blocks), dim3(256), lds, (hipStream_t)stream, B, V, H, (const T*)h_top,
                                     (long)ldh, (const T*)w_fc, (long)ldw, bias, 1.f / temp, seed, step, eos_id, table, W, base, add_out, x,
                                     (long)x_ld, end_pads, eos_mask, w_out));
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_moses_sample_filtered_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                    float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                    const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                    int64_t* w_out, float* logq, int64_t* hash, void* stream) {
  if (!sample_filtered_args_ok(dtype, B, V, H, h_top, w_fc, temp, top_k, top_p, step, table, W, base, add_out, x, end_pads, eos_mask, w_out))
    return MVAE_ERR_INVALID;
  return sample_filtered_launch<false>(dtype, B, V, H, h_top, ldh, w_fc, ldw, bias, temp, top_k, top_p, seed, step, eos_id, table, W, base, add_out,
                                       x, x_ld, end_pads, eos_mask, w_out, logq, hash, nullptr, nullptr, 0, stream);
}

int mvae_moses_sample_syntax_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                  float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                  const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                  int64_t* w_out, float* logq, int64_t* hash, const int32_t* tok_info, int32_t* gstate, int max_len, void* stream) {
  if (!sample_filtered_args_ok(dtype, B, V, H, h_top, w_fc, temp, top_k, top_p, step, table, W, base, add_out, x, end_pads, eos_mask, w_out))
    return MVAE_ERR_INVALID;
  if (!tok_info || !gstate || max_len < 3 || step < 1 || step >= max_len) return MVAE_ERR_INVALID;
  if (eos_id < 0 || eos_id >= V) return MVAE_ERR_INVALID;            // the empty-set fallback emits it
  return sample_filtered_launch<true>(dtype, B, V, H, h_top, ldh, w_fc, ldw, bias, temp, top_k, top_p, seed, step, eos_id, table, W, base, add_out,
                                      x, x_ld, end_pads, eos_mask, w_out, logq, hash, tok_info, gstate, max_len, stream);
}

int mvae_moses_sample_forced_step(int dtype, int B, int V, int H, const void* h_top, int64_t ldh, const void* w_fc, int64_t ldw, const float* bias,
                                  float temp, int top_k, float top_p, uint32_t seed, int step, int eos_id, const float* table, int W,
                                  const float* base, float* add_out, int64_t* x, int64_t x_ld, int64_t* end_pads, uint8_t* eos_mask,
                                  int64_t* w_out, float* logq, int64_t* hash, const int32_t* tok_info, int32_t* gstate, int max_len,
                                  const int32_t* forced, int64_t forced_ld, void* stream) {
  if (!sample_filtered_args_ok(dtype, B, V, H, h_top, w_fc, temp, top_k, top_p, step, table, W, base, add_out, x, end_pads, eos_mask, w_out))
    return MVAE_ERR_INVALID;
  if (!forced || forced_ld <= step) return MVAE_ERR_INVALID;
  if (!tok_info != !gstate) return MVAE_ERR_INVALID;                 // both or neither: NULL turns the automaton off
  if (!tok_info)
    return sample_filtered_launch<false, true>(dtype, B, V, H, h_top, ldh, w_fc, ldw, bias, temp, top_k, top_p, seed, step, eos_id, table, W, base,
                                               add_out, x, x_ld, end_pads, eos_mask, w_out, logq, hash, nullptr, nullptr, 0, stream, forced, forced_ld);
  if (max_len < 3 || step < 1 || step >= max_len) return MVAE_ERR_INVALID;
  if (eos_id < 0 || eos_id >= V) return MVAE_ERR_INVALID;
  return sample_filtered_launch<true, true>(dtype, B, V, H, h_top, ldh, w_fc, ldw, bias, temp, top_k, top_p, seed, step, eos_id, table, W, base,
                                            add_out, x, x_ld, end_pads, eos_mask, w_out, logq, hash, tok_info, gstate, max_len, stream, forced, forced_ld);
}

int mvae_smiles_prefix_state(int B, int P, int V, const int32_t* ids, int64_t ids_ld, const int32_t* lens, const int32_t* tok_info, int32_t* state,
                             int32_t* need, int32_t* bad_pos, void* stream) {
  if (!ids || !lens || !tok_info || !state || !need || !bad_pos || B < 1 || P < 0 || V < 1 || V > 64 || ids_ld < P) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_prefix_state_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, P, V, ids, (long)ids_ld, lens, tok_info,
                     state, need, bad_pos);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_smiles_syntax_check(int B, int T, int V, const int64_t* x, int64_t x_ld, const int32_t* tok_info, int eos_id, uint8_t* valid, int32_t* bad_pos,
                             void* stream) {
  if (!x || !tok_info || !valid || B < 1 || T < 1 || V < 1 || V > 64 || x_ld < T || eos_id < 0 || eos_id >= V) return MVAE_ERR_INVALID;
  hipLaunchKernelGGL(smiles_syntax_check_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, T, V, x, (long)x_ld, tok_info, eos_id, valid, bad_pos);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

int mvae_moses_beam_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride, int64_t ldh,
                         const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table, int W,
                         const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok, int32_t* hist_par,
                         void* stream) {
  if (!beam_step_args_ok(dtype, B, K, V, H, layers, state, ldh, w_fc, ldw, step, eos_id, pad_id, table, W, base, add_out, score, fin, ends, hist_tok,
                         hist_par))
    return MVAE_ERR_INVALID;
  return beam_step_launch<false>(dtype, B, K, V, H, layers, state, layer_stride, half_stride, ldh, w_fc, ldw, bias, step, eos_id, pad_id, table, W,
                                 base, add_out, score, fin, ends, hist_tok, hist_par, nullptr, nullptr, 0, stream);
}

int mvae_moses_beam_syntax_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride,
                                int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table,
                                int W, const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok,
                                int32_t* hist_par, const int32_t* tok_info, int32_t* gstate, int max_len, void* stream) {
  if (!beam_step_args_ok(dtype, B, K, V, H, layers, state, ldh, w_fc, ldw, step, eos_id, pad_id, table, W, base, add_out, score, fin, ends, hist_tok,
                         hist_par))
    return MVAE_ERR_INVALID;
  if (!tok_info || !gstate || max_len < 3 || step < 1 || step >= max_len) return MVAE_ERR_INVALID;
  if (eos_id < 0 || eos_id >= V) return MVAE_ERR_INVALID;
  return beam_step_launch<true>(dtype, B, K, V, H, layers, state, layer_stride, half_stride, ldh, w_fc, ldw, bias, step, eos_id, pad_id, table, W,
                                base, add_out, score, fin, ends, hist_tok, hist_par, tok_info, gstate, max_len, stream);
}

int mvae_moses_beam_forced_step(int dtype, int B, int K, int V, int H, int layers, void* state, int64_t layer_stride, int64_t half_stride,
                                int64_t ldh, const void* w_fc, int64_t ldw, const float* bias, int step, int eos_id, int pad_id, const float* table,
                                int W, const float* base, float* add_out, float* score, uint8_t* fin, int64_t* ends, int32_t* hist_tok,
                                int32_t* hist_par, const int32_t* tok_info, int32_t* gstate, int max_len, const int32_t* forced, int64_t forced_ld,
                                void* stream) {
  if (!beam_step_args_ok(dtype, B, K, V, H, layers, state, ldh, w_fc, ldw, step, eos_id, pad_id, table, W, base, add_out, score, fin, ends, hist_tok,
                         hist_par))
    return MVAE_ERR_INVALID;
  if (!forced || forced_ld <= step) return MVAE_ERR_INVALID;
  if (!tok_info != !gstate) return MVAE_ERR_INVALID;                 // both or neither: NULL turns the automaton off
  if (!tok_info)
    return beam_step_launch<false, true>(dtype, B, K, V, H, layers, state, layer_stride, half_stride, ldh, w_fc, ldw, bias, step, eos_id, pad_id,
                                         table, W, base, add_out, score, fin, ends, hist_tok, hist_par, nullptr, nullptr, 0, stream, forced, forced_ld);
  if (max_len < 3 || step >= max_len) return MVAE_ERR_INVALID;
  return beam_step_launch<true, true>(dtype, B, K, V, H, layers, state, layer_stride, half_stride, ldh, w_fc, ldw, bias, step, eos_id, pad_id, table,
                                      W, base, add_out, score, fin, ends, hist_tok, hist_par, tok_info, gstate, max_len, stream, forced, forced_ld);
}

int mvae_moses_beam_finalize(int B, int K, int max_len, int bos_id, const int32_t* hist_tok, const int32_t* hist_par, const int64_t* ends,
                             const float* score, int64_t* ids, int64_t* ends_out, float* score_out, void* stream) {
  if (!hist_tok || !hist_par || !ends || !score || !ids || B < 1 || K < 1 || K > BEAM_KMAX || max_len < 1) return MVAE_ERR_INVALID;
  long blocks = ((long)B * K + 255) / 256; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(moses_beam_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, B, K, max_len, bos_id, hist_tok,
                     hist_par, ends, score, ids, ends_out, score_out);
  MVAE_CHECK_HIP(hipGetLastError());
  return MVAE_OK;
}

}  // extern "C"
